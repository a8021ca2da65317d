"""The scan and session kernels, return_perm, WindowJob and the Server routing
on the device.  Every comparison is exact against the pure-Python oracle of
window_common (int64 bit patterns, order keys where rows may tie), but for
the one general-f64 sum, whose bound is derived in its test.  Sizes come
from the extension (ops.seg_scan_caps): S rows per tile, C tiles per trip
of the carry pass."""

import math
import random

import pytest
import torch

import group_common as gc
import window_common as wc
from mapreduce_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PS, PCH = ops.SEG_SCAN_TILE, ops.SEG_CARRY_CHUNK
GPC = (ops.GROUP_TILE, ops.GROUP_RANK_MAX)


@pytest.fixture(scope="module")
def caps():
    return ops.seg_scan_caps()


def test_caps_come_from_the_extension(caps):
    assert caps == tuple(ops.ext().seg_scan_caps()) == (PS, PCH)
    S, C = caps
    assert S == 256 * 8 and C % 256 == 0


# parametrised by name over the Python constants; the first assertion checks
# they are the extension's, so the ids name the layouts the device runs
@pytest.mark.parametrize("name", sorted(wc.layouts(PS)))
def test_scan_matches_oracle(name, caps):
    assert caps == (PS, PCH)
    lens = wc.layouts(PS)[name]
    for family, fam_ops in wc.FAMILIES.items():
        keys, vals = wc.layout_data(PS, name, family)
        kbuf, vbuf, kv, vv = gc.baited(keys, vals, DEV)
        k0, v0 = kbuf.clone(), vbuf.view(torch.int64).clone()
        lo = vbuf.data_ptr()
        for op in fam_ops:
            out = ops.scan_by_key_sorted(kv, vv, op)
            assert out.dtype == vals.dtype and out.numel() == vals.numel()
            assert gc.to_bits(out) == wc.expected_scan(PS, name, family,
                                                       op), (family, op)
            if lens:
                assert not lo <= out.data_ptr() < lo + vbuf.numel() * 8
        assert torch.equal(kbuf, k0)
        assert torch.equal(vbuf.view(torch.int64), v0)


def test_carry_pass_takes_a_second_chunk(caps):
    """(C + 1) * S rows in three long segments.  i64 only, so the oracle
    walk stays short: wrapping sums and the running maximum."""
    S, C = caps
    lens = wc.second_chunk_layout(S, C)
    n = sum(lens)
    assert n == (C + 1) * S
    keys = wc.layout_keys(lens).to(DEV)
    g = torch.Generator().manual_seed(5)
    vals = torch.randint(-2 ** 63, 2 ** 63 - 1, (n,), dtype=torch.int64,
                         generator=g)
    dv = vals.to(DEV)
    tf, ta = ops.ext().seg_scan_reduce(keys, dv, 0, False)
    assert tf.numel() == C + 1
    assert gc.to_bits(ops.scan_by_key_sorted(keys, dv, "sum")) == \
        wc.oracle_scan(lens, vals, "sum")
    assert gc.to_bits(ops.scan_by_key_sorted(keys, dv, "max")) == \
        wc.oracle_scan(lens, vals, "max")


def test_general_f64_sum_within_the_derived_bound(caps):
    """Any summation order of m terms is within (m - 1) u sum|v| + O(u^2)
    of the exact sum, u = 2^-53; the bound asserted is twice that first
    order, m 2^-52 sum|v|, against math.fsum of the prefix."""
    S, _ = caps
    rng = random.Random(9)
    lens = []
    while sum(lens) < S + 400:
        lens.append(rng.randrange(1, 400))
    lens = tuple(lens)
    n = sum(lens)
    vals = wc.values("f64_general", n)
    keys = wc.layout_keys(lens)
    got = ops.scan_by_key_sorted(keys.to(DEV), vals.to(DEV), "sum").cpu()
    got = got.tolist()
    v = vals.tolist()
    worst = 0.0
    i = 0
    for m in lens:
        for j in range(1, m + 1):
            pre = v[i:i + j]
            bound = j * 2.0 ** -52 * math.fsum(abs(x) for x in pre)
            err = abs(got[i + j - 1] - math.fsum(pre))
            worst = max(worst, err / bound if bound else err)
            assert err <= bound, (i, j, err, bound)
        i += m
    print(f"general f64 sum: worst error / bound = {worst:.3g}")


def test_scan_host_checks():
    k = torch.arange(40, dtype=torch.int64, device=DEV) // 3
    v = torch.arange(40, dtype=torch.int64, device=DEV)
    e = ops.ext()
    with pytest.raises(TypeError, match="int64 or float64"):
        ops.scan_by_key_sorted(k, v.to(torch.int32))
    with pytest.raises(RuntimeError, match="keys must be int64"):
        ops.scan_by_key_sorted(k.to(torch.int32), v)
    with pytest.raises(RuntimeError, match="one value per key"):
        ops.scan_by_key_sorted(k, v[:-1])
    with pytest.raises(RuntimeError, match="GPU"):
        ops.scan_by_key_sorted(k, v.cpu())
    with pytest.raises(RuntimeError, match="GPU"):
        ops.scan_by_key_sorted(k.cpu(), v)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.scan_by_key_sorted(k, torch.stack([v, v], 1)[:, 0])
    with pytest.raises(ValueError, match="op must be"):
        ops.scan_by_key_sorted(k, v, "prod")
    with pytest.raises(RuntimeError, match="op must be"):
        e.scan_by_key_sorted(k, v, 3, False)
    tf, ta = e.seg_scan_reduce(k, v, 0, False)
    with pytest.raises(RuntimeError, match="one entry per tile"):
        e.seg_scan_apply(k, v, torch.cat([tf, tf]), torch.cat([ta, ta]), 0,
                         False)
    with pytest.raises(RuntimeError, match="one entry per tile"):
        e.seg_scan_carry(tf, ta[:0], 0, False)
    # n == 0 runs the same checks and returns an empty column
    out = ops.scan_by_key_sorted(k[:0], v[:0].view(torch.float64), "min")
    assert out.numel() == 0 and out.dtype == torch.float64 and out.is_cuda
    with pytest.raises(RuntimeError, match="GPU"):
        ops.scan_by_key_sorted(k[:0], v[:0].cpu())
    with pytest.raises(RuntimeError, match="keys must be int64"):
        ops.scan_by_key_sorted(k[:0].to(torch.int32), v[:0])


# ------------------------------------------------------------- return_perm

@pytest.mark.parametrize("family", ["random_i64", "two_valued", "f64"])
@pytest.mark.parametrize("name", sorted(gc.cases(GPC)))
def test_return_perm(name, family, monkeypatch):
    keys, vals, off = gc.case_data(GPC, name, family)
    _, exp_bits = gc.expected(GPC, name, family)
    exp_perm = wc.oracle_perm(off, vals)
    kbuf, vbuf, kv, vv = gc.baited(keys, vals, DEV)
    k0, v0 = kbuf.clone(), vbuf.view(torch.int64).clone()
    for two_sort in (False, True):
        if two_sort:
            monkeypatch.setenv("MR_GROUP_TWO_SORT", "1")
        else:
            monkeypatch.delenv("MR_GROUP_TWO_SORT", raising=False)
        plain = ops.sort_values_in_groups(kv, vv)
        assert isinstance(plain, torch.Tensor)
        out, perm = ops.sort_values_in_groups(kv, vv, return_perm=True)
        assert out.dtype == vals.dtype and perm.dtype == torch.int64
        assert perm.numel() == vals.numel()
        assert perm.cpu().tolist() == exp_perm
        assert gc.to_bits(out) == exp_bits == gc.to_bits(plain)
        if off[1:]:
            assert gc.to_bits(vv.index_select(0, perm)) == exp_bits
    assert torch.equal(kbuf, k0) and torch.equal(vbuf.view(torch.int64), v0)


# ---------------------------------------------------------------- sessions

def test_session_flags_edges(caps):
    S, _ = caps
    cases = {
        "gap_exact_and_plus_one": ([7, 7, 7, 7], [0, 10, 21, 31], 10),
        "full_span": ([1, 1], [gc.I64_MIN, gc.I64_MAX], gc.I64_MAX),
        "half_span": ([1, 1, 1], [gc.I64_MIN, -1, gc.I64_MAX - 1],
                      gc.I64_MAX),
        "gap_zero_duplicates": ([3, 3, 3, 3], [5, 5, 6, 6], 0),
        "key_change_equal_times": ([3, 3, 4, 4], [9, 9, 9, 9], 100),
        # one key over S + 2 rows one second apart but for the step into
        # row S: a session boundary on a tile edge
        "tile_edge": ([5] * (S + 2),
                      list(range(S)) + [S + 10, S + 11], 10),
    }
    for name, (keys, times, gap) in cases.items():
        flags = wc.oracle_session_flags(keys, times, gap)
        k = torch.tensor(keys, dtype=torch.int64, device=DEV)
        t = torch.tensor(times, dtype=torch.int64, device=DEV)
        assert ops.session_flags(k, t, gap).cpu().tolist() == flags, name
        sk, so = ops.group_sessions(k, t, gap)
        ek, eo = wc.oracle_sessions(keys, times, gap)
        assert sk.cpu().tolist() == ek and so.cpu().tolist() == eo, name
    assert wc.oracle_session_flags(*cases["full_span"]) == [1, 1]
    assert wc.oracle_session_flags(*cases["gap_exact_and_plus_one"]) == [
        1, 0, 1, 0]
    assert wc.oracle_sessions(*cases["tile_edge"])[1] == [0, S, S + 2]
    k = torch.zeros(3, dtype=torch.int64, device=DEV)
    with pytest.raises(TypeError, match="int64"):
        ops.session_flags(k, k.to(torch.float64), 5)
    with pytest.raises(ValueError, match="gap"):
        ops.session_flags(k, k, 2 ** 63)
    with pytest.raises(RuntimeError, match="one time per key"):
        ops.session_flags(k, k[:-1], 1)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.session_flags(k, k.cpu(), 1)


# --------------------------------------------------------------- WindowJob

def check_result(res, keys, order, vals):
    exp = wc.job_oracle(keys, order, vals)
    got = wc.job_lists(res)
    assert got == exp and len(exp[0]) > 600
    uk, off, _, _ = exp
    lens = tuple(b - a for a, b in zip(off, off[1:]))
    assert max(lens) > PS   # a key longer than a tile of either kernel
    f64 = vals.dtype == torch.float64
    hv = res.values.cpu()
    for op in (("min", "max") if f64 else wc.OPS):
        run = res.scan(op).cpu()
        want = wc.oracle_scan(lens, hv, op)
        assert gc.okeys(run) == [gc.okey(b, f64) for b in want], op
        if not f64:
            assert gc.to_bits(run) == want
    if order.dtype == torch.int64:
        times = res.order.cpu().tolist()
        gap = 3000
        rows, per_key = wc.oracle_job_sessions(got, times, gap)
        ses = res.sessions(gap)
        assert list(zip(gc.to_bits(ses.keys), ses.start.cpu().tolist(),
                        ses.end.cpu().tolist(),
                        ses.count.cpu().tolist())) == rows
        assert ses.per_key.cpu().tolist() == per_key
        if not f64:
            slens = tuple(r[3] for r in rows)
            assert gc.to_bits(res.scan("sum", within_sessions=gap)) == \
                wc.oracle_scan(slens, hv, "sum")


@pytest.fixture(scope="module")
def rows():
    """5 000 rows over 700 keys plus one hot key of S + 100 rows, with ties
    in the order column: i64 order and values, and f64 order and values."""
    return {f64: wc.make_rows(43, 5000, 700, f64, f64, hot=PS + 100)
            for f64 in (False, True)}


@pytest.mark.parametrize("f64", [False, True])
def test_window_job_on_device(f64, rows):
    from mapreduce_amd.gpu.window import WindowJob

    keys, order, vals = rows[f64]
    dk, do, dv = (t.to(DEV) for t in rows[f64])
    keep = [t.clone() for t in (dk, do.view(torch.int64),
                                dv.view(torch.int64))]
    res = WindowJob(DEV).run(dk, do, dv)
    check_result(res, keys, order, vals)
    assert res.order.dtype == order.dtype and res.values.dtype == vals.dtype
    assert torch.equal(dk, keep[0])
    assert torch.equal(do.view(torch.int64), keep[1])
    assert torch.equal(dv.view(torch.int64), keep[2])
    # without a value column
    res = WindowJob(DEV).run(dk, do)
    assert wc.job_lists(res) == wc.job_oracle(keys, order)


@pytest.fixture()
def rccl_ws1(monkeypatch):
    assert torch.cuda.is_available()
    import torch.distributed as td

    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", "29597")  # this file's own
    torch.cuda.set_device(0)
    td.init_process_group("nccl", rank=0, world_size=1,
                          device_id=torch.device("cuda", 0))
    monkeypatch.setenv("MR_FORCE_COLLECTIVE", "1")
    try:
        yield td
    finally:
        td.destroy_process_group()


def test_window_job_through_real_rccl(rccl_ws1, rows):
    """Every collective call site of the job — the count exchange and the
    three all-to-alls — on RCCL at world 1 (self-exchange)."""
    from mapreduce_amd.gpu import dist as dx
    from mapreduce_amd.gpu.window import WindowJob

    assert dx.force_collectives()
    keys, order, vals = rows[False]
    res = WindowJob(DEV).run(keys.to(DEV), order.to(DEV), vals.to(DEV))
    check_result(res, keys, order, vals)


# --------------------------------------------------------------- the Server

def test_sessions_on_hardware(monkeypatch):
    import importlib

    import mapreduce_amd.examples.sessions as se
    from mapreduce_amd import job as jobmod
    from mapreduce_amd import run_local
    from mapreduce_amd.parallel.coord import LocalCoordinator
    from mapreduce_amd.server import Server

    def fresh():
        importlib.reload(se)
        jobmod._module_cache.clear()
        jobmod._inited.clear()

    args = {"seed": 9, "n": 6000, "nusers": 40, "splits": 4, "parts": 4}
    roles = ("taskfn", "mapfn", "partitionfn", "reducefn", "finalfn")
    monkeypatch.setenv("MR_GPU_TIER", "off")
    fresh()
    srv = run_local({"fns": {r: se for r in roles}, "verbose": False,
                     "init_args": args}, nworkers=2)
    assert srv.finished and "tier" not in srv.stats
    host = dict(se.RESULTS)
    assert len(host) > 10

    monkeypatch.delenv("MR_GPU_TIER")
    fresh()
    srv = Server(coord=LocalCoordinator()).configure(
        {"fns": {r: se for r in roles}, "verbose": False,
         "init_args": args})
    assert srv._gpu_engine_kind() == "window"
    srv.loop()
    assert srv.finished
    assert srv.stats["tier"] == "gpu"
    assert srv.stats["engine"] == "window:sessions"
    assert dict(se.RESULTS) == host
    assert list(se.RESULTS) == sorted(se.RESULTS)
    # a user with more clicks than a tile holds
    assert max(sum(c for _, _, c in r) for r in host.values()) > PS
