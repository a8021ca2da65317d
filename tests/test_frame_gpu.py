"""The frame kernels, OrderedRows.rolling and the Server routing of
examples/rolling_spend on the device.  Every comparison is exact on bit
patterns against the oracle of frame_common, but for the one general-f64
sum, whose bound is that derived in
test_window_gpu.test_general_f64_sum_within_the_derived_bound.  Sizes come
from the extension (ops.frame_caps): T rows per tile of the window bounds
kernel, W rows of a window staged in LDS, R rows per tile of the reduce
kernels."""

import math

import pytest
import torch

import frame_common as fc
import group_common as gc
import window_common as wc
from mapreduce_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PT, PW, PR = ops.FRAME_TILE, ops.FRAME_WIN, ops.FRAME_RTILE
BIG = 2 ** 63 - 1
OPN = {"sum": 0, "min": 1, "max": 2}


@pytest.fixture(scope="module")
def caps():
    return ops.frame_caps()


def test_caps_come_from_the_extension(caps):
    assert caps == tuple(ops.ext().frame_caps()) == (PT, PW, PR)
    T, W, R = caps
    assert T % 256 == 0 and W > T and R == 256 * 8


def bait(t, below, above):
    """-> (buffer, view): t as the exact-size inner slice of a tensor two
    entries longer, 8 bytes off the buffer's 16-byte alignment."""
    buf = torch.empty(t.numel() + 2, dtype=torch.int64)
    buf[1:-1] = t.view(torch.int64)
    buf[0], buf[-1] = below, above
    buf = buf.to(DEV).view(t.dtype)
    return buf, buf[1:-1]


def outside(out, *bufs):
    return all(not b.data_ptr() <= out.data_ptr() < b.data_ptr()
               + b.numel() * 8 for b in bufs)


# ------------------------------------------------------------------ bounds

# parametrised by name over the Python constants; the first assertion checks
# they are the extension's, so the ids name the cases the device runs
@pytest.mark.parametrize("name", sorted(fc.bounds_cases(PT, PW, PR)))
def test_frame_bounds_matches_oracle(name, caps, monkeypatch):
    assert caps == (PT, PW, PR)
    k, t, params = fc.bounds_cases(PT, PW, PR)[name]
    # the flanks continue the first and the last key with the extreme
    # times: a probe outside [0, n) changes a frame
    kbuf, tbuf, kv, tv = gc.baited(
        gc.to_i64(k), torch.tensor(t, dtype=torch.int64), DEV)
    k0, t0 = kbuf.clone(), tbuf.clone()
    if k:
        assert kv.data_ptr() % 16 == 8 and tv.data_ptr() % 16 == 8
    for p, f in params:
        want = fc.expected_bounds(PT, PW, PR, name, p, f)
        for row in ("0", "1"):   # the window kernel, the row kernel
            monkeypatch.setenv("MR_FRAME_ROW", row)
            lo, hi = ops.frame_bounds(kv, tv, p, f)
            assert lo.dtype == hi.dtype == torch.int64
            assert lo.is_cuda and hi.is_cuda
            assert (lo.cpu().tolist(), hi.cpu().tolist()) == want, (p, f, row)
            if k:
                assert outside(lo, kbuf, tbuf) and outside(hi, kbuf, tbuf)
                assert lo.data_ptr() != hi.data_ptr()
    assert torch.equal(kbuf, k0) and torch.equal(tbuf, t0)


def test_the_default_bounds_kernel_matches_both(caps, monkeypatch):
    k, t, _ = fc.bounds_cases(PT, PW, PR)["ties"]
    kv, tv = gc.to_i64(k).to(DEV), torch.tensor(t, device=DEV)
    monkeypatch.delenv("MR_FRAME_ROW", raising=False)
    lo, hi = ops.frame_bounds(kv, tv, 1, 2)
    assert (lo.cpu().tolist(), hi.cpu().tolist()) == fc.oracle_range_frames(
        k, t, 1, 2)


# ------------------------------------------------------------------ reduce

def run_reduce(vals, lo, hi, fam_ops, want):
    """frame_reduce of baited copies under every op; inputs unchanged."""
    f64 = vals.dtype == torch.float64
    n = vals.numel()
    if f64:
        below = gc.to_i64([gc.f64_bits(float("-inf"))])[0]
        above = gc.to_i64([gc.f64_bits(float("inf"))])[0]
    else:
        below, above = gc.I64_MIN, gc.I64_MAX
    vbuf, vv = bait(vals, below, above)
    lbuf, lv = bait(torch.tensor(lo, dtype=torch.int64), 0, 0)
    hbuf, hv = bait(torch.tensor(hi, dtype=torch.int64), n, n)
    keep = [b.view(torch.int64).clone() for b in (vbuf, lbuf, hbuf)]
    assert vv.data_ptr() % 16 == 8
    for op in fam_ops:
        out = ops.frame_reduce(vv, lv, hv, op)
        assert out.dtype == vals.dtype and out.numel() == n and out.is_cuda
        assert gc.to_bits(out) == want(op), op
        assert outside(out, vbuf, lbuf, hbuf)
    for b, k in zip((vbuf, lbuf, hbuf), keep):
        assert torch.equal(b.view(torch.int64), k)


@pytest.mark.parametrize("name", sorted(fc.reduce_cases(PR)))
def test_frame_reduce_matches_oracle(name, caps):
    """sum / min / max on i64 (full range: the sums wrap) and f64 (small
    integers: the sums are exact; specials: -0.0 / +0.0, infinities and
    NaNs of four payloads, where the earliest row of the frame must win)."""
    assert caps == (PT, PW, PR)
    lo, hi = fc.reduce_cases(PR)[name]
    for family, fam_ops in fc.FAMILIES.items():
        run_reduce(fc.reduce_data(PR, name, family), lo, hi, fam_ops,
                   lambda op: fc.expected_reduce(PR, name, family, op))


def test_duplicated_extremes_keep_the_earliest_row_of_the_frame(caps):
    """No negative value, so a zero is the minimum and a NaN the maximum of
    most frames: zeros of both signs and NaNs of four payloads alternate,
    and the bits that come back say which row won."""
    _, _, R = caps
    n = 2 * R + 100
    pos = gc.f64_bits(2.5)
    bits = [0 if i % 3 == 0 else fc.SIGN if i % 3 == 1
            else gc.NAN_BITS[i // 5 % 4] if i % 5 == 0 else pos + i
            for i in range(n)]
    vals = gc.to_i64(bits).view(torch.float64)
    lo = [max(0, i - (i % 50) * 60) for i in range(n)]
    hi = [min(n, i + 1 + i % 3) for i in range(n)]
    assert any(a // R + 1 < (b - 1) // R for a, b in zip(lo, hi))
    want = {op: fc.oracle_reduce(vals, lo, hi, op) for op in ("min", "max")}
    assert len(set(want["min"])) >= 2 and len(set(want["max"])) >= 4
    run_reduce(vals, lo, hi, ("min", "max"), want.__getitem__)


def test_an_inf_reaches_only_the_frames_that_hold_it(caps):
    """One +inf in the middle of a long key.  A frame without it comes back
    finite and exact; a difference of two running sums would give NaN for
    every frame behind it."""
    _, _, R = caps
    n = 3 * R + 40
    vals = fc.values("f64_int", n)
    mid = R + R // 2
    vals[mid] = float("inf")
    for back in (100, R + 10):
        lo = [max(0, i - back) for i in range(n)]
        hi = [i + 1 for i in range(n)]
        got = ops.frame_reduce(vals.to(DEV), torch.tensor(lo, device=DEV),
                               torch.tensor(hi, device=DEV), "sum").cpu()
        holds = torch.tensor([a <= mid < b for a, b in zip(lo, hi)])
        assert holds.sum() == back + 1
        assert (got[holds] == float("inf")).all()
        assert torch.isfinite(got[~holds]).all()
        assert gc.to_bits(got) == fc.oracle_reduce(vals, lo, hi, "sum")


def test_general_f64_frame_sum_within_the_derived_bound(caps):
    """Any summation order of m terms is within (m - 1) u sum|v| + O(u^2)
    of the exact sum, u = 2^-53; the bound asserted is twice that first
    order, m 2^-52 sum|v| over the frame's own m rows, against math.fsum of
    the frame."""
    _, _, R = caps
    n = 3 * R + 50
    vals = fc.values("f64_general", n)
    lo = [max(0, i - (i % 13) * 300) for i in range(n)]
    hi = [min(n, i + 1 + i % 4) for i in range(n)]
    assert any(a // R + 1 < (b - 1) // R for a, b in zip(lo, hi))
    got = ops.frame_reduce(vals.to(DEV), torch.tensor(lo, device=DEV),
                           torch.tensor(hi, device=DEV), "sum").cpu().tolist()
    v = vals.tolist()
    worst = 0.0
    for i, (a, b) in enumerate(zip(lo, hi)):
        w = v[a:b]
        bound = (b - a) * 2.0 ** -52 * math.fsum(abs(x) for x in w)
        err = abs(got[i] - math.fsum(w))
        worst = max(worst, err / bound if bound else err)
        assert err <= bound, (i, a, b, err, bound)
    print(f"general f64 frame sum: worst error / bound = {worst:.3g}")


def test_stages_tile_count_and_tree(caps):
    """The exposed passes: one aggregate per tile, a tree of
    floor(log2(ntiles)) + 1 levels that holds only whole nodes, prefix and
    suffix aggregates inside every tile."""
    _, _, R = caps
    e = ops.ext()
    for n, levels in ((R, [1]), (R + 1, [2, 1]), (9 * R + 5, [10, 5, 2, 1])):
        assert ops.frame_tree_levels(-(-n // R)) == levels
        vals = fc.values("i64_full", n)
        dv = vals.to(DEV)
        tile_lo = [i // R * R for i in range(n)]
        tile_hi = [min(n, i // R * R + R) for i in range(n)]
        rows = list(range(n))
        for op in ("sum", "max"):
            pre, suf, tiles = e.frame_tile(dv, OPN[op], False)
            assert pre.numel() == suf.numel() == n
            assert tiles.numel() == levels[0]
            assert gc.to_bits(pre) == fc.oracle_reduce(
                vals, tile_lo, [i + 1 for i in rows], op)
            assert gc.to_bits(suf) == fc.oracle_reduce(vals, rows, tile_hi,
                                                       op)
            tree = e.frame_tree(tiles, OPN[op], False)
            assert tree.numel() == sum(levels)
            a, b = [], []
            for lv, cnt in enumerate(levels):
                a += [t * R << lv for t in range(cnt)]
                b += [min(n, (t + 1) * R << lv) for t in range(cnt)]
            assert gc.to_bits(tree) == fc.oracle_reduce(vals, a, b, op)
            lo = torch.tensor([max(0, i - 3 * R) for i in rows], device=DEV)
            hi = torch.tensor([i + 1 for i in rows], device=DEV)
            out = e.frame_apply(dv, lo, hi, pre, suf, tree, OPN[op], False)
            assert torch.equal(out, ops.frame_reduce(dv, lo, hi, op))


def test_frame_host_checks():
    k = torch.arange(40, dtype=torch.int64, device=DEV) // 3
    t = torch.arange(40, dtype=torch.int64, device=DEV)
    lo, hi = t.clone(), t + 1
    e = ops.ext()
    strided = torch.stack([t, t], 1)[:, 0]
    for kk, tt in ((k, t), (k[:0], t[:0])):   # n == 0 runs the same checks
        with pytest.raises(RuntimeError, match="GPU"):
            ops.frame_bounds(kk, tt.cpu(), 1)
        with pytest.raises(RuntimeError, match="GPU"):
            ops.frame_bounds(kk.cpu(), tt, 1)
        with pytest.raises(RuntimeError, match="keys must be int64"):
            e.frame_bounds(kk.to(torch.int32), tt, 1, 0, False)
        with pytest.raises(RuntimeError, match="times must be int64"):
            e.frame_bounds(kk, tt.to(torch.float64), 1, 0, True)
        with pytest.raises(RuntimeError, match="preceding"):
            e.frame_bounds(kk, tt, -1, 0, False)
        with pytest.raises(RuntimeError, match="following"):
            e.frame_bounds(kk, tt, 0, -1, True)
        with pytest.raises(RuntimeError, match="GPU"):
            ops.frame_reduce(tt, tt.cpu(), tt + 1)
        with pytest.raises(RuntimeError, match="GPU"):
            ops.frame_reduce(tt.cpu(), tt, tt + 1)
        with pytest.raises(RuntimeError, match="op must be"):
            e.frame_reduce(tt, tt, tt + 1, 3, False)
        with pytest.raises(RuntimeError, match="lo must be int64"):
            e.frame_reduce(tt, tt.to(torch.int32), tt + 1, 0, False)
        with pytest.raises(RuntimeError, match="hi must be int64"):
            e.frame_reduce(tt, tt, tt.to(torch.float64), 0, False)
    with pytest.raises(RuntimeError, match="one time per key"):
        e.frame_bounds(k, t[:-1], 1, 0, False)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.frame_bounds(k, strided, 1)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.frame_bounds(strided, t, 1)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.frame_reduce(strided, lo, hi)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.frame_reduce(t, strided, hi)
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.frame_reduce(t, lo, strided)
    with pytest.raises(RuntimeError, match="lo must hold 40 entries"):
        e.frame_reduce(t, lo[:-1], hi, 0, False)
    with pytest.raises(RuntimeError, match="hi must hold 40 entries"):
        e.frame_reduce(t, lo, hi[:-1], 0, False)
    pre, suf, tiles = e.frame_tile(t, 0, False)
    tree = e.frame_tree(tiles, 0, False)
    with pytest.raises(RuntimeError, match="tree must hold 1 entries"):
        e.frame_apply(t, lo, hi, pre, suf, torch.cat([tree, tree]), 0, False)
    with pytest.raises(RuntimeError, match="pre must hold 40 entries"):
        e.frame_apply(t, lo, hi, pre[:-1], suf, tree, 0, False)
    with pytest.raises(RuntimeError, match="op must be"):
        e.frame_tile(t, -1, False)
    with pytest.raises(RuntimeError, match="op must be"):
        e.frame_tree(tiles, 3, False)
    # the Python layer's own refusals hold on the device too
    with pytest.raises(TypeError, match="int64 times"):
        ops.frame_bounds(k, t.to(torch.float64), 1)
    with pytest.raises(ValueError, match="preceding"):
        ops.frame_bounds(k, t, 2 ** 63)
    with pytest.raises(ValueError, match="op must be"):
        ops.frame_reduce(t, lo, hi, "mean")
    # n == 0: empty columns of the right dtype on the device
    l0, h0 = ops.frame_bounds(k[:0], t[:0], 5, 5)
    assert l0.numel() == h0.numel() == 0 and l0.is_cuda and h0.is_cuda
    out = ops.frame_reduce(t[:0].view(torch.float64), l0, h0, "min")
    assert out.numel() == 0 and out.dtype == torch.float64 and out.is_cuda
    lo_r, hi_r = ops.frame_bounds_rows(torch.tensor([0, 3, 3, 40],
                                                    device=DEV), 2, 1)
    assert lo_r.is_cuda and (lo_r.cpu().tolist(), hi_r.cpu().tolist()) == \
        fc.oracle_row_frames([0, 3, 3, 40], 2, 1)


# ------------------------------------------------------- OrderedRows.rolling

@pytest.fixture(scope="module")
def rows():
    """5 000 rows over 700 keys plus one hot key of R + 100 rows, with ties
    in the order column: i64 order and values, and f64 order and values."""
    return {f64: wc.make_rows(43, 5000, 700, f64, f64, hot=PR + 100)
            for f64 in (False, True)}


@pytest.mark.parametrize("f64", [False, True])
def test_rolling_on_device(f64, rows):
    from mapreduce_amd.gpu.window import WindowJob

    res = WindowJob(DEV).run(*(t.to(DEV) for t in rows[f64]))
    assert res.counts().max().item() > PR   # a key longer than a tile
    assert res.values.is_cuda
    fc.check_rolling(res, f64, not f64)
    if f64:
        with pytest.raises(TypeError, match="int64 times"):
            res.rolling("min", 5)


@pytest.fixture()
def rccl_ws1(monkeypatch):
    assert torch.cuda.is_available()
    import torch.distributed as td

    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", "29603")  # this file's own
    torch.cuda.set_device(0)
    td.init_process_group("nccl", rank=0, world_size=1,
                          device_id=torch.device("cuda", 0))
    monkeypatch.setenv("MR_FORCE_COLLECTIVE", "1")
    try:
        yield td
    finally:
        td.destroy_process_group()


def test_rolling_through_real_rccl(rccl_ws1, rows):
    """The job's exchange on RCCL at world 1 (self-exchange), rolling on the
    partition it leaves."""
    from mapreduce_amd.gpu import dist as dx
    from mapreduce_amd.gpu.window import WindowJob

    assert dx.force_collectives()
    res = WindowJob(DEV).run(*(t.to(DEV) for t in rows[False]))
    fc.check_rolling(res, False, True)


# --------------------------------------------------------------- the Server

def test_rolling_spend_on_hardware(monkeypatch):
    import importlib

    import mapreduce_amd.examples.rolling_spend as rs
    from mapreduce_amd import job as jobmod
    from mapreduce_amd import run_local
    from mapreduce_amd.parallel.coord import LocalCoordinator
    from mapreduce_amd.server import Server

    def fresh():
        importlib.reload(rs)
        jobmod._module_cache.clear()
        jobmod._inited.clear()

    args = {"seed": 9, "n": 6000, "nusers": 40, "splits": 4, "parts": 4}
    roles = ("taskfn", "mapfn", "partitionfn", "reducefn", "finalfn")
    monkeypatch.setenv("MR_GPU_TIER", "off")
    fresh()
    srv = run_local({"fns": {r: rs for r in roles}, "verbose": False,
                     "init_args": args}, nworkers=2)
    assert srv.finished and "tier" not in srv.stats
    host = dict(rs.RESULTS)
    assert len(host) > 10

    monkeypatch.delenv("MR_GPU_TIER")
    fresh()
    srv = Server(coord=LocalCoordinator()).configure(
        {"fns": {r: rs for r in roles}, "verbose": False,
         "init_args": args})
    assert srv._gpu_engine_kind() == "window"
    srv.loop()
    assert srv.finished
    assert srv.stats["tier"] == "gpu"
    assert srv.stats["engine"] == "window:rolling"
    assert dict(rs.RESULTS) == host
    assert list(rs.RESULTS) == sorted(rs.RESULTS)
    # a user with more purchases than a tile holds
    assert max(len(r) for r in host.values()) > PR
