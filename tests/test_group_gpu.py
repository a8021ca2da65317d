"""The group kernels, the ops, GroupedValuesJob and the Server routing on the
device.  Every comparison is exact against the pure-Python oracle of
group_common: values through their int64 bit patterns and their order keys
(f64 == plus isnan where floats are compared), never a tolerance.  Sizes
come from the extension (ops.group_caps): T rows per LDS-sorted tile."""

import math

import pytest
import torch

import group_common as gc
from mapreduce_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PY_CAPS = (ops.GROUP_TILE, ops.GROUP_QMAX)
PT = ops.GROUP_TILE
PC = (ops.GROUP_TILE, ops.GROUP_RANK_MAX)


@pytest.fixture(scope="module")
def caps():
    return ops.group_caps()


def test_caps_come_from_the_extension(caps):
    assert caps == tuple(ops.ext().group_caps()) == PY_CAPS
    T, Q = caps
    assert T & (T - 1) == 0 and T <= 1 << 15 and Q == 8
    assert ops.group_rank_max() == ops.ext().group_rank_max() == PC[1]


def test_order_keys_on_device():
    for fam in ("random_i64", "f64"):
        v = gc.case_values(fam, 3 * 256 + 5)
        assert gc.to_bits(ops.group_order_keys(v.to(DEV))) == gc.okeys(v)


def same_floats(a, b):
    return all(x == y or (math.isnan(x) and math.isnan(y))
               for x, y in zip(a, b)) and len(a) == len(b)


# parametrised by name over the Python constants; the first assertion checks
# they are the extension's, so the ids name the cases the device runs
@pytest.mark.parametrize("family", gc.FAMILIES)
@pytest.mark.parametrize("name", sorted(gc.cases(PC)))
def test_sort_values_in_groups_matches_oracle(name, family, caps,
                                              monkeypatch):
    assert caps == PY_CAPS
    keys, vals, off = gc.case_data(PC, name, family)
    exp_ok, exp_bits = gc.expected(PC, name, family)
    kbuf, vbuf, kv, vv = gc.baited(keys, vals, DEV)
    k0, v0 = kbuf.clone(), vbuf.view(torch.int64).clone()

    monkeypatch.delenv("MR_GROUP_TWO_SORT", raising=False)
    out = ops.sort_values_in_groups(kv, vv)
    monkeypatch.setenv("MR_GROUP_TWO_SORT", "1")
    two = ops.sort_values_in_groups(kv, vv)
    monkeypatch.delenv("MR_GROUP_TWO_SORT")

    for got in (out, two):
        assert got.dtype == vals.dtype and got.numel() == vals.numel()
        assert gc.okeys(got) == exp_ok
        # equal order keys keep their input order on every path
        assert gc.to_bits(got) == exp_bits
        if off[1:]:
            lo = vbuf.data_ptr()
            hi = lo + vbuf.numel() * 8
            assert not lo <= got.data_ptr() < hi
    if family == "f64":
        srt = []
        for a, b in zip(off, off[1:]):
            # Python's own order on the floats, NaN last
            g = vals[a:b].tolist()
            srt.extend(sorted(x for x in g if not math.isnan(x)))
            srt.extend(x for x in g if math.isnan(x))
        assert same_floats(out.cpu().tolist(), srt)
    assert gc.okeys(out) == gc.okeys(two)
    assert torch.equal(kbuf, k0) and torch.equal(vbuf.view(torch.int64), v0)
    # offsets handed in give the same answer
    _, offsets = ops.group_by_key_sorted(kv)
    assert offsets.cpu().tolist() == off
    again = ops.sort_values_in_groups(kv, vv, offsets)
    assert torch.equal(again.view(torch.int64), out.view(torch.int64))


@pytest.fixture(scope="module")
def ordered():
    """(offsets list, device offsets, ordered device values, order keys,
    device keys, host values) per (case, family), built once."""
    out = {}
    for name, fam in (("short_random", "f64"), ("mix", "random_i64"),
                      ("mix", "two_valued"), ("mix", "f64"),
                      ("n2_one", "f64"), ("n2_two", "random_i64"),
                      ("singles", "f64"), ("threes", "two_valued")):
        keys, vals, off = gc.case_data(PC, name, fam)
        exp_ok, exp_bits = gc.expected(PC, name, fam)
        sv = gc.to_i64(exp_bits).view(vals.dtype).to(DEV)
        out[(name, fam)] = (off, torch.tensor(off, device=DEV), sv, exp_ok,
                            keys.to(DEV), vals)
    return out


@pytest.mark.parametrize("interpolation", ["lower", "higher"])
@pytest.mark.parametrize("case", [("short_random", "f64"),
                                  ("mix", "random_i64"), ("n2_one", "f64"),
                                  ("n2_two", "random_i64"),
                                  ("singles", "f64")])
def test_group_quantiles(case, interpolation, ordered):
    off, offsets, sv, exp_ok, _, _ = ordered[case]
    higher = interpolation == "higher"
    fracs = [(0, 1), (1, 2), (99, 100), (1, 1)]
    got = ops.group_quantiles(offsets, sv, fracs, interpolation)
    assert got.dtype == sv.dtype and tuple(got.shape) == (len(off) - 1, 4)
    assert [gc.okeys(r) for r in got.cpu()] == gc.oracle_quantiles(
        off, exp_ok, [(n, d, higher) for n, d in fracs])
    # Q = GROUP_QMAX, with a denominator at the cap
    fracs = [(i, 7) for i in range(7)] + [(999_999, 10 ** 6)]
    assert len(fracs) == ops.GROUP_QMAX
    got = ops.group_quantiles(offsets, sv, fracs, interpolation)
    assert [gc.okeys(r) for r in got.cpu()] == gc.oracle_quantiles(
        off, exp_ok, [(n, d, higher) for n, d in fracs])


@pytest.mark.parametrize("largest", [True, False])
@pytest.mark.parametrize("case", [("short_random", "f64"),
                                  ("n2_one", "f64"),
                                  ("threes", "two_valued")])
def test_group_topk(case, largest, ordered):
    off, offsets, sv, exp_ok, _, _ = ordered[case]
    longest = max(b - a for a, b in zip(off, off[1:]))
    for k in (1, 3, longest + 2):
        top, cnt = ops.group_topk(offsets, sv, k, largest)
        rows, ecnt = gc.oracle_topk(off, exp_ok, k, largest)
        assert cnt.cpu().tolist() == ecnt
        assert tuple(top.shape) == (len(off) - 1, k)
        for raw, e, c in zip(top.cpu(), rows, ecnt):
            assert gc.okeys(raw)[:c] == e[:c]
            assert gc.to_bits(raw)[c:] == [0] * (k - c)


@pytest.mark.parametrize("case", [("mix", "two_valued"), ("mix", "f64"),
                                  ("threes", "two_valued"),
                                  ("short_random", "f64")])
def test_group_distinct(case, ordered):
    off, _, sv, _, keys, vals = ordered[case]
    got = ops.group_distinct(keys, sv).cpu().tolist()
    assert got == gc.oracle_distinct(off, vals)
    if case[1] == "two_valued":
        assert max(got) == 2
    else:
        # zeros of both signs count once, NaNs of every payload count once
        plain = [len(set(gc.to_bits(vals[a:b]))) for a, b in zip(off,
                                                                 off[1:])]
        assert sum(got) < sum(plain)
    z = torch.tensor([0.0, -0.0, 0.0, float("nan"), -float("nan")],
                     dtype=torch.float64, device=DEV)
    k = torch.zeros(5, dtype=torch.int64, device=DEV)
    assert ops.group_distinct(k, z).cpu().tolist() == [2]


def test_host_checks():
    keys, vals, off = gc.case_data(PC, "short_random", "random_i64")
    k, v = keys.to(DEV), vals.to(DEV)
    offsets = torch.tensor(off, device=DEV)
    e = ops.ext()
    with pytest.raises(RuntimeError, match="int64"):
        ops.sort_values_in_groups(k.to(torch.int32), v)
    with pytest.raises(TypeError, match="int64 or float64"):
        ops.sort_values_in_groups(k, v.to(torch.int32))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.sort_values_in_groups(k, v.cpu())
    with pytest.raises(RuntimeError, match="GPU"):
        ops.sort_values_in_groups(k.cpu(), v)
    with pytest.raises(ValueError, match="one value per key"):
        ops.sort_values_in_groups(k, v[:-1])
    two = torch.stack([v, v], 1)[:, 0]
    with pytest.raises(RuntimeError, match="contiguous"):
        e.group_tile_sort(k, two, False)
    with pytest.raises(RuntimeError, match="one segment id per value"):
        e.group_tile_sort(k[:-1], v, False)
    with pytest.raises(RuntimeError, match="contiguous"):
        e.group_order_keys(two, False)
    with pytest.raises(RuntimeError, match="one value per key"):
        e.group_distinct_flags(k, v[:-1], False)
    with pytest.raises(RuntimeError, match="GPU"):
        e.group_distinct_flags(k.cpu(), v, False)
    with pytest.raises(RuntimeError, match="nseg \\+ 1"):
        e.group_pick(offsets[:0], v, [1], [2], [False])
    with pytest.raises(RuntimeError, match="int64"):
        e.group_pick(offsets.to(torch.int32), v, [1], [2], [False])
    with pytest.raises(RuntimeError, match="GPU"):
        e.group_pick(offsets.cpu(), v, [1], [2], [False])
    with pytest.raises(RuntimeError, match="den must be"):
        e.group_pick(offsets, v, [0], [0], [False])
    with pytest.raises(RuntimeError, match="den must be"):
        e.group_pick(offsets, v, [1], [10 ** 6 + 1], [False])
    with pytest.raises(RuntimeError, match="num must be"):
        e.group_pick(offsets, v, [3], [2], [False])
    with pytest.raises(RuntimeError, match="num must be"):
        e.group_pick(offsets, v, [-1], [2], [False])
    with pytest.raises(RuntimeError, match="Q must be"):
        e.group_pick(offsets, v, [], [], [])
    with pytest.raises(RuntimeError, match="Q must be"):
        e.group_pick(offsets, v, [1] * 9, [2] * 9, [False] * 9)
    with pytest.raises(RuntimeError, match="one entry per specification"):
        e.group_pick(offsets, v, [1, 1], [2], [False, False])
    # the same refusals one layer up, before anything is launched
    with pytest.raises(TypeError, match="float"):
        ops.group_quantiles(offsets, v, [0.5])
    with pytest.raises(ValueError, match="den"):
        ops.group_quantiles(offsets, v, [(1, 0)])
    with pytest.raises(ValueError, match="num"):
        ops.group_quantiles(offsets, v, [(3, 2)])
    with pytest.raises(ValueError, match="Q must be"):
        ops.group_quantiles(offsets, v, [(1, 2)] * 9)
    # offsets that point outside the values read nothing and give 0
    wild = torch.tensor([-5, 3, 10 ** 9], device=DEV)
    assert e.group_pick(wild, v, [1], [2], [False]).cpu().tolist() == [
        [0], [0]]


# ------------------------------------------------------- GroupedValuesJob

@pytest.fixture(scope="module")
def rows():
    """5 000 rows over 700 keys plus one hot key of T + 100 rows, per value
    dtype, on the host; the oracle per (dtype, combine) is shared."""
    return {f64: gc.make_rows(41, 5000, 700, f64, hot=PT + 100)
            for f64 in (False, True)}


@pytest.fixture(scope="module")
def job_expected(rows):
    return {(f64, str(c)): gc.job_oracle(*rows[f64], c)
            for f64 in rows for c in gc.COMBINES}


@pytest.mark.parametrize("small_sort", [None, "1"])
@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("combine", gc.COMBINES, ids=str)
def test_grouped_job_on_device(combine, f64, small_sort, rows, job_expected,
                               monkeypatch):
    from mapreduce_amd.gpu.grouped import GroupedValuesJob

    if small_sort is not None:
        # read per call: the in-tree radix sort carries the payload even
        # at this size
        monkeypatch.setenv("MR_SMALL_SORT_N", small_sort)
    keys, vals = (t.to(DEV) for t in rows[f64])
    keep = keys.clone(), vals.view(torch.int64).clone()
    res = GroupedValuesJob(DEV, combine=combine).run(keys, vals)
    exp = job_expected[(f64, str(combine))]
    assert gc.job_lists(res) == exp and len(exp[0]) > 600
    assert res.values.dtype == vals.dtype
    assert torch.equal(keys, keep[0])
    assert torch.equal(vals.view(torch.int64), keep[1])
    uk, off, ok = exp
    assert gc.okeys(res.median().cpu()) == [
        ok[a + (b - a - 1) // 2] for a, b in zip(off, off[1:])]
    assert res.distinct().cpu().tolist() == [
        len(set(ok[a:b])) for a, b in zip(off, off[1:])]
    if combine is None:
        assert max(res.counts().cpu().tolist()) == PT + 100


@pytest.fixture()
def rccl_ws1(monkeypatch):
    assert torch.cuda.is_available()
    import torch.distributed as td

    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", "29593")  # this file's own
    torch.cuda.set_device(0)
    td.init_process_group("nccl", rank=0, world_size=1,
                          device_id=torch.device("cuda", 0))
    monkeypatch.setenv("MR_FORCE_COLLECTIVE", "1")
    try:
        yield td
    finally:
        td.destroy_process_group()


def test_grouped_job_through_real_rccl(rccl_ws1, rows, job_expected):
    """Every collective call site of the job — the count exchange and the
    two all-to-alls — on RCCL at world 1 (self-exchange), with and without
    a combine ahead of the exchange."""
    from mapreduce_amd.gpu import dist as dx
    from mapreduce_amd.gpu.grouped import GroupedValuesJob

    assert dx.force_collectives()
    keys, vals = (t.to(DEV) for t in rows[True])
    for combine in (None, ("topk", 3), "distinct"):
        res = GroupedValuesJob(DEV, combine=combine).run(keys, vals)
        assert gc.job_lists(res) == job_expected[(True, str(combine))]


# --------------------------------------------------------------- the Server

def test_percentiles_on_hardware(monkeypatch):
    import importlib

    import mapreduce_amd.examples.percentiles as pc
    from mapreduce_amd import job as jobmod
    from mapreduce_amd.parallel.coord import LocalCoordinator
    from mapreduce_amd.server import Server

    monkeypatch.delenv("MR_GPU_TIER", raising=False)
    importlib.reload(pc)
    jobmod._module_cache.clear()
    jobmod._inited.clear()
    args = {"seed": 9, "n": 6000, "nendpoints": 40, "splits": 4, "parts": 4}
    roles = ("taskfn", "mapfn", "partitionfn", "reducefn", "finalfn")
    srv = Server(coord=LocalCoordinator()).configure(
        {"fns": {r: pc for r in roles}, "verbose": False,
         "init_args": args})
    assert srv._gpu_engine_kind() == "group"
    srv.loop()
    assert srv.finished
    assert srv.stats["tier"] == "gpu"
    assert srv.stats["engine"] == "group:quantile"
    groups = {}
    for e, ms in pc.make_rows(9, 6000, 40):
        groups.setdefault(e, []).append(ms)
    exp = {}
    for e, vs in groups.items():
        s = sorted(vs)
        exp[e] = tuple(s[(n * (len(s) - 1)) // d] for n, d in pc.FRACS)
    assert dict(pc.RESULTS) == exp and len(exp) > 10
    assert list(pc.RESULTS) == sorted(pc.RESULTS)
    assert max(len(v) for v in groups.values()) > PT  # a straddling key
