"""The rolling-aggregate family without a GPU: the case generators, the CPU
tier of ops.frame_bounds / frame_bounds_rows / frame_reduce against the
oracle of frame_common, parameter validation, OrderedRows.rolling, the
reducer names, the Server routing and examples/rolling_spend on both tiers.
Every comparison is exact but where a bound is stated."""

import numpy as np
import pytest
import torch

import frame_common as fc
import group_common as gc
import window_common as wc
from mapreduce_amd import ops
from mapreduce_amd.gpu.window import WindowJob

T, W, R = ops.frame_caps()
BCASES = fc.bounds_cases(T, W, R)
RCASES = fc.reduce_cases(R)
ROLES = ("taskfn", "mapfn", "partitionfn", "reducefn", "finalfn")
BIG = 2 ** 63 - 1


# ------------------------------------------------------------ the generators

def test_cases_have_the_properties_the_gpu_tests_rely_on():
    assert (T, W, R) == (ops.FRAME_TILE, ops.FRAME_WIN, ops.FRAME_RTILE)
    assert W > T > 64 and R == 256 * 8
    # bounds: rows sorted (the oracle asserts it), frames hold their row
    for name, (k, t, params) in BCASES.items():
        assert len(k) == len(t)
        for p, f in params:
            lo, hi = fc.expected_bounds(T, W, R, name, p, f)
            assert all(a <= i < b for i, (a, b) in enumerate(zip(lo, hi)))
            assert lo == sorted(lo) and hi == sorted(hi), name
    k, t, _ = BCASES["one_key_ticks"]
    assert len(k) == 3 * R + 17 and set(k) == {7}
    assert all(b - a == 1 for a, b in zip(t, t[1:]))
    # the run of peers is longer than W and lies across the tile edge at T
    k, t, _ = BCASES["peers_over_W"]
    lo, hi = fc.expected_bounds(T, W, R, "peers_over_W", 0, 0)
    assert lo[T - 100] == T - 100 < T < hi[T - 100] == T - 100 + W + 50
    assert hi[T - 1] - lo[0] > W
    # the window of tile 2 is exactly W rows, then W + 1
    for (p, f), size in zip(BCASES["window_W"][2], (W, W + 1) * 3):
        lo, hi = fc.expected_bounds(T, W, R, "window_W", p, f)
        assert hi[3 * T - 1] - lo[2 * T] == size
    # preceding = following = 0: the frames are the peer groups
    k, t, _ = BCASES["ties"]
    lo, hi = fc.expected_bounds(T, W, R, "ties", 0, 0)
    assert max(b - a for a, b in zip(lo, hi)) > 2
    for i, (a, b) in enumerate(zip(lo, hi)):
        assert {(k[j], t[j]) for j in range(a, b)} == {(k[i], t[i])}
        assert a == 0 or (k[a - 1], t[a - 1]) != (k[i], t[i])
        assert b == len(k) or (k[b], t[b]) != (k[i], t[i])
    # row 0's lower end saturates at 0, row 3's upper end at 2^64 - 1
    assert fc.expected_bounds(T, W, R, "saturate", BIG, BIG) == (
        [0, 0, 1, 2], [2, 3, 4, 4])
    assert fc.expected_bounds(T, W, R, "saturate", 1, 1) == (
        [0, 1, 1, 3], [1, 3, 3, 4])
    k, t, _ = BCASES["key_change_at_tile_edge"]
    heads = [i for i in range(1, len(k)) if k[i] != k[i - 1]]
    assert heads == [T - 1, T, T + 1] and len(set(t)) == 1
    assert fc.expected_bounds(T, W, R, "key_change_at_tile_edge", BIG,
                              BIG)[0][T - 1:T + 2] == [T - 1, T, T + 1]
    assert any(x & fc.SIGN for x in BCASES["singles"][0])
    assert any(not x & fc.SIGN for x in BCASES["singles"][0])

    # reduce: which paths the frames take
    def inside(name):
        lo, hi = RCASES[name]
        return [a // R == (b - 1) // R for a, b in zip(lo, hi)]

    lo, hi = RCASES["in_chunk"]
    assert all(a // 64 == (b - 1) // 64 for a, b in zip(lo, hi))
    assert len(lo) > R
    lo, hi = RCASES["cross_chunk"]
    assert any(a // 64 != (b - 1) // 64 for a, b in zip(lo, hi))
    assert not all(inside("one_tile_edge"))
    assert {c for _, c in fc.whole_tiles(*RCASES["one_tile_edge"], R)} == {0}
    assert {c for _, c in fc.whole_tiles(*RCASES["one_whole_tile"], R)} == {
        0, 1}
    lo, hi = RCASES["nine_tiles"]
    n = len(lo)
    assert n == 9 * R + 5 and -(-n // R) == 10
    spans = set(fc.whole_tiles(lo, hi, R))
    assert {c for _, c in spans} == set(range(9))
    for c in range(1, 8):   # odd and even first tiles; 8 tiles start at 1
        assert {s % 2 for s, cc in spans if cc == c} == {0, 1}, c
    assert any(inside("nine_tiles"))


def test_oracle_on_hand_cases():
    k, t = [1, 1, 1, 1, 2], [0, 5, 5, 11, 5]
    assert fc.oracle_range_frames(k, t, 5, 0) == ([0, 0, 0, 3, 4],
                                                  [1, 3, 3, 4, 5])
    assert fc.oracle_range_frames(k, t, 0, 6) == ([0, 1, 1, 3, 4],
                                                  [3, 4, 4, 4, 5])
    assert fc.oracle_row_frames([0, 3, 3, 5], 1, 0) == ([0, 0, 1, 3, 3],
                                                        [1, 2, 3, 4, 5])
    big = gc.I64_MAX
    v = torch.tensor([3, -1, -1, 9, big])
    lo, hi = [0, 0, 1, 2, 3], [2, 3, 4, 5, 5]
    assert fc.oracle_reduce(v, lo, hi, "sum") == [
        2, 1, 7, (8 + big) & fc.M64, (9 + big) & fc.M64]   # the last two wrap
    assert fc.oracle_reduce(v, lo, hi, "min") == [
        fc.M64, fc.M64, fc.M64, fc.M64, 9]
    z = gc.to_i64([0, fc.SIGN, fc.SIGN, 0]).view(torch.float64)
    # -0.0 equals +0.0: the earliest row of the frame wins
    assert fc.oracle_reduce(z, [0, 1, 1, 2], [2, 2, 4, 4], "max") == [
        0, fc.SIGN, fc.SIGN, fc.SIGN]


# ------------------------------------------------------------------ the ops

@pytest.mark.parametrize("name", sorted(BCASES))
def test_frame_bounds_cpu(name):
    k, t, params = BCASES[name]
    kt, tt = gc.to_i64(k), torch.tensor(t, dtype=torch.int64)
    k0, t0 = kt.clone(), tt.clone()
    for p, f in params:
        lo, hi = ops.frame_bounds(kt, tt, p, f)
        assert lo.dtype == hi.dtype == torch.int64
        assert (lo.tolist(), hi.tolist()) == fc.expected_bounds(
            T, W, R, name, p, f), (p, f)
    assert torch.equal(kt, k0) and torch.equal(tt, t0)


def test_frame_bounds_rows_cpu():
    for lens in ((), (1,), (3, 1, 5), (2,) * 40 + (90,)):
        off = gc.offsets_of(lens)
        for p, f in ((0, 0), (1, 0), (0, 2), (3, 3), (2 ** 31 - 1, 2 ** 31 - 1)):
            lo, hi = ops.frame_bounds_rows(torch.tensor(off), p, f)
            assert (lo.tolist(), hi.tolist()) == fc.oracle_row_frames(
                off, p, f)
            lo2, hi2 = ops.frame_bounds_rows(torch.tensor(off), p, f,
                                             nrows=off[-1])
            assert torch.equal(lo, lo2) and torch.equal(hi, hi2)


@pytest.mark.parametrize("name", sorted(RCASES))
def test_frame_reduce_cpu(name):
    lo, hi = (torch.tensor(x, dtype=torch.int64) for x in RCASES[name])
    for family, fam_ops in fc.FAMILIES.items():
        vals = fc.reduce_data(R, name, family)
        v0 = vals.clone()
        for op in fam_ops:
            out = ops.frame_reduce(vals, lo, hi, op)
            assert out.dtype == vals.dtype and out.numel() == vals.numel()
            assert gc.to_bits(out) == fc.expected_reduce(R, name, family,
                                                         op), (family, op)
        assert gc.to_bits(vals) == gc.to_bits(v0)


def test_frame_reduce_cpu_clamps_frames_outside_the_contract():
    v = torch.tensor([5, 1, 7, 3], dtype=torch.int64)
    lo = torch.tensor([-3, 2, 9, 0])    # below 0, behind the row, beyond n
    hi = torch.tensor([0, 1, 99, -5])   # before the row, beyond n
    # clamped: [0, 1) [1, 2) [2, 4) [0, 4)
    assert ops.frame_reduce(v, lo, hi, "sum").tolist() == [5, 1, 10, 16]
    assert ops.frame_reduce(v, lo, hi, "min").tolist() == [5, 1, 3, 1]
    f = v.to(torch.float64)
    assert ops.frame_reduce(f, lo, hi, "max").tolist() == [5., 1., 7., 7.]
    assert ops.frame_reduce(f, lo, hi, "sum").tolist() == [5., 1., 10., 16.]


def test_an_inf_reaches_only_the_frames_that_hold_it_cpu():
    v = torch.arange(50, dtype=torch.float64)
    v[20] = float("inf")
    lo = torch.clamp(torch.arange(50) - 3, min=0)
    hi = torch.arange(50) + 1
    out = ops.frame_reduce(v, lo, hi, "sum")
    assert torch.isinf(out[20:24]).all()
    assert torch.isfinite(out[:20]).all() and torch.isfinite(out[24:]).all()
    assert out[24].item() == 21 + 22 + 23 + 24


def test_parameter_validation():
    k = torch.zeros(3, dtype=torch.int64)
    off = torch.tensor([0, 3])
    for bad in (True, 1.0, "1", None):
        with pytest.raises(TypeError, match="preceding"):
            ops.frame_bounds(k, k, bad)
        with pytest.raises(TypeError, match="following"):
            ops.frame_bounds(k, k, 1, bad)
        with pytest.raises(TypeError, match="preceding"):
            ops.frame_bounds_rows(off, bad)
        with pytest.raises(TypeError, match="following"):
            ops.frame_bounds_rows(off, 0, bad)
    for bad in (-1, 2 ** 63):
        with pytest.raises(ValueError, match="preceding"):
            ops.frame_bounds(k, k, bad)
        with pytest.raises(ValueError, match="following"):
            ops.frame_bounds(k, k, 0, bad)
    for bad in (-1, 2 ** 31):
        with pytest.raises(ValueError, match="preceding"):
            ops.frame_bounds_rows(off, bad)
        with pytest.raises(ValueError, match="following"):
            ops.frame_bounds_rows(off, 0, bad)
    assert ops.frame_bounds(k, k, BIG, BIG)[1].tolist() == [3, 3, 3]
    with pytest.raises(TypeError, match="int64 times"):
        ops.frame_bounds(k, k.to(torch.float64), 1)
    with pytest.raises(TypeError, match="keys must be int64"):
        ops.frame_bounds(k.to(torch.int32), k, 1)
    with pytest.raises(ValueError, match="one time per key"):
        ops.frame_bounds(k, k[:-1], 1)
    with pytest.raises(ValueError, match="op must be"):
        ops.frame_reduce(k, k, k + 1, "count")
    with pytest.raises(TypeError, match="int64 or float64"):
        ops.frame_reduce(k.to(torch.int32), k, k + 1)
    with pytest.raises(TypeError, match="lo and hi must be int64"):
        ops.frame_reduce(k, k.to(torch.int32), k + 1)
    with pytest.raises(ValueError, match="one lo and one hi"):
        ops.frame_reduce(k, k[:-1], k + 1)
    out = ops.frame_reduce(k[:0].to(torch.float64), k[:0], k[:0], "max")
    assert out.numel() == 0 and out.dtype == torch.float64
    assert ops.frame_tree_levels(1) == [1]
    assert ops.frame_tree_levels(2) == [2, 1]
    assert ops.frame_tree_levels(10) == [10, 5, 2, 1]


# ------------------------------------------------------- OrderedRows.rolling

@pytest.mark.parametrize("f64", [False, True])
def test_rolling_single_rank(f64):
    keys, order, vals = wc.make_rows(31, 900, 60, f64, f64, hot=300)
    res = WindowJob("cpu").run(keys, order, vals)
    fc.check_rolling(res, f64, not f64)


def test_rolling_refusals():
    keys, order, vals = wc.make_rows(31, 50, 5, True, False)
    res = WindowJob("cpu").run(keys, order, vals)
    with pytest.raises(TypeError, match="int64 times"):
        res.rolling("sum", 5)
    with pytest.raises(TypeError, match="int64 times"):
        res.frames(5)
    with pytest.raises(ValueError, match="unit must be"):
        res.frames(5, unit="groups")
    with pytest.raises(ValueError, match="op must be one of"):
        res.rolling("median", 5, unit="rows")
    bare = WindowJob("cpu").run(keys, order.to(torch.int64))
    assert bare.rolling("count", 2, 2).tolist() == (
        bare.frames(2, 2)[1] - bare.frames(2, 2)[0]).tolist()
    for op in ("sum", "min", "max", "mean"):
        with pytest.raises(ValueError, match="value column"):
            bare.rolling(op, 2)
    empty = WindowJob("cpu").run(keys[:0], order[:0].to(torch.int64),
                                 vals[:0])
    assert empty.rolling("sum", 2).numel() == 0
    assert empty.rolling("count", 2, unit="rows").numel() == 0


# ------------------------------------------------------------ reducer names

@pytest.mark.parametrize("name,exp", [
    ("rolling:sum:3600", ("sum", 3600, 0, "range")),
    ("rolling:max:99,rows", ("max", 99, 0, "rows")),
    ("rolling:count:5,fol=5", ("count", 5, 5, "range")),
    ("rolling:mean:0,rows,fol=7", ("mean", 0, 7, "rows")),
    ("rolling:min:9223372036854775807,fol=9223372036854775807",
     ("min", BIG, BIG, "range")),
    ("rolling:min:2147483647,rows", ("min", 2 ** 31 - 1, 0, "rows")),
])
def test_rolling_reducer_names(name, exp):
    from mapreduce_amd.server import Server

    op, arg = Server.parse_window_reducer(name)
    assert op == "rolling"
    assert (arg["op"], arg["preceding"], arg["following"],
            arg["unit"]) == exp
    assert Server.parse_group_reducer(name) is None
    assert Server.parse_asof_reducer(name) is None


@pytest.mark.parametrize("name", [
    "rolling", "rolling:", "rolling:sum", "rolling:sum:", "rolling:sum:x",
    "rolling:sum:-1", "rolling:sum:1.5", "rolling:median:5",
    "rolling:sum:9223372036854775808", "rolling:sum:5,fol=9223372036854775808",
    "rolling:sum:2147483648,rows", "rolling:sum:5,rows,fol=2147483648",
    "rolling:sum:5,rows,rows", "rolling:sum:5,fol=1,fol=2",
    "rolling:sum:5,fol=", "rolling:sum:5,", "rolling:sum:5,range",
    "rolling:sum:5:6", "rolling:SUM:5", "rolling:sum: 5"])
def test_malformed_rolling_reducers_are_refused(name, monkeypatch):
    from mapreduce_amd.parallel.coord import LocalCoordinator
    from mapreduce_amd.server import Server

    monkeypatch.setenv("MR_GPU_TIER", "force")
    with pytest.raises(ValueError) as e:
        Server(coord=LocalCoordinator()).configure(
            {"fns": _toy_fns([], reducefn_gpu=name), "verbose": False})
    assert repr(name) in str(e.value)
    for other in ("sum", "cumsum", "sessions:5", "join_asof", "roll:sum:5"):
        got = Server.parse_window_reducer(other)
        assert got is None or got[0] != "rolling"


# (key, order, value)
ROWS = [(2, 30, 5), (1, 10, 7), (2, 10, -3), (1, 10, 7), (2, 30, 4),
        (3, 0, 0), (2, 20, 9)]


def _toy_fns(seen, cols=3, **over):
    fns = {
        "taskfn": lambda emit: emit(1, "x"),
        "mapfn": lambda k, v, emit: None,
        "mapfn_gpu_pairs": lambda k, v: tuple([r[c] for r in ROWS]
                                              for c in range(cols)),
        "partitionfn": lambda k: 0,
        "reducefn": lambda k, vs, emit: emit(sum(vs)),
        "finalfn": lambda pairs: seen.extend(pairs) or True,
    }
    fns.update(over)
    return {r: fns for r in ROLES + ("combinerfn",)}


@pytest.mark.parametrize("name,cols,exp", [
    ("rolling:sum:10", 3, [(1, [(10, 14), (10, 14)]),
                           (2, [(10, -3), (20, 6), (30, 18), (30, 18)]),
                           (3, [(0, 0)])]),
    ("rolling:sum:1,rows", 3, [(1, [(10, 7), (10, 14)]),
                               (2, [(10, -3), (20, 6), (30, 13), (30, 9)]),
                               (3, [(0, 0)])]),
    ("rolling:min:0,fol=10", 3, [(1, [(10, 7), (10, 7)]),
                                 (2, [(10, -3), (20, 4), (30, 4), (30, 4)]),
                                 (3, [(0, 0)])]),
    ("rolling:max:9", 3, [(1, [(10, 7), (10, 7)]),
                          (2, [(10, -3), (20, 9), (30, 5), (30, 5)]),
                          (3, [(0, 0)])]),
    ("rolling:mean:10", 3, [(1, [(10, 7.0), (10, 7.0)]),
                            (2, [(10, -3.0), (20, 3.0), (30, 6.0), (30, 6.0)]),
                            (3, [(0, 0.0)])]),
    ("rolling:count:10,fol=10", 2, [(1, [(10, 2), (10, 2)]),
                                    (2, [(10, 2), (20, 4), (30, 3), (30, 3)]),
                                    (3, [(0, 1)])]),
    ("rolling:count:1,rows", 2, [(1, [(10, 1), (10, 2)]),
                                 (2, [(10, 1), (20, 2), (30, 2), (30, 2)]),
                                 (3, [(0, 1)])]),
])
def test_rolling_reducers_hand_finalfn_the_documented_pairs(name, cols, exp,
                                                            monkeypatch):
    from mapreduce_amd.parallel.coord import LocalCoordinator
    from mapreduce_amd.server import Server

    monkeypatch.setenv("MR_GPU_TIER", "force")
    seen = []
    srv = Server(coord=LocalCoordinator()).configure(
        {"fns": _toy_fns(seen, cols, reducefn_gpu=name), "verbose": False})
    assert srv._gpu_engine_kind() == "window"
    srv.loop()
    assert seen == exp
    assert srv.stats["tier"] == "gpu"
    assert srv.stats["engine"] == "window:rolling"


@pytest.mark.parametrize("name,cols", [
    ("rolling:sum:5", 2), ("rolling:count:5", 3), ("rolling:mean:5,rows", 2)])
def test_wrong_arity_names_the_reducer(name, cols, monkeypatch):
    from mapreduce_amd.parallel.coord import LocalCoordinator
    from mapreduce_amd.server import Server

    monkeypatch.setenv("MR_GPU_TIER", "force")
    srv = Server(coord=LocalCoordinator()).configure(
        {"fns": _toy_fns([], cols, reducefn_gpu=name), "verbose": False})
    with pytest.raises(ValueError) as e:
        srv.loop()
    assert repr(name) in str(e.value) and "mapfn_gpu_pairs" in str(e.value)


def test_range_frames_over_a_float_order_column_are_refused(monkeypatch):
    from mapreduce_amd.parallel.coord import LocalCoordinator
    from mapreduce_amd.server import Server

    monkeypatch.setenv("MR_GPU_TIER", "force")
    rows = lambda k, v: ([1, 1, 1], [0.1, 0.3, 0.2], [1, 2, 3])
    srv = Server(coord=LocalCoordinator()).configure(
        {"fns": _toy_fns([], reducefn_gpu="rolling:sum:5",
                         mapfn_gpu_pairs=rows), "verbose": False})
    with pytest.raises(TypeError, match="int64 times"):
        srv.loop()
    seen = []
    srv = Server(coord=LocalCoordinator()).configure(
        {"fns": _toy_fns(seen, reducefn_gpu="rolling:sum:1,rows",
                         mapfn_gpu_pairs=rows), "verbose": False})
    srv.loop()
    assert seen == [(1, [(0.1, 1), (0.2, 4), (0.3, 5)])]


# ------------------------------------------------------------- the example

def _fresh_spend():
    import importlib

    import mapreduce_amd.examples.rolling_spend as rs
    from mapreduce_amd import job as jobmod
    importlib.reload(rs)
    jobmod._module_cache.clear()
    jobmod._inited.clear()
    return rs


def test_rolling_spend_gpu_tier_equals_host_tier(monkeypatch):
    from mapreduce_amd import run_local
    from mapreduce_amd.parallel.coord import LocalCoordinator
    from mapreduce_amd.server import Server

    args = {"seed": 4, "n": 1500, "nusers": 20, "splits": 3, "parts": 4}
    monkeypatch.setenv("MR_GPU_TIER", "off")
    rs = _fresh_spend()
    srv = run_local({"fns": {r: rs for r in ROLES}, "verbose": False,
                     "init_args": args}, nworkers=2)
    assert srv.finished and "tier" not in srv.stats
    host = dict(rs.RESULTS)

    # the answer from the rows themselves, one frame at a time
    groups = {}
    for u, ts, a in rs.make_rows(4, 1500, 20):
        groups.setdefault(u, []).append((ts, a))
    exp = {}
    for u, rows in groups.items():
        rows.sort()
        exp[u] = [(t, sum(a for s, a in rows if t - rs.WINDOW <= s <= t))
                  for t, _ in rows]
    assert host == exp and len(exp) > 5
    gaps = {b[0] - a[0] for rows in groups.values()
            for a, b in zip(rows, rows[1:])}
    assert {0, rs.WINDOW, rs.WINDOW + 1} <= gaps
    assert rs.window([(10, 1), (10, 2), (3610, 4), (3611, 8)]) == [
        (10, 3), (10, 3), (3610, 7), (3611, 12)]

    monkeypatch.setenv("MR_GPU_TIER", "force")
    rs = _fresh_spend()
    srv2 = Server(coord=LocalCoordinator()).configure(
        {"fns": {r: rs for r in ROLES}, "verbose": False,
         "init_args": args})
    assert srv2._gpu_engine_kind() == "window"
    srv2.loop()
    assert srv2.finished and srv2.stats["tier"] == "gpu"
    assert srv2.stats["engine"] == "window:rolling"
    assert dict(rs.RESULTS) == host
    assert list(rs.RESULTS) == sorted(rs.RESULTS)
    doc, _ = srv2.coord.get_doc("task_gpu")
    assert doc is not None and doc["status"] == "FINISHED"
