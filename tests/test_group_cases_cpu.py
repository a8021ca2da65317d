"""The group family without a GPU: the case generators, every op on the CPU
tier, GroupedValuesJob single rank and under gloo world=2, and the Server
routing of examples/percentiles.  Every comparison is exact against the
pure-Python oracle of group_common."""

import fractions
import os
import socket

import pytest
import torch

import group_common as gc
from mapreduce_amd import ops
from mapreduce_amd.gpu.grouped import GroupedValuesJob

T, QMAX = ops.group_caps()
R = ops.group_rank_max()
C = (T, R)
CASES = gc.cases(C)
SPECS = [(0, 1, False), (1, 2, False), (1, 2, True), (99, 100, False),
         (99, 100, True), (1, 1, False)]


# ------------------------------------------------------------ the generators

def test_case_generators_have_the_properties_the_gpu_tests_rely_on():
    assert (T, QMAX, R) == (ops.GROUP_TILE, ops.GROUP_QMAX,
                            ops.GROUP_RANK_MAX)
    assert 2 * R + 2 < T
    assert T & (T - 1) == 0 and T % 3 != 0
    none, every, some = set(), set(), set()
    for name, lens in CASES.items():
        n = sum(lens)
        s = gc.straddler_rows(lens, T)
        (none if s == 0 else every if s == n else some).add(name)
        keys = gc.case_keys(lens)
        assert keys == sorted(keys) and len(set(keys)) == len(lens), name
        assert n < 25_000, name
    assert {"n0", "n1", "singles", "tile_exact", "rank_max",
            "rank_over"} <= none
    # the threshold between the tile kernel's two sorts, from both sides
    assert max(CASES["rank_max"]) == R and max(CASES["rank_over"]) == R + 1
    assert max(CASES["short_random"]) <= R and sum(CASES["rank_over"]) < T
    # short groups on either side of a group that leaves its tile
    off = gc.offsets_of(CASES["short_then_long"])
    assert off[1] < R and off[2] // T == 1 and off[3] - off[2] < R
    assert {"long", "whole"} <= every
    assert {"straddle_by_one", "last_row_start", "threes", "mix",
            "short_then_long"} <= some
    # sizes and shapes named by the cases
    assert [sum(CASES[c]) for c in ("n0", "n1", "n2_one", "n2_two")] == [
        0, 1, 2, 2]
    assert sum(CASES["singles"]) == T + 3
    assert sum(CASES["threes"]) == 3 * T + 1
    # a group of three lies across both inner tile boundaries of "threes"
    # (T is a power of two); the last row is a group of its own at 3T
    off = gc.offsets_of(CASES["threes"])
    assert T not in off and 2 * T not in off and off[-2] == 3 * T
    # straddles by exactly one row; a group beginning on a tile's last row
    assert gc.offsets_of(CASES["straddle_by_one"])[1:] == [T - 1, T + 1]
    assert gc.offsets_of(CASES["last_row_start"])[1] == T - 1
    assert gc.straddler_rows(CASES["mix"], T) == 2 + T + 2 * T + 1
    # keys straddle the sign bit: the i64 view is not ascending
    sk = gc.to_i64(gc.case_keys(CASES["mix"])).tolist()
    assert sk != sorted(sk)
    # the f64 family holds what the order key canonicalises
    bits = set(gc.to_bits(gc.case_values("f64", 400)))
    assert {0, gc.SIGN} <= bits and set(gc.NAN_BITS) <= bits
    assert gc.f64_bits(5e-324) in bits and gc.f64_bits(float("inf")) in bits
    vals = gc.case_values("random_i64", 50).tolist()
    assert gc.I64_MIN in vals and gc.I64_MAX in vals


def test_order_key_rules():
    f = gc.f64_bits
    ok = lambda x: gc.okey(f(x), True)
    assert ok(-0.0) == ok(0.0)
    assert ok(float("-inf")) < ok(-1.5) < ok(-5e-324) < ok(0.0) < ok(5e-324)
    assert ok(1.5) < ok(float("inf")) < gc.okey(gc.NAN_BITS[0], True)
    assert len({gc.okey(b, True) for b in gc.NAN_BITS}) == 1
    assert gc.okey(gc.I64_MIN & gc.M64, False) == 0
    assert gc.okey(gc.I64_MAX, False) == gc.M64
    # the CPU tier's order keys are these
    for fam in ("random_i64", "f64"):
        v = gc.case_values(fam, 300)
        assert gc.to_bits(ops.group_order_keys(v)) == gc.okeys(v)


# -------------------------------------------------------------------- the ops

@pytest.mark.parametrize("family", gc.FAMILIES)
@pytest.mark.parametrize("name", sorted(CASES))
def test_ops_cpu_match_oracle(name, family):
    keys, vals, off = gc.case_data(C, name, family)
    exp_ok, exp_bits = gc.expected(C, name, family)
    kbuf, vbuf, kv, vv = gc.baited(keys, vals)
    k0, v0 = kbuf.clone(), vbuf.view(torch.int64).clone()
    uk, offsets = ops.group_by_key_sorted(kv)
    assert offsets.tolist() == off
    assert gc.to_bits(uk) == [gc.to_bits(keys)[a] for a in off[:-1]]
    out = ops.sort_values_in_groups(kv, vv)
    assert out.dtype == vals.dtype
    assert gc.to_bits(out) == exp_bits
    assert gc.okeys(out) == exp_ok
    assert torch.equal(kbuf, k0) and torch.equal(vbuf.view(torch.int64), v0)
    assert not off[1:] or out.data_ptr() != vv.data_ptr()
    if not off[1:]:
        return
    for higher in (False, True):
        specs = [s for s in SPECS if s[2] == higher]
        got = ops.group_quantiles(
            offsets, out, [(n, d) for n, d, _ in specs],
            "higher" if higher else "lower")
        assert [gc.okeys(r) for r in got] == gc.oracle_quantiles(
            off, exp_ok, specs)
    longest = max(b - a for a, b in zip(off, off[1:]))
    for k in (1, 3, longest + 2) if longest < 100 else (1, 3):
        for largest in (True, False):
            top, cnt = ops.group_topk(offsets, out, k, largest)
            rows, ecnt = gc.oracle_topk(off, exp_ok, k, largest)
            assert cnt.tolist() == ecnt
            tb = [gc.okeys(r) for r in top]
            for r, e, c, raw in zip(tb, rows, ecnt, top):
                assert r[:c] == e[:c]
                assert gc.to_bits(raw)[c:] == [0] * (k - c)
    assert ops.group_distinct(kv, out).tolist() == gc.oracle_distinct(
        off, vals)


def test_quantile_fractions_and_refusals():
    keys, vals, off = gc.case_data(C, "short_random", "f64")
    _, offsets = ops.group_by_key_sorted(keys)
    sv = ops.sort_values_in_groups(keys, vals)
    a = ops.group_quantiles(offsets, sv, [fractions.Fraction(1, 2), (2, 4)])
    assert gc.okeys(a[:, 0]) == gc.okeys(a[:, 1])
    full = ops.group_quantiles(offsets, sv, [(i, 7) for i in range(QMAX)])
    assert tuple(full.shape) == (len(off) - 1, QMAX)
    with pytest.raises(TypeError, match="float"):
        ops.group_quantiles(offsets, sv, [0.5])
    with pytest.raises(ValueError, match="den"):
        ops.group_quantiles(offsets, sv, [(0, 0)])
    with pytest.raises(ValueError, match="den"):
        ops.group_quantiles(offsets, sv, [(1, 10 ** 6 + 1)])
    with pytest.raises(ValueError, match="num"):
        ops.group_quantiles(offsets, sv, [(-1, 2)])
    with pytest.raises(ValueError, match="num"):
        ops.group_quantiles(offsets, sv, [(3, 2)])
    with pytest.raises(ValueError, match="Q must be"):
        ops.group_quantiles(offsets, sv, [])
    with pytest.raises(ValueError, match="Q must be"):
        ops.group_quantiles(offsets, sv, [(1, 2)] * (QMAX + 1))
    with pytest.raises(ValueError, match="interpolation"):
        ops.group_quantiles(offsets, sv, [(1, 2)], "linear")
    with pytest.raises(ValueError, match="k must be"):
        ops.group_topk(offsets, sv, 0)
    with pytest.raises(TypeError, match="int64 or float64"):
        ops.sort_values_in_groups(keys, vals.to(torch.float32))
    with pytest.raises(ValueError, match="one value per key"):
        ops.sort_values_in_groups(keys, vals[:-1])


def test_two_sort_knob_is_a_no_op_on_the_cpu_tier(monkeypatch):
    keys, vals, _ = gc.case_data(C, "mix", "f64")
    _, exp_bits = gc.expected(C, "mix", "f64")
    monkeypatch.setenv("MR_GROUP_TWO_SORT", "1")
    assert gc.to_bits(ops.sort_values_in_groups(keys, vals)) == exp_bits


# ------------------------------------------------------------ single rank

@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("combine", gc.COMBINES, ids=str)
def test_grouped_job_single_rank(combine, f64):
    keys, vals = gc.make_rows(21, 900, 60, f64, hot=150)
    keep = keys.clone(), vals.view(torch.int64).clone()
    res = GroupedValuesJob("cpu", combine=combine).run(keys, vals)
    exp = gc.job_oracle(keys, vals, combine)
    assert gc.job_lists(res) == exp and len(exp[0]) > 50
    assert res.values.dtype == vals.dtype
    assert torch.equal(keys, keep[0])
    assert torch.equal(vals.view(torch.int64), keep[1])
    # the result's own methods
    uk, off, ok = exp
    lens = [b - a for a, b in zip(off, off[1:])]
    assert res.counts().tolist() == lens
    assert gc.okeys(res.median()) == [
        ok[a + (b - a - 1) // 2] for a, b in zip(off, off[1:])]
    assert res.distinct().tolist() == [
        len(set(ok[a:b])) for a, b in zip(off, off[1:])]
    top, cnt = res.topk(2)
    assert cnt.tolist() == [min(2, n) for n in lens]
    host = res.to_host()
    assert [k & gc.M64 for k, _ in host] == uk
    assert [len(v) for _, v in host] == lens


def test_grouped_job_empty_and_refusals():
    e = torch.empty(0, dtype=torch.int64)
    res = GroupedValuesJob("cpu").run(e, e.view(torch.float64))
    assert res.keys.numel() == 0 and res.offsets.tolist() == [0]
    assert res.values.dtype == torch.float64
    assert res.distinct().numel() == 0 and res.to_host() == []
    for bad in ("median", ("topk", 0), ("topk", 2.0), ("best", 3)):
        with pytest.raises(ValueError, match="combine"):
            GroupedValuesJob("cpu", combine=bad)
    with pytest.raises(TypeError, match="int64 or float64"):
        GroupedValuesJob("cpu").run(torch.zeros(3, dtype=torch.int64),
                                    torch.zeros(3, dtype=torch.float32))


# ------------------------------------------------------------- gloo world=2

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _rank_inputs(rank, starve):
    # the starved variant carries f64 values, the other i64
    keys, vals = gc.make_rows(300 + rank, 700, 50, starve, hot=90)
    if starve and rank == 1:  # this rank stages nothing
        keys, vals = keys[:0], vals[:0]
    return keys, vals


def _ws2_worker(rank, world, port, starve):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.distributed.init_process_group("gloo", rank=rank, world_size=world)
    try:
        keys, vals = _rank_inputs(rank, starve)
        ins = [_rank_inputs(r, starve) for r in range(world)]
        allk = torch.cat([i[0] for i in ins])
        allv = torch.cat([i[1] for i in ins])
        for combine in gc.COMBINES:
            res = GroupedValuesJob("cpu", combine=combine).run(keys, vals)
            assert res.values.dtype == allv.dtype
            mine = gc.job_lists(res)
            # each shard holds only its own keys (mulhi partition)
            assert all((k * world) >> 64 == rank for k in mine[0])
            shards = [None] * world
            torch.distributed.all_gather_object(shards, mine)
            if rank == 0:
                # rank-major shards are the single-rank result over the
                # ranks' inputs together (test_grouped_job_single_rank
                # holds the job to this oracle at world 1)
                uk, off, ok = gc.job_oracle(allk, allv, combine)
                assert len(uk) > 40
                assert [x for s in shards for x in s[0]] == uk, combine
                assert [x for s in shards for x in s[2]] == ok, combine
                lens = [b - a for s in shards
                        for a, b in zip(s[1], s[1][1:])]
                assert lens == [b - a for a, b in zip(off, off[1:])]
    finally:
        torch.distributed.destroy_process_group()


@pytest.mark.timeout(180)
@pytest.mark.parametrize("starve", [False, True])
def test_grouped_job_gloo_ws2(starve):
    torch.multiprocessing.spawn(
        _ws2_worker, args=(2, _free_port(), starve), nprocs=2, join=True)


# ---------------------------------------------------------- Server routing

ROLES = ("taskfn", "mapfn", "partitionfn", "reducefn", "finalfn")


def _fresh_percentiles():
    import importlib

    import mapreduce_amd.examples.percentiles as pc
    from mapreduce_amd import job as jobmod
    importlib.reload(pc)
    jobmod._module_cache.clear()
    jobmod._inited.clear()
    return pc


def test_percentiles_gpu_tier_equals_host_tier(monkeypatch):
    from mapreduce_amd import run_local
    from mapreduce_amd.parallel.coord import LocalCoordinator
    from mapreduce_amd.server import Server

    args = {"seed": 4, "n": 1500, "nendpoints": 20, "splits": 3, "parts": 4}
    monkeypatch.setenv("MR_GPU_TIER", "off")
    pc = _fresh_percentiles()
    srv = run_local({"fns": {r: pc for r in ROLES}, "verbose": False,
                     "init_args": args}, nworkers=2)
    assert srv.finished and "tier" not in srv.stats
    host = dict(pc.RESULTS)

    # the answer from the rows themselves
    groups = {}
    for e, ms in pc.make_rows(4, 1500, 20):
        groups.setdefault(e, []).append(ms)
    exp = {}
    for e, vs in groups.items():
        s = sorted(vs)
        exp[e] = tuple(s[(n * (len(s) - 1)) // d] for n, d in pc.FRACS)
    assert host == exp and len(exp) > 5

    monkeypatch.setenv("MR_GPU_TIER", "force")
    pc = _fresh_percentiles()
    srv2 = Server(coord=LocalCoordinator()).configure(
        {"fns": {r: pc for r in ROLES}, "verbose": False,
         "init_args": args})
    assert srv2._gpu_engine_kind() == "group"
    srv2.loop()
    assert srv2.finished and srv2.stats["tier"] == "gpu"
    assert srv2.stats["engine"] == "group:quantile"
    assert dict(pc.RESULTS) == host
    assert list(pc.RESULTS) == sorted(pc.RESULTS)
    doc, _ = srv2.coord.get_doc("task_gpu")
    assert doc is not None and doc["status"] == "FINISHED"


ROWS = [(2, 5), (1, 7), (2, -3), (1, 7), (2, 5), (3, 0), (2, 9)]


def _toy_fns(seen, **over):
    fns = {
        "taskfn": lambda emit: emit(1, "x"),
        "mapfn": lambda k, v, emit: None,
        "mapfn_gpu_pairs": lambda k, v: ([r[0] for r in ROWS],
                                         [r[1] for r in ROWS]),
        "partitionfn": lambda k: 0,
        "reducefn": lambda k, vs, emit: emit(sum(vs)),
        "finalfn": lambda pairs: seen.extend(pairs) or True,
    }
    fns.update(over)
    return {r: fns for r in ROLES + ("combinerfn",)}


@pytest.mark.parametrize("name,exp", [
    ("group", [(1, [7, 7]), (2, [-3, 5, 5, 9]), (3, [0])]),
    ("median", [(1, [7]), (2, [5]), (3, [0])]),
    ("quantile:1/1", [(1, [7]), (2, [9]), (3, [0])]),
    ("quantile:0/1,1/2,1/1", [(1, [(7, 7, 7)]), (2, [(-3, 5, 9)]),
                              (3, [(0, 0, 0)])]),
    ("topk:2", [(1, [7, 7]), (2, [9, 5]), (3, [0])]),
    ("bottomk:3", [(1, [7, 7]), (2, [-3, 5, 5]), (3, [0])]),
    ("distinct", [(1, [1]), (2, [3]), (3, [1])]),
])
def test_group_reducers_hand_finalfn_the_documented_pairs(name, exp,
                                                          monkeypatch):
    from mapreduce_amd.parallel.coord import LocalCoordinator
    from mapreduce_amd.server import Server

    monkeypatch.setenv("MR_GPU_TIER", "force")
    seen = []
    srv = Server(coord=LocalCoordinator()).configure(
        {"fns": _toy_fns(seen, reducefn_gpu=name), "verbose": False})
    assert srv._gpu_engine_kind() == "group"
    srv.loop()
    assert seen == exp
    assert srv.stats["tier"] == "gpu"
    assert srv.stats["engine"] == "group:" + name.split(":")[0]


@pytest.mark.parametrize("name", [
    "quantile", "quantile:", "quantile:1", "quantile:1/0", "quantile:3/2",
    "quantile:1/2,", "quantile:0.5", "quantile:-1/2", "quantile:1/1000001",
    "quantile:" + ",".join(["1/2"] * 9), "topk", "topk:", "topk:0",
    "topk:x", "topk:-1", "bottomk:1.5", "median:2", "group:1", "distinct:x"])
def test_malformed_group_reducers_are_refused(name, monkeypatch):
    from mapreduce_amd.parallel.coord import LocalCoordinator
    from mapreduce_amd.server import Server

    monkeypatch.setenv("MR_GPU_TIER", "force")
    with pytest.raises(ValueError) as e:
        Server(coord=LocalCoordinator()).configure(
            {"fns": _toy_fns([], reducefn_gpu=name), "verbose": False}
        ).loop()
    assert repr(name) in str(e.value)


def test_sum_reducer_still_routes_to_pairs_beside_group(monkeypatch):
    from mapreduce_amd.parallel.coord import LocalCoordinator
    from mapreduce_amd.server import Server

    monkeypatch.setenv("MR_GPU_TIER", "force")
    srv = Server(coord=LocalCoordinator()).configure(
        {"fns": _toy_fns([], reducefn_gpu="sum", associative_reducer=True,
                         commutative_reducer=True), "verbose": False})
    assert srv._gpu_engine_kind() == "pairs"
    srv = Server(coord=LocalCoordinator()).configure(
        {"fns": _toy_fns([], reducefn_gpu="join"), "verbose": False})
    assert srv._gpu_engine_kind() == "join"
    for name in ("group", "median", "quantile:1/2", "topk:3", "bottomk:1",
                 "distinct"):
        srv = Server(coord=LocalCoordinator()).configure(
            {"fns": _toy_fns([], reducefn_gpu=name), "verbose": False})
        assert srv._gpu_engine_kind() == "group"
    # without the staging hook the name decides nothing
    fns = _toy_fns([], reducefn_gpu="median")
    for r in fns.values():
        r.pop("mapfn_gpu_pairs", None)
    srv = Server(coord=LocalCoordinator()).configure(
        {"fns": fns, "verbose": False})
    assert srv._gpu_engine_kind() is None
