"""The as-of family without a GPU: ops.asof_sorted on the CPU tier,
AsofJoinJob single rank and under gloo world=2, and the Server routing of
examples/asof_quotes.  Every comparison is exact against the brute-force
oracle of asof_common."""

import os
import socket

import pytest
import torch

import asof_common as ac
from mapreduce_amd import ops
from mapreduce_amd.gpu.asof import AsofJoinJob

CAPS = ops.asof_caps()
T, W = CAPS
CASES = ac.cases(*CAPS)


# ---------------------------------------------------------------- the op

@pytest.mark.parametrize("direction", ac.DIRECTIONS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_asof_sorted_cpu_matches_oracle(name, direction):
    case = CASES[name]
    bufs, views = ac.baited(case)
    keep = [b.clone() for b in bufs]
    for d, exact, tol in ac.modes(case):
        if d != direction:
            continue
        got = ops.asof_sorted(*views, direction=d, tolerance=tol,
                              allow_exact=exact)
        assert got.dtype == torch.int64
        assert got.tolist() == ac.expected(CAPS, name, d, exact, tol), (
            d, exact, tol)
    for b, k in zip(bufs, keep):
        assert torch.equal(b.view(torch.int64), k.view(torch.int64))


def _exp(name, d="backward", exact=True, tol=None):
    return ac.expected(CAPS, name, d, exact, tol)


def test_case_generators_have_the_properties_the_gpu_tests_rely_on():
    seen_l, seen_r = set(), set()
    for name, c in CASES.items():
        for k, t in ((c.lk, c.lt), (c.rk, c.rt)):
            rows = [(a, ac.okey(b, c.f64)) for a, b in zip(k, t)]
            assert rows == sorted(rows), name
            assert len(rows) <= 3 * max(T, W) + 17, name
        if name.startswith("dup_"):
            seen_l.add(len(c.lk))
            seen_r.add(len(c.rk))
            if len(c.lk) >= 63 and len(c.rk) >= 63:
                # some rows match and the mid tolerance cuts some of them
                full = _exp(name)
                cut = _exp(name, tol=ac.TOL_MID)
                assert any(r >= 0 for r in cut) and cut != full, name
    assert seen_l >= set(ac.sizes(T)) and seen_r >= set(ac.sizes(T))
    assert all(r == -1 for r in _exp("disjoint", "nearest"))
    n = len(CASES["identical"].lk)
    assert n > 2 * T and _exp("identical") == list(range(n))
    assert _exp("identical", "forward") == list(range(n))

    # heavy duplicates: backward and forward differ on exact matches
    c = CASES["heavy"]
    assert len(set(zip(c.rk, c.rt))) <= 15
    assert _exp("heavy") != _exp("heavy", "forward")
    # a run of equal (key, time): backward takes the last, forward the first
    assert _exp("all_equal") == [299] * 300
    assert _exp("all_equal", "forward") == [0] * 300
    assert _exp("all_equal", "nearest") == [299] * 300  # the tie
    assert _exp("all_equal", "nearest", exact=False) == [-1] * 300

    # the windows: exactly W and W + 1 right rows under tile 0
    for extra in (0, 1):
        for suffix, tiles in (("", 1), ("_tiles", 2)):
            name = f"window_{W + extra}{suffix}"
            c = CASES[name]
            assert (len(c.lk) + T - 1) // T == tiles, name
            lo, hi = ac.window(CAPS, name, 0)
            assert hi - lo == W + extra, name
            assert any(r >= 0 for r in _exp(name)[-3:])
            if tiles == 2:
                lo, hi = ac.window(CAPS, name, 1)
                assert 0 < hi - lo <= W and lo > 0
    # the global fallback: three left rows over more than W right rows
    c = CASES["hot_fallback"]
    lo, hi = ac.window(CAPS, "hot_fallback", 0)
    assert len(c.lk) == 3 and hi - lo > 3 * W
    assert all(r >= 0 for r in _exp("hot_fallback"))
    # the run of equal right rows starts inside tile 0's window and ends
    # behind it; tile 1 starts on the run
    c = CASES["run_across_window_end"]
    lo, hi = ac.window(CAPS, "run_across_window_end", 0)
    run = [j for j, t in enumerate(c.rt) if t == 110]
    assert len(run) == 50 and run[0] == hi - 1 and run[-1] >= hi
    assert _exp("run_across_window_end", "forward", exact=False)[T - 1] == \
        run[0]
    assert c.lt[T] == 110 and _exp("run_across_window_end")[T] == run[-1]
    assert _exp("run_across_window_end", "forward")[T] == run[0]

    # sign bit: the i64 view of the sorted u64 column is NOT ascending
    sk = ac.to_i64(CASES["sign_keys"].lk).tolist()
    assert sk != sorted(sk)
    # a span over 2^63 matches without a tolerance and under none
    full = _exp("extreme_span")
    assert full[:3] == [0, 1, 2] and full[3:] == [-1, -1, -1]
    assert _exp("extreme_span", "forward")[3:] == [3, 4, 5]
    for tol in (0, 1):
        assert _exp("extreme_span", "nearest", tol=tol) == [-1] * 6
    top = _exp("extreme_span", "nearest", tol=ac.I64_MAX)
    assert top == [-1, -1, 2, -1, -1, 5]
    # exactly tol matches, tol + 1 does not
    assert _exp("tol_edge", "nearest", tol=ac.TOL_MID) == [0, -1, 2, -1, 4]
    assert _exp("tol_edge", "nearest", tol=ac.TOL_MID - 1) == [-1] * 5
    assert _exp("tol_edge", "nearest") == [0, 1, 2, 3, 4]
    # no leak across keys, forward or backward
    c = CASES["empty_run"]
    for d in ac.DIRECTIONS:
        got = _exp("empty_run", d)
        assert [got[i] for i, k in enumerate(c.lk) if k == 20] == [-1] * 3
    assert _exp("empty_run", "forward") == [0, -1, -1, -1, -1, 3, -1]
    assert _exp("empty_run") == [-1, 2, -1, -1, -1, -1, 5]
    # f64: -0.0 and +0.0 are one time, NaN is a time above +inf
    c = CASES["f64_specials"]
    got = _exp("f64_specials")
    z = [i for i, (k, t) in enumerate(zip(c.lk, c.lt)) if k == 1 and t == 0]
    assert len(z) == 2 and got[z[0]] == got[z[1]]
    assert sorted(ac.f64_bits(c.rt[j]) >> 63
                  for j in range(got[z[0]] - 3, got[z[0]] + 1)) == [0, 0, 1, 1]
    nan = [i for i, (k, t) in enumerate(zip(c.lk, c.lt)) if k == 1 and t != t]
    assert c.rt[got[nan[0]]] != c.rt[got[nan[0]]]
    assert c.rt[_exp("f64_specials", exact=False)[nan[0]]] == ac.INF


def test_asof_sorted_refusals():
    k = ac.to_i64([1, 2, 2, 3])
    t = torch.tensor([1, 2, 3, 4])
    f = t.to(torch.float64)
    assert ops.asof_sorted(k, t, k, t).tolist() == [0, 1, 2, 3]
    with pytest.raises(ValueError, match="direction"):
        ops.asof_sorted(k, t, k, t, direction="sideways")
    with pytest.raises(TypeError):
        ops.asof_sorted(k.to(torch.int32), t, k, t)
    with pytest.raises(TypeError):
        ops.asof_sorted(k, t.to(torch.int32), k, t.to(torch.int32))
    with pytest.raises(TypeError, match="dtype"):
        ops.asof_sorted(k, t, k, f)
    with pytest.raises(TypeError, match="tolerance"):
        ops.asof_sorted(k, f, k, f, tolerance=1)
    with pytest.raises(TypeError, match="tolerance"):
        ops.asof_sorted(k, t, k, t, tolerance=1.0)
    for tol in (-1, 2 ** 63):
        with pytest.raises(ValueError, match="tolerance"):
            ops.asof_sorted(k, t, k, t, tolerance=tol)
    ops.asof_sorted(k, t, k, t, tolerance=2 ** 63 - 1)
    with pytest.raises(ValueError, match="one time per key"):
        ops.asof_sorted(k, t[:3], k, t)
    with pytest.raises(ValueError, match="one time per key"):
        ops.asof_sorted(k, t, k[:2], t)
    assert ops.asof_caps() == (ops.ASOF_TILE, ops.ASOF_WIN)


# ------------------------------------------------------------ single rank

JOB_MODES = [("backward", None, True), ("forward", 3, True),
             ("nearest", None, False), ("nearest", 2, True)]


def _job_inputs(tf64, vf64, nl=700, nr=500, nkeys=60):
    lk, lt, lv = ac.make_relation(21, nl, nkeys, tf64, vf64)
    rk, rt, rv = ac.make_relation(22, nr, nkeys + 20, tf64, not vf64)
    rk[:200] = lk[:200]  # shared keys beyond the pools' own overlap
    return lk, lt, lv, rk, rt, rv


@pytest.mark.parametrize("how", ("left", "inner"))
@pytest.mark.parametrize("tf64,vf64", [(False, False), (True, True),
                                       (False, True)])
def test_asof_job_single_rank(tf64, vf64, how):
    cols = _job_inputs(tf64, vf64)
    keep = [c.clone() for c in cols]
    for direction, tol, exact in JOB_MODES:
        if tf64 and tol is not None:
            continue
        res = AsofJoinJob("cpu", direction=direction, tolerance=tol,
                          allow_exact=exact, how=how).run(*cols)
        exp = ac.job_oracle(*cols, direction, tol, exact, how)
        assert ac.job_rows(res) == exp, (direction, tol, exact)
        assert any(r[5] for r in exp)
        assert (how == "inner") or not all(r[5] for r in exp)
        assert res.ltimes.dtype == res.rtimes.dtype == cols[1].dtype
        assert res.lvals.dtype == cols[2].dtype
        assert res.rvals.dtype == cols[5].dtype
        assert (res.matched is None) == (how == "inner")
    for c, k in zip(cols, keep):
        assert torch.equal(c.view(torch.int64), k.view(torch.int64))


@pytest.mark.parametrize("tf64", (False, True))
def test_asof_job_is_invariant_under_a_shuffle_of_the_rows(tf64):
    cols = _job_inputs(tf64, True)
    base = None
    for seed in (None, 1, 2):
        cur = cols
        if seed is not None:
            g = torch.Generator().manual_seed(seed)
            pl = torch.randperm(cols[0].numel(), generator=g)
            pr = torch.randperm(cols[3].numel(), generator=g)
            cur = [c[pl] for c in cols[:3]] + [c[pr] for c in cols[3:]]
        for direction in ("backward", "forward"):
            rows = ac.canonical(ac.job_rows(
                AsofJoinJob("cpu", direction=direction).run(*cur)),
                tf64, True, False)
            if seed is None:
                base = base or {}
                base[direction] = rows
            else:
                assert rows == base[direction]
    # equal (key, time) right rows: backward the largest value, forward
    # the smallest
    k = ac.to_i64([5, 5, 5])
    t = torch.tensor([3, 3, 3])
    v = torch.tensor([20, 10, 30])
    one = (ac.to_i64([5]), torch.tensor([3]), torch.tensor([1]))
    assert AsofJoinJob("cpu").run(*one, k, t, v).rvals.tolist() == [30]
    assert AsofJoinJob("cpu", direction="forward").run(
        *one, k, t, v).rvals.tolist() == [10]


def test_asof_job_empty_sides_and_refusals():
    lk, lt, lv = ac.make_relation(3, 40, 8, False, True)
    e = torch.empty(0, dtype=torch.int64)
    ef = torch.empty(0, dtype=torch.float64)
    for how in ("left", "inner"):
        res = AsofJoinJob("cpu", how=how).run(lk, lt, lv, e, e, ef)
        assert ac.job_rows(res) == ac.job_oracle(lk, lt, lv, e, e, ef,
                                                 how=how)
        assert res.keys.numel() == (40 if how == "left" else 0)
        assert res.rvals.dtype == torch.float64
        assert res.rtimes.dtype == torch.int64
        res = AsofJoinJob("cpu", how=how).run(e, e, ef, lk, lt, lv)
        assert res.keys.numel() == 0 and res.lvals.dtype == torch.float64
        res = AsofJoinJob("cpu", how=how).run(e, e, e, e, e, e)
        assert res.keys.numel() == 0
    with pytest.raises(ValueError, match="how"):
        AsofJoinJob("cpu", how="outer")
    with pytest.raises(ValueError, match="direction"):
        AsofJoinJob("cpu", direction="sideways")
    with pytest.raises(ValueError, match="tolerance"):
        AsofJoinJob("cpu", tolerance=-1)
    with pytest.raises(TypeError, match="dtype"):
        AsofJoinJob("cpu").run(lk, lt, lv, lk, lt.to(torch.float64), lv)
    with pytest.raises(ValueError, match="per left key"):
        AsofJoinJob("cpu").run(lk, lt[:5], lv, lk, lt, lv)
    with pytest.raises(ValueError, match="per right"):
        AsofJoinJob("cpu").run(lk, lt, lv, lk, lt, lv[:5])
    with pytest.raises(TypeError, match="tolerance"):
        AsofJoinJob("cpu", tolerance=1).run(
            lk, lt.to(torch.float64), lv, lk, lt.to(torch.float64), lv)


# ------------------------------------------------------------- gloo world=2

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _rank_inputs(rank):
    lk, lt, lv = ac.make_relation(100 + rank, 600, 80, False, False)
    rk, rt, rv = ac.make_relation(200 + rank, 450, 80, False, True)
    rk[:150] = lk[:150]
    if rank == 1:  # this rank stages nothing on the right
        rk, rt, rv = rk[:0], rt[:0], rv[:0]
    return lk, lt, lv, rk, rt, rv


def _ws2_worker(rank, world, port):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.distributed.init_process_group("gloo", rank=rank, world_size=world)
    try:
        job = AsofJoinJob("cpu", direction="nearest", tolerance=4)
        mine = ac.job_rows(job.run(*_rank_inputs(rank)))
        # each shard holds only its own keys (mulhi partition)
        assert all((r[0] * world) >> 64 == rank for r in mine)
        shards = [None] * world
        torch.distributed.all_gather_object(shards, mine)
        if rank == 0:
            # the world=1 result over the ranks' inputs concatenated:
            # rank-major shards are the global key order
            ins = [_rank_inputs(r) for r in range(world)]
            cat = [torch.cat([i[c] for i in ins]) for c in range(6)]
            exp = ac.job_oracle(*cat, "nearest", 4, True, "left")
            assert any(r[5] for r in exp) and not all(r[5] for r in exp)
            got = [r for s in shards for r in s]
            assert ac.canonical(got, False, False, True) == ac.canonical(
                exp, False, False, True)
            assert all(s for s in shards)
    finally:
        torch.distributed.destroy_process_group()


@pytest.mark.timeout(180)
def test_asof_job_gloo_ws2():
    torch.multiprocessing.spawn(
        _ws2_worker, args=(2, _free_port()), nprocs=2, join=True)


# ---------------------------------------------------------- Server routing

def _fresh_asof_quotes():
    import importlib

    import mapreduce_amd.examples.asof_quotes as aq
    from mapreduce_amd import job as jobmod
    importlib.reload(aq)
    jobmod._module_cache.clear()
    jobmod._inited.clear()
    return aq


ROLES = ("taskfn", "mapfn", "partitionfn", "reducefn", "finalfn")


@pytest.mark.parametrize("opts", [
    {"direction": "backward"},
    {"direction": "forward", "tolerance": 3},
    {"direction": "nearest", "strict": True, "inner": True},
], ids=("backward", "forward_tol", "nearest_strict_inner"))
def test_asof_quotes_gpu_tier_equals_host_tier(opts, monkeypatch):
    from mapreduce_amd import run_local
    from mapreduce_amd.parallel.coord import LocalCoordinator
    from mapreduce_amd.server import Server

    args = dict(opts, seed=5, nl=300, nr=240, nkeys=30, splits=3, parts=4)
    monkeypatch.setenv("MR_GPU_TIER", "off")
    aq = _fresh_asof_quotes()
    srv = run_local({"fns": {r: aq for r in ROLES}, "verbose": False,
                     "init_args": args}, nworkers=2)
    assert srv.finished and "tier" not in srv.stats
    host = dict(aq.RESULTS)
    assert host

    left, right = aq.make_relations(5, 300, 240, 30)
    exp = ac.brute_quotes(left, right, opts["direction"],
                        opts.get("tolerance"), opts.get("strict", False),
                        opts.get("inner", False))
    exp = {k: sorted(v, key=aq._order) for k, v in exp.items()}
    assert host == exp
    rows = [r for v in exp.values() for r in v]
    assert any(r[2] is not None for r in rows)
    if not opts.get("inner"):
        assert any(r[2] is None for r in rows)

    monkeypatch.setenv("MR_GPU_TIER", "force")
    aq = _fresh_asof_quotes()
    srv2 = Server(coord=LocalCoordinator()).configure(
        {"fns": {r: aq for r in ROLES}, "verbose": False,
         "init_args": args})
    assert srv2._gpu_engine_kind() == "asof"
    srv2.loop()
    assert srv2.finished and srv2.stats["tier"] == "gpu"
    assert srv2.stats["engine"] == "asof"
    assert dict(aq.RESULTS) == host
    # finalfn saw the keys in global key order
    assert list(aq.RESULTS) == sorted(aq.RESULTS)
    doc, _ = srv2.coord.get_doc("task_gpu")
    assert doc is not None and doc["status"] == "FINISHED"


def test_parse_asof_reducer():
    from mapreduce_amd.server import Server

    p = Server.parse_asof_reducer
    base = {"direction": "backward", "allow_exact": True, "how": "left",
            "tolerance": None}
    assert p("join_asof") == base
    assert p("join_asof:backward") == base
    assert p("join_asof:forward") == dict(base, direction="forward")
    assert p("join_asof:strict") == dict(base, allow_exact=False)
    assert p("join_asof:inner,nearest") == dict(base, how="inner",
                                                direction="nearest")
    assert p("join_asof:tol=0") == dict(base, tolerance=0)
    assert p("join_asof:nearest,strict,inner,tol=9223372036854775807") == {
        "direction": "nearest", "allow_exact": False, "how": "inner",
        "tolerance": 2 ** 63 - 1}
    for bad in ("join_asof:", "join_asof:sideways", "join_asof:backward,",
                "join_asof:backward,forward", "join_asof:strict,strict",
                "join_asof:tol=", "join_asof:tol=-1", "join_asof:tol=1.5",
                "join_asof:tol=9223372036854775808", "join_asof:tol=1,tol=2",
                "join_asof:Backward", "join_asof: forward",
                "join_asof:inner,inner", "join_asof:tol=+1"):
        with pytest.raises(ValueError) as e:
            p(bad)
        assert repr(bad) in str(e.value)
    for other in ("join", "join_left", "join_asof2", "asof", "cumsum",
                  "sessions:5", "sum", "median", "sort", None, 5):
        assert p(other) is None
    # the sibling parsers do not claim the name either
    assert Server.parse_group_reducer("join_asof:forward") is None
    assert Server.parse_window_reducer("join_asof:forward") is None


def _toy_fns(**over):
    fns = {
        "taskfn": lambda emit: emit(1, "x"),
        "mapfn": lambda k, v, emit: None,
        "mapfn_gpu_pairs": lambda k, v: ([1, 1, 2], [10, 20, 30],
                                         [1, 2, 3]),
        "partitionfn": lambda k: 0,
        "reducefn": lambda k, vs, emit: emit(sum(vs)),
        "finalfn": lambda pairs: True,
    }
    fns.update(over)
    return {r: fns for r in ROLES + ("combinerfn",)}


def _server(monkeypatch, **over):
    from mapreduce_amd.parallel.coord import LocalCoordinator
    from mapreduce_amd.server import Server

    monkeypatch.setenv("MR_GPU_TIER", "force")
    return Server(coord=LocalCoordinator()).configure(
        {"fns": _toy_fns(**over), "verbose": False})


def test_asof_refuses_a_three_tuple_from_the_staging_hook(monkeypatch):
    srv = _server(monkeypatch, reducefn_gpu="join_asof:forward")
    assert srv._gpu_engine_kind() == "asof"
    with pytest.raises(ValueError, match=r"mapfn_gpu_pairs.*\(keys, times, "
                                         r"vals, side\).*3-tuple"):
        srv.loop()
    srv = _server(monkeypatch, reducefn_gpu="join_asof",
                  mapfn_gpu_pairs=lambda k, v: ([1], [1], [1], 2))
    with pytest.raises(ValueError, match="mapfn_gpu_pairs"):
        srv.loop()


def test_asof_refuses_a_malformed_name_at_configure(monkeypatch):
    with pytest.raises(ValueError, match="join_asof:sideways"):
        _server(monkeypatch, reducefn_gpu="join_asof:sideways")


def test_asof_refuses_sides_with_different_time_dtypes(monkeypatch):
    srv = _server(
        monkeypatch, reducefn_gpu="join_asof",
        taskfn=lambda emit: (emit(0, "l"), emit(1, "r")),
        mapfn_gpu_pairs=lambda k, v: (
            ([1], [1], [5], 0) if v == "l" else ([1], [0.5], [6], 1)))
    with pytest.raises(TypeError, match="times"):
        srv.loop()


def test_asof_loop_hands_finalfn_rows_in_key_order(monkeypatch):
    seen = []
    srv = _server(
        monkeypatch, reducefn_gpu="join_asof",
        taskfn=lambda emit: (emit(0, "l"), emit(1, "r")),
        mapfn_gpu_pairs=lambda k, v: (
            ([2, 1, -1, 1], [5, 9, 1, 2], [1.5, 2.5, 3.5, 4.5], 0)
            if v == "l" else ([1, 1, 2], [3, 8, 6], [30, 80, 60], 1)),
        finalfn=lambda pairs: seen.extend(
            (k, [tuple(r) for r in rows]) for k, rows in pairs) or True)
    srv.loop()
    assert srv.stats["engine"] == "asof" and srv.stats["tier"] == "gpu"
    assert seen == [(1, [(2, 4.5, None, None), (9, 2.5, 8, 80)]),
                    (2, [(5, 1.5, None, None)]),
                    (-1, [(1, 3.5, None, None)])]


def test_other_reducers_still_route_to_their_own_kinds(monkeypatch):
    for name, kind in (("join", "join"), ("join_left", "join"),
                       ("cumsum", "window"), ("sessions:5", "window"),
                       ("median", "group"), ("sort", "sort"),
                       ("join_asof", "asof"), ("join_asof:tol=3", "asof")):
        assert _server(monkeypatch,
                       reducefn_gpu=name)._gpu_engine_kind() == kind
    srv = _server(monkeypatch, reducefn_gpu="sum", associative_reducer=True,
                  commutative_reducer=True)
    assert srv._gpu_engine_kind() == "pairs"
    assert _server(monkeypatch, reducefn_gpu="asof")._gpu_engine_kind() is None
