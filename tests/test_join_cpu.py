"""The join family without a GPU: ops.join_sorted on the CPU tier, JoinJob
single rank and under gloo world=2, and the Server routing of
examples/join_tables.  Every comparison is exact against the brute-force
oracle of join_common."""

import os
import socket

import pytest
import torch

import join_common as jc
from mapreduce_amd import ops
from mapreduce_amd.gpu.join import JoinJob

CAPS = ops.join_caps() + ops.join_bounds_caps()
T, S, BT, W = CAPS
CASES = jc.cases(*CAPS)


# ---------------------------------------------------------------- the op

@pytest.mark.parametrize("how", jc.HOWS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_join_sorted_cpu_matches_oracle(name, how):
    lk, rk = CASES[name]
    lbuf, rbuf, lv, rv = jc.baited(lk, rk)
    l0, r0 = lbuf.clone(), rbuf.clone()
    got = jc.as_lists(ops.join_sorted(lv, rv, how), how)
    assert got == jc.expected(CAPS, name, how)
    assert torch.equal(lbuf, l0) and torch.equal(rbuf, r0)


def test_case_generators_have_the_properties_the_gpu_tests_rely_on():
    seen_l, seen_r = set(), set()
    for name, (lk, rk) in CASES.items():
        assert lk == sorted(lk) and rk == sorted(rk), name
        if name.startswith("dup64_"):
            seen_l.add(len(lk))
            seen_r.add(len(rk))
    assert seen_l >= set(jc.sizes(T)) and seen_r >= set(jc.sizes(T))
    for how in ("inner", "left"):  # every case stays small
        for name in CASES:
            assert len(jc.expected(CAPS, name, how)[0]) < 2_000_000
    # no match at all / exactly 1:1
    assert jc.expected(CAPS, "disjoint", "inner") == ([], [])
    n = len(CASES["identical"][0])
    assert jc.expected(CAPS, "identical", "inner") == (list(range(n)),
                                                       list(range(n)))
    # all_equal: every left run (300 rows) crosses a tile boundary somewhere
    li, _ = jc.expected(CAPS, "all_equal", "inner")
    assert len(li) == 90_000 and len(li) > 2 * T
    # hot A: one left row whose run spans four tiles
    li, ri = jc.expected(CAPS, "hot_a", "inner")
    assert li == [1] * (3 * T + 5) and len({j // T for j in range(len(li))}) == 4
    # hot B: one tile reaches more distinct left rows than LDS stages
    for name in ("hot_b", "hot_b_gaps"):
        li, _ = jc.expected(CAPS, name, "inner")
        assert len(li) <= T and li[-1] - li[0] + 1 > S, name
    li, _ = jc.expected(CAPS, "hot_b", "inner")
    assert li == list(range(S + 7))
    li, _ = jc.expected(CAPS, "hot_b_gaps", "left")
    assert len(li) > 4 * T  # the same rows spread over many tiles
    # windowed bounds: one tile of left rows spanning exactly W right keys
    # and W + 1; several tiles of left rows
    for extra in (0, 1):
        lk, rk = CASES[f"window_{W + extra}"]
        assert len(lk) <= BT and len(rk) == W + extra
        assert lk[0] == rk[0] and lk[-1] == rk[-1]
    assert len(CASES["window_tiles"][0]) > 2 * BT
    # sign bit: the i64 view of the sorted u64 column is NOT ascending
    sk = jc.to_i64(CASES["sign"][0]).tolist()
    assert sk != sorted(sk)
    # unmatched rows first, last and in between
    assert jc.expected(CAPS, "unmatched", "anti") == [0, 3, 7]
    _, ri = jc.expected(CAPS, "unmatched", "left")
    assert ri[0] == -1 and ri[-1] == -1 and -1 in ri[1:-1]


def test_join_sorted_checks_and_limits():
    lk = jc.to_i64([1, 2, 2, 3])
    rk = jc.to_i64([2, 2, 3])
    with pytest.raises(ValueError, match="how"):
        ops.join_sorted(lk, rk, "outer")
    with pytest.raises(TypeError):
        ops.join_sorted(lk.to(torch.int32), rk)
    total = 5
    ops.join_sorted(lk, rk, "inner", max_rows=total)
    with pytest.raises(ops.JoinTooLarge) as e:
        ops.join_sorted(lk, rk, "inner", max_rows=total - 1)
    assert isinstance(e.value, ValueError)
    assert str(total) in str(e.value) and str(total - 1) in str(e.value)
    with pytest.raises(ops.JoinTooLarge):
        ops.join_sorted(lk, rk, "left", max_rows=5)  # 6 rows with the pad
    assert ops.join_caps() == (ops.JOIN_TILE, ops.JOIN_LDS_ROWS)
    assert ops.join_bounds_caps() == (ops.JOIN_BOUNDS_TILE,
                                      ops.JOIN_BOUNDS_WIN)


# ------------------------------------------------------------ single rank

@pytest.mark.parametrize("lf64,rf64", [(False, False), (True, True),
                                       (False, True)])
@pytest.mark.parametrize("how", jc.HOWS)
def test_join_job_single_rank(how, lf64, rf64):
    lk, lv = jc.make_relation(11, 700, 90, lf64)
    rk, rv = jc.make_relation(12, 500, 110, rf64)
    rk[:200] = lk[:200]  # shared keys beyond the pool's own overlap
    keep = [t.clone() for t in (lk, lv.view(torch.int64), rk,
                                rv.view(torch.int64))]
    res = JoinJob("cpu", how=how).run(lk, lv, rk, rv)
    exp = jc.job_oracle(lk, lv, rk, rv, how)
    assert jc.job_lists(res) == exp
    assert len(exp[0]) > 0
    assert res.lvals.dtype == lv.dtype
    if how in ("inner", "left"):
        assert res.rvals.dtype == rv.dtype
    else:
        assert res.rvals is None
    assert (res.matched is not None) == (how == "left")
    for t, k in zip((lk, lv.view(torch.int64), rk, rv.view(torch.int64)),
                    keep):
        assert torch.equal(t, k)


def test_join_job_empty_sides_and_limit():
    lk, lv = jc.make_relation(3, 40, 8, True)
    e = torch.empty(0, dtype=torch.int64)
    for how in jc.HOWS:
        res = JoinJob("cpu", how=how).run(lk, lv, e, e)
        assert jc.job_lists(res) == jc.job_oracle(lk, lv, e, e, how)
        res = JoinJob("cpu", how=how).run(e, e, lk, lv)
        assert res.keys.numel() == 0
    with pytest.raises(ops.JoinTooLarge):
        JoinJob("cpu", how="inner", max_rows=10).run(lk, lv, lk, lv)
    with pytest.raises(ValueError):
        JoinJob("cpu", how="outer")


# ------------------------------------------------------------- gloo world=2

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _rank_inputs(rank, starve):
    lk, lv = jc.make_relation(100 + rank, 600, 80, False)
    rk, rv = jc.make_relation(200 + rank, 450, 80, True)
    rk[:150] = lk[:150]
    if starve and rank == 1:  # this rank stages nothing on the right
        rk, rv = rk[:0], rv[:0]
    return lk, lv, rk, rv


def _ws2_worker(rank, world, port, how, starve):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.distributed.init_process_group("gloo", rank=rank, world_size=world)
    try:
        lk, lv, rk, rv = _rank_inputs(rank, starve)
        res = JoinJob("cpu", how=how).run(lk, lv, rk, rv)
        mine = jc.job_lists(res)
        # each shard holds only its own keys (mulhi partition)
        assert all((k * world) >> 64 == rank for k in mine[0])
        shards = [None] * world
        torch.distributed.all_gather_object(shards, mine)
        if rank == 0:
            # the oracle over the ranks' inputs concatenated in rank
            # order: within a key, rows keep (source rank, source order),
            # and rank-major shards are the global key order
            ins = [_rank_inputs(r, starve) for r in range(world)]
            cat = [torch.cat([i[c] for i in ins]) for c in range(4)]
            exp = jc.job_oracle(*cat, how)
            assert len(exp[0]) > 0
            for c in range(4):
                if exp[c] is None:
                    assert all(s[c] is None for s in shards)
                else:
                    assert [x for s in shards for x in s[c]] == exp[c], c
    finally:
        torch.distributed.destroy_process_group()


@pytest.mark.timeout(180)
@pytest.mark.parametrize("how,starve", [("inner", False), ("left", True),
                                        ("semi", False), ("anti", True)])
def test_join_job_gloo_ws2(how, starve):
    torch.multiprocessing.spawn(
        _ws2_worker, args=(2, _free_port(), how, starve), nprocs=2,
        join=True)


def _too_large_worker(rank, world, port, qdir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.distributed.init_process_group("gloo", rank=rank, world_size=world)
    try:
        # every row shares ONE key, so one rank owns the whole 600 x 450
        # output and the other owns nothing: only the owner is over
        lk, lv, rk, rv = _rank_inputs(rank, False)
        lk = torch.full_like(lk, 5)
        rk = torch.full_like(rk, 5)
        try:
            JoinJob("cpu", how="inner", max_rows=1000).run(lk, lv, rk, rv)
            raised = None
        except ops.JoinTooLarge as e:
            raised = (e.total, e.max_rows)
        torch.distributed.barrier()  # neither rank is stuck in a collective
        with open(os.path.join(qdir, f"r{rank}.txt"), "w") as fh:
            fh.write(repr(raised))
    finally:
        torch.distributed.destroy_process_group()


@pytest.mark.timeout(180)
def test_join_too_large_raises_on_both_ranks_gloo_ws2(tmp_path):
    torch.multiprocessing.spawn(
        _too_large_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2,
        join=True)
    want = repr((1200 * 900, 1000))
    assert (tmp_path / "r0.txt").read_text() == want
    assert (tmp_path / "r1.txt").read_text() == want


# ---------------------------------------------------------- Server routing

def _fresh_join_tables():
    import importlib

    import mapreduce_amd.examples.join_tables as jt
    from mapreduce_amd import job as jobmod
    importlib.reload(jt)
    jobmod._module_cache.clear()
    jobmod._inited.clear()
    return jt


ROLES = ("taskfn", "mapfn", "partitionfn", "reducefn", "finalfn")


@pytest.mark.parametrize("how", jc.HOWS)
def test_join_tables_gpu_tier_equals_host_tier(how, monkeypatch):
    from mapreduce_amd import run_local
    from mapreduce_amd.parallel.coord import LocalCoordinator
    from mapreduce_amd.server import Server

    args = {"how": how, "seed": 5, "nl": 300, "nr": 240, "nkeys": 90,
            "splits": 3, "parts": 4}
    monkeypatch.setenv("MR_GPU_TIER", "off")
    jt = _fresh_join_tables()
    srv = run_local({"fns": {r: jt for r in ROLES}, "verbose": False,
                     "init_args": args}, nworkers=2)
    assert srv.finished and "tier" not in srv.stats
    host = dict(jt.RESULTS)
    assert host

    # the brute-force answer, from the relations themselves
    left, right = jt.make_relations(5, 300, 240, 90)
    exp = {}
    for k, l in left:
        rs = [r for rk, r in right if rk == k]
        if how == "inner":
            rows = [(l, r) for r in rs]
        elif how == "left":
            rows = [(l, r) for r in rs] or [(l, None)]
        else:
            rows = [l] if bool(rs) == (how == "semi") else []
        if rows:
            exp.setdefault(k, []).extend(rows)
    exp = {k: sorted(v, key=jt._order) for k, v in exp.items()}
    assert host == exp

    monkeypatch.setenv("MR_GPU_TIER", "force")
    jt = _fresh_join_tables()
    srv2 = Server(coord=LocalCoordinator()).configure(
        {"fns": {r: jt for r in ROLES}, "verbose": False,
         "init_args": args})
    assert srv2._gpu_engine_kind() == "join"
    srv2.loop()
    assert srv2.finished and srv2.stats["tier"] == "gpu"
    assert srv2.stats["engine"] == "join"
    assert dict(jt.RESULTS) == host
    # finalfn saw the keys in global key order
    assert list(jt.RESULTS) == sorted(jt.RESULTS)
    doc, _ = srv2.coord.get_doc("task_gpu")
    assert doc is not None and doc["status"] == "FINISHED"


def _toy_fns(**over):
    fns = {
        "taskfn": lambda emit: emit(1, "x"),
        "mapfn": lambda k, v, emit: None,
        "mapfn_gpu_pairs": lambda k, v: ([1, 1, 2], [10, 20, 30]),
        "partitionfn": lambda k: 0,
        "reducefn": lambda k, vs, emit: emit(sum(vs)),
        "finalfn": lambda pairs: True,
    }
    fns.update(over)
    return {r: fns for r in ROLES + ("combinerfn",)}


def test_join_refuses_a_two_tuple_from_the_staging_hook(monkeypatch):
    from mapreduce_amd.parallel.coord import LocalCoordinator
    from mapreduce_amd.server import Server

    monkeypatch.setenv("MR_GPU_TIER", "force")
    srv = Server(coord=LocalCoordinator()).configure(
        {"fns": _toy_fns(reducefn_gpu="join"), "verbose": False})
    assert srv._gpu_engine_kind() == "join"
    with pytest.raises(ValueError, match=r"mapfn_gpu_pairs.*\(keys, vals, "
                                         r"side\)"):
        srv.loop()


def test_sum_reducer_still_routes_to_pairs(monkeypatch):
    from mapreduce_amd.parallel.coord import LocalCoordinator
    from mapreduce_amd.server import Server

    monkeypatch.setenv("MR_GPU_TIER", "force")
    srv = Server(coord=LocalCoordinator()).configure(
        {"fns": _toy_fns(reducefn_gpu="sum", associative_reducer=True,
                         commutative_reducer=True), "verbose": False})
    assert srv._gpu_engine_kind() == "pairs"
    for name in ("join", "join_left", "join_semi", "join_anti"):
        srv = Server(coord=LocalCoordinator()).configure(
            {"fns": _toy_fns(reducefn_gpu=name), "verbose": False})
        assert srv._gpu_engine_kind() == "join"
