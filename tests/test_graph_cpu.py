"""GraphJob, Graph.pagerank and Graph.components through the CPU tier, the
Server routing of examples/pagerank on both tiers, and the gloo world=2
process test of the vertex-replicated, edge-partitioned scheme."""

import math
import os
import socket

import pytest
import torch

import graph_common as gc
from mapreduce_amd.gpu.graph import GraphJob

SRC, DST = gc.multigraph(11, 300, 3000)
COMPONENTS = gc.component_cases()


# ------------------------------------------------------------------- build

def test_build_orders_edges_by_dst_then_src_and_counts_multiplicity():
    s = [5, -1, 5, 5, 7, -1, 9]
    d = [7, 7, 7, 5, 7, 5, -1]
    g = gc.build("cpu", s, d)
    assert g.nodes.tolist() == [5, 7, 9, -1]  # u64 order: -1 is the largest
    assert g.src.dtype == torch.int32 and g.offsets.dtype == torch.int64
    assert g.offsets.tolist() == [0, 2, 6, 6, 7]
    # in-edges of 5: from 5 (self-loop) and -1; of 7: 5 twice, 7, -1
    assert g.src.tolist() == [0, 3, 0, 0, 1, 3, 2]
    assert g.outdeg.tolist() == [3, 1, 1, 2]
    assert g.inv_out.tolist() == [1 / 3, 1.0, 1.0, 0.5]
    sym = gc.build("cpu", s, d, symmetric=True)
    assert sym.m == 14 and sym.outdeg.tolist() == [5, 5, 1, 3]
    assert sym.offsets.tolist() == [0, 5, 10, 11, 14]


def test_build_refusals_and_the_empty_graph():
    job = GraphJob("cpu")
    with pytest.raises(TypeError, match="must be int64"):
        job.run(torch.tensor([1.0]), torch.tensor([1]))
    with pytest.raises(ValueError, match="one destination per source"):
        job.run(torch.tensor([1, 2]), torch.tensor([1]))
    e = torch.empty(0, dtype=torch.int64)
    g = job.run(e, e, symmetric=True)
    assert g.n == 0 and g.m == 0 and g.offsets.tolist() == [0]
    pr = g.pagerank(iters=5)
    assert pr.ranks.numel() == 0 and pr.iterations == 0
    labels, rounds = g.components()
    assert labels.numel() == 0 and rounds == 0
    with pytest.raises(ValueError, match="symmetric=True"):
        gc.build("cpu", [1], [2]).components()


# ---------------------------------------------------------------- PageRank

def test_pagerank_matches_the_oracle_within_the_derived_bound():
    gc.check_pagerank("cpu", SRC, DST)


def test_pagerank_stops_at_the_oracles_iteration():
    gc.check_early_stop("cpu", SRC, DST)


def test_more_continues_bit_for_bit():
    gc.check_more("cpu", SRC, DST)


def test_pagerank_from_a_start_vector():
    g = gc.build("cpu", SRC, DST)
    first = g.pagerank(0.85, 6)
    again = g.pagerank(0.85, 4, start=first.ranks)
    whole = g.pagerank(0.85, 10)
    assert torch.equal(again.ranks, whole.ranks)
    with pytest.raises(ValueError, match="start must be float64"):
        g.pagerank(start=first.ranks[:-1])


# -------------------------------------------------------------- components

@pytest.mark.parametrize("name", sorted(COMPONENTS))
def test_components_match_union_find(name):
    gc.check_components("cpu", *COMPONENTS[name])


# ---------------------------------------------------------- Server routing

ROLES = ("taskfn", "mapfn", "partitionfn", "reducefn", "finalfn")


def _fresh_pagerank():
    import importlib

    import mapreduce_amd.examples.pagerank as pg
    from mapreduce_amd import job as jobmod
    importlib.reload(pg)
    jobmod._module_cache.clear()
    jobmod._inited.clear()
    return pg


def run_example_gpu_tier(monkeypatch, mode, args):
    from mapreduce_amd.parallel.coord import LocalCoordinator
    from mapreduce_amd.server import Server

    monkeypatch.setenv("MR_GPU_TIER", mode)
    pg = _fresh_pagerank()
    srv = Server(coord=LocalCoordinator()).configure(
        {"fns": {r: pg for r in ROLES}, "verbose": False,
         "init_args": args})
    assert srv._gpu_engine_kind() == "graph"
    srv.loop()
    assert srv.finished and srv.stats["tier"] == "gpu"
    assert srv.stats["engine"] == "graph:pagerank"
    return pg, srv


def check_example_result(pg, ranks, edges):
    """The one-step residual of a tier's result."""
    s, d = [e[0] for e in edges], [e[1] for e in edges]
    n = len(set(s) | set(d))
    assert sorted(ranks) == sorted(set(s) | set(d))
    res = gc.pagerank_residual(ranks, s, d, pg.DAMPING)
    assert res <= pg.DAMPING * pg.TOL + n * 2.0 ** -50, res
    # the example's own reference rule is the oracle's
    one = pg.step(ranks, edges)
    two, _, _ = gc.pagerank_oracle(s, d, pg.DAMPING, 1, 0.0, ranks)
    assert one == two
    return n


def test_pagerank_example_on_both_tiers(monkeypatch):
    from mapreduce_amd import run_local

    args = {"seed": 3, "n": 60, "m": 400, "splits": 3, "parts": 4}
    monkeypatch.setenv("MR_GPU_TIER", "off")
    pg = _fresh_pagerank()
    srv = run_local({"fns": {r: pg for r in ROLES}, "verbose": False,
                     "init_args": args}, nworkers=2)
    assert srv.finished and "tier" not in srv.stats
    host = dict(pg.RESULTS)
    edges = pg.make_edges(3, 60, 400)
    f = gc.graph_features([e[0] for e in edges], [e[1] for e in edges])
    assert f["dangling"] and f["source_only"] and f["parallel"]
    assert f["self_loops"]
    n = check_example_result(pg, host, edges)
    host_rounds = pg._STATE["rounds"]
    assert host_rounds > 10

    pg, srv2 = run_example_gpu_tier(monkeypatch, "force", args)
    dev = dict(pg.RESULTS)
    check_example_result(pg, dev, edges)
    # the same finalfn ends the device run in two rounds, the second of
    # one iteration
    assert pg._STATE["rounds"] == 2 and srv2.iteration == 2
    assert 2 < srv2.stats["graph_iterations"] <= host_rounds + 1
    # finalfn saw the nodes in key order
    assert list(pg.RESULTS) == sorted(pg.RESULTS)
    doc, _ = srv2.coord.get_doc("task_gpu")
    assert doc is not None and doc["status"] == "FINISHED"
    l1 = math.fsum(abs(host[v] - dev[v]) for v in host)
    d, tol = pg.DAMPING, pg.TOL
    assert l1 <= 2 * d * tol / (1 - d) + n * 2.0 ** -50, l1


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


def _server(monkeypatch, **over):
    from mapreduce_amd.parallel.coord import LocalCoordinator
    from mapreduce_amd.server import Server

    monkeypatch.setenv("MR_GPU_TIER", "force")
    return Server(coord=LocalCoordinator()).configure(
        {"fns": _toy_fns(**over), "verbose": False})


def test_components_task_given_as_a_dict_of_functions(monkeypatch):
    s, d = COMPONENTS["negative_keys"]
    seen = []
    srv = _server(
        monkeypatch, reducefn_gpu="components",
        taskfn=lambda emit: (emit(0, 0), emit(1, 1)),
        mapfn_gpu_pairs=lambda k, v: (s[v::2], d[v::2]),
        finalfn=lambda pairs: seen.extend(pairs) or True)
    assert srv._gpu_engine_kind() == "graph"
    srv.loop()
    assert srv.stats["tier"] == "gpu"
    assert srv.stats["engine"] == "graph:components"
    assert 0 < srv.stats["graph_iterations"] <= gc.rounds_bound(len(seen))
    exp = gc.component_oracle(s, d)
    assert {k: v for k, v in seen} == {k: [v] for k, v in exp.items()}
    assert [k for k, _ in seen] == sorted(exp, key=gc.u64_order)


def test_gpu_key_decode_and_the_loop_reply(monkeypatch):
    rounds = []

    def finalfn(pairs):
        rounds.append(dict(pairs))
        return "loop" if len(rounds) < 3 else True

    srv = _server(
        monkeypatch, reducefn_gpu="pagerank:d=0.5,iters=2",
        mapfn_gpu_pairs=lambda k, v: ([1, 2, 3, 3], [2, 3, 1, 2]),
        gpu_key_decode=lambda k: f"n{k}", finalfn=finalfn)
    srv.loop()
    assert srv.stats["graph_iterations"] == 6
    assert list(rounds[0]) == ["n1", "n2", "n3"]
    exp, _, _ = gc.pagerank_oracle([1, 2, 3, 3], [2, 3, 1, 2], 0.5, 6)
    for k, v in exp.items():
        assert rounds[2][f"n{k}"] == [pytest.approx(v, rel=1e-14)]
    # the resident state was continued, not restarted
    two, _, _ = gc.pagerank_oracle([1, 2, 3, 3], [2, 3, 1, 2], 0.5, 2)
    assert rounds[0]["n1"] == [pytest.approx(two[1], rel=1e-14)]
    assert rounds[2]["n1"] != rounds[0]["n1"]


def test_graph_engine_refuses_a_three_tuple_from_the_staging_hook(
        monkeypatch):
    srv = _server(monkeypatch, reducefn_gpu="pagerank",
                  mapfn_gpu_pairs=lambda k, v: ([1], [2], [3]))
    with pytest.raises(ValueError, match=r"mapfn_gpu_pairs.*\(src, dst\)"
                                         r".*3-tuple"):
        srv.loop()


def test_parse_graph_reducer():
    from mapreduce_amd.server import Server

    p = Server.parse_graph_reducer
    base = {"algo": "pagerank", "damping": 0.85, "iters": 100, "tol": 0.0}
    assert p("pagerank") == base
    assert p("components") == {"algo": "components"}
    assert p("pagerank:d=0.5") == dict(base, damping=0.5)
    assert p("pagerank:iters=7") == dict(base, iters=7)
    assert p("pagerank:tol=1e-9") == dict(base, tol=1e-9)
    assert p("pagerank:tol=1e-06,d=1,iters=1") == {
        "algo": "pagerank", "damping": 1.0, "iters": 1, "tol": 1e-6}
    assert p("pagerank:d=0,iters=3,tol=.5") == {
        "algo": "pagerank", "damping": 0.0, "iters": 3, "tol": 0.5}
    for bad in ("pagerank:", "components:", "components:x", "pagerank:d",
                "pagerank:d=", "pagerank:d=1.5", "pagerank:d=-0.1",
                "pagerank:d=nan", "pagerank:tol=inf", "pagerank:tol=-1",
                "pagerank:iters=0", "pagerank:iters=1.5", "pagerank:iters=",
                "pagerank:d=0.5,d=0.6", "pagerank:d=0.5,", "pagerank:x=1",
                "pagerank: d=0.5", "pagerank:tol=1e400", "pagerank:iters=+3",
                "pagerank:D=0.5"):
        with pytest.raises(ValueError) as e:
            p(bad)
        assert repr(bad) in str(e.value)
    for other in ("pagerank2", "page", "component", "sum", "join",
                  "cumsum", "median", "sort", "join_asof", None, 5):
        assert p(other) is None
    assert Server.parse_group_reducer("pagerank:d=0.5") is None
    assert Server.parse_window_reducer("components") is None
    assert Server.parse_asof_reducer("pagerank") is None


def test_malformed_graph_reducer_is_refused_at_configure(monkeypatch):
    with pytest.raises(ValueError, match="pagerank:d=2"):
        _server(monkeypatch, reducefn_gpu="pagerank:d=2")


def test_every_reducer_of_the_nine_families_keeps_its_kind(monkeypatch):
    three = lambda k, v: ([1, 1, 2], [10, 20, 30], [1, 2, 3])  # noqa: E731
    for name, kind in (
            ("sort", "sort"), ("join", "join"), ("join_left", "join"),
            ("join_semi", "join"), ("join_anti", "join"),
            ("group", "group"), ("median", "group"),
            ("quantile:1/2,9/10", "group"), ("topk:3", "group"),
            ("bottomk:2", "group"), ("distinct", "group"),
            ("cumsum", "window"), ("cummin", "window"),
            ("cummax", "window"), ("sessions:5", "window"),
            ("rolling:sum:60", "window"),
            ("rolling:max:3,fol=1,rows", "window"),
            ("join_asof", "asof"), ("join_asof:forward,tol=3", "asof"),
            ("pagerank", "graph"), ("pagerank:d=0.9,iters=5", "graph"),
            ("components", "graph")):
        srv = _server(monkeypatch, reducefn_gpu=name, mapfn_gpu_pairs=three)
        assert srv._gpu_engine_kind() == kind, name
    flags = dict(associative_reducer=True, commutative_reducer=True,
                 idempotent_reducer=True)
    for name in ("sum", "min", "max", "minmax"):
        srv = _server(monkeypatch, reducefn_gpu=name, **flags)
        assert srv._gpu_engine_kind() == "pairs", name
    # a pair reducer without its flags still routes nowhere
    assert _server(monkeypatch, reducefn_gpu="sum")._gpu_engine_kind() is None
    mg = lambda k, v: b""  # noqa: E731
    srv = _server(monkeypatch, reducefn_gpu="sum", mapfn_gpu=mg,
                  mapfn_gpu_pairs=None, **flags)
    assert srv._gpu_engine_kind() == "bytes"
    srv = _server(monkeypatch, reducefn_gpu="index", mapfn_gpu=mg,
                  mapfn_gpu_pairs=None)
    assert srv._gpu_engine_kind() == "index"
    srv = _server(monkeypatch, reducefn_gpu="gradsum", mapfn_gpu_pairs=None,
                  mapfn_gpu_grads=lambda k, v: {}, **flags)
    assert srv._gpu_engine_kind() == "gradsum"


# ------------------------------------------------ gloo world=2 process test

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _rank_edges(rank):
    """Rank 0 stages two thirds of the PageRank edges and rank 1 the rest;
    the component edges split by parity."""
    cut = 2 * len(SRC) // 3
    pr = (SRC[:cut], DST[:cut]) if rank == 0 else (SRC[cut:], DST[cut:])
    s, d = COMPONENTS["negative_keys"]
    return pr, (s[rank::2], d[rank::2])


def _ws2_worker(rank, world, port):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.distributed.init_process_group("gloo", rank=rank, world_size=world)
    try:
        (ps, pd), (cs, cd) = _rank_edges(rank)
        t = lambda x: torch.tensor(x, dtype=torch.int64)  # noqa: E731
        g = GraphJob("cpu").run(t(ps), t(pd))
        assert g.world == world and g.m == len(ps)
        pr = g.pagerank(0.85, 20)
        a, b = g.owned()
        mine = list(zip(g.nodes[a:b].tolist(), pr.ranks[a:b].tolist()))
        # early stop: rank 0 decides, both ranks stop together
        _, _, deltas = gc.pagerank_oracle(SRC, DST, gc.EARLY_DAMPING, 8)
        early = g.pagerank(gc.EARLY_DAMPING, 8, gc.early_stop_tol(deltas))
        c = GraphJob("cpu").run(t(cs), t(cd), symmetric=True)
        labels, rounds = c.components()
        a, b = c.owned()
        lab = list(zip(c.nodes[a:b].tolist(), labels[a:b].tolist()))
        shards = [None] * world
        torch.distributed.all_gather_object(
            shards, (mine, lab, rounds, early.iterations))
        if rank == 0:
            assert all(s[0] and s[1] for s in shards)
            got = [r for s in shards for r in s[0]]
            exp, _, _ = gc.pagerank_oracle(SRC, DST, 0.85, 20)
            # rank-major slices are the global key order
            assert [k for k, _ in got] == sorted(exp, key=gc.u64_order)
            bound = gc.pagerank_bound(SRC, DST, 20)
            assert all(abs(v - exp[k]) <= bound * exp[k] for k, v in got)
            assert [s[3] for s in shards] == [3, 3]
            # world=1 over the concatenated inputs gives the union-find
            # labels (test_components_match_union_find): so does world=2
            s, d = COMPONENTS["negative_keys"]
            got = [r for s_ in shards for r in s_[1]]
            uf = gc.component_oracle(s, d)
            assert [k for k, _ in got] == sorted(uf, key=gc.u64_order)
            assert dict(got) == uf
            assert shards[0][2] == shards[1][2] <= gc.rounds_bound(len(uf))
    finally:
        torch.distributed.destroy_process_group()


@pytest.mark.timeout(180)
def test_graph_job_gloo_ws2():
    torch.multiprocessing.spawn(
        _ws2_worker, args=(2, _free_port()), nprocs=2, join=True)
