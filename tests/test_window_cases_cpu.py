"""The window family without a GPU: the layout generators, every op on the CPU
tier, return_perm, WindowJob single rank and under gloo world=2, and the
Server routing of examples/sessions.  Every comparison is exact against the
pure-Python oracle of window_common."""

import os
import socket

import numpy as np
import pytest
import torch

import group_common as gc
import window_common as wc
from mapreduce_amd import ops
from mapreduce_amd.gpu.window import WindowJob

S, C = ops.seg_scan_caps()
LAYOUTS = wc.layouts(S)
GT, GR = ops.group_caps()[0], ops.group_rank_max()
GCASES = gc.cases((GT, GR))


# ------------------------------------------------------------ the generators

def test_layouts_have_the_properties_the_gpu_tests_rely_on():
    assert (S, C) == (ops.SEG_SCAN_TILE, ops.SEG_CARRY_CHUNK)
    assert S % 2 == 0 and S > 65 and C >= 2
    sizes = wc.SIZES(S)
    assert sizes == (0, 1, 2, 63, 64, 65, S - 1, S, S + 1, 3 * S + 17)
    for n in sizes[1:]:
        assert sum(LAYOUTS[f"singles_{n}"]) == n
        assert set(LAYOUTS[f"singles_{n}"]) == {1}
        assert LAYOUTS[f"one_{n}"] == (n,)
        assert sum(LAYOUTS[f"pairs_{n}"]) == n
        assert set(LAYOUTS[f"pairs_{n}"][:-1]) <= {2}
    assert sum(LAYOUTS["n0"]) == 0
    # one segment over everything: only tile 0 holds a head
    n = 3 * S + 17
    assert wc.headless_tiles(LAYOUTS[f"one_{n}"], S) == [1, 2, 3]
    assert wc.headless_tiles(LAYOUTS[f"singles_{n}"], S) == []
    # a pair lies across no tile boundary (S is even) ...
    assert all(h % 2 == 0 for h in wc.heads_of(LAYOUTS[f"pairs_{n}"]))
    # ... the heads exactly at S and at S - 1
    assert wc.heads_of(LAYOUTS["head_at_S"]) == [0, S]
    assert wc.heads_of(LAYOUTS["head_at_S_minus_1"]) == [0, S - 1]
    # a segment from S/2 to 2S + S/2: its middle tile has no head
    off = wc.offsets_of(LAYOUTS["middle_tile_headless"])
    assert off == [0, S // 2, 2 * S + S // 2, 3 * S]
    assert wc.headless_tiles(LAYOUTS["middle_tile_headless"], S) == [1]
    r = LAYOUTS["random"]
    assert min(r) >= 1 and max(r) <= 3 * S and max(r) > S
    assert wc.headless_tiles(r, S)
    # the second chunk of the carry pass
    big = wc.second_chunk_layout(S, C)
    assert sum(big) == (C + 1) * S and len(big) == 3 and min(big) > 2 * S
    boff = wc.offsets_of(big)
    assert boff[2] < C * S < boff[3]   # a segment crosses tile C
    assert sum(big) <= 1 << 22         # the f64_int exactness argument
    for name, lens in LAYOUTS.items():
        assert sum(lens) < 50_000, name
        keys = wc.layout_keys(lens)
        kb = gc.to_bits(keys)
        heads = [i for i in range(len(kb)) if i == 0 or kb[i] != kb[i - 1]]
        assert heads == wc.heads_of(lens), name
    # keys are grouped, not sorted
    kb = gc.to_bits(wc.layout_keys(LAYOUTS["random"]))
    assert kb != sorted(kb)
    # the families
    v = wc.values("f64_int", 500)
    assert all(float(x).is_integer() and abs(x) <= 2 ** 20
               for x in v.tolist())
    bits = set(gc.to_bits(wc.values("f64_special", 400)))
    assert {0, gc.SIGN} <= bits and set(gc.NAN_BITS) <= bits
    iv = wc.values("i64_full", 50).tolist()
    assert gc.I64_MIN in iv and gc.I64_MAX in iv


def test_oracle_on_hand_cases():
    v = torch.tensor([1, 2, 3, gc.I64_MAX, 1, -5], dtype=torch.int64)
    assert wc.oracle_scan((3, 2, 1), v, "sum") == [
        1, 3, 6, gc.I64_MAX, 1 << 63, (-5) & wc.M64]
    assert wc.oracle_scan((3, 2, 1), v, "min") == [
        1, 1, 1, gc.I64_MAX, 1, (-5) & wc.M64]
    z = torch.tensor([0.0, -0.0, float("nan"), 1.0, -0.0, 0.0],
                     dtype=torch.float64)
    fb = gc.f64_bits
    # equal order keys keep the earlier row's bits; NaN is the largest
    assert wc.oracle_scan((4, 2), z, "min") == [
        fb(0.0), fb(0.0), fb(0.0), fb(0.0), fb(-0.0), fb(-0.0)]
    got = wc.oracle_scan((4, 2), z, "max")
    assert got[:2] == [fb(0.0), fb(0.0)] and got[2] == got[3] == gc.to_bits(
        z)[2]


# -------------------------------------------------------------------- the ops

@pytest.mark.parametrize("name", sorted(LAYOUTS))
def test_scan_cpu_matches_oracle(name):
    lens = LAYOUTS[name]
    for family, fam_ops in wc.FAMILIES.items():
        keys, vals = wc.layout_data(S, name, family)
        kbuf, vbuf, kv, vv = gc.baited(keys, vals)
        k0, v0 = kbuf.clone(), vbuf.view(torch.int64).clone()
        for op in fam_ops:
            out = ops.scan_by_key_sorted(kv, vv, op)
            assert out.dtype == vals.dtype and out.numel() == vals.numel()
            assert gc.to_bits(out) == wc.expected_scan(S, name, family,
                                                       op), (family, op)
            assert not lens or out.data_ptr() != vv.data_ptr()
        assert torch.equal(kbuf, k0)
        assert torch.equal(vbuf.view(torch.int64), v0)


def test_scan_refusals_cpu():
    k = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(ValueError, match="op must be"):
        ops.scan_by_key_sorted(k, k, "prod")
    with pytest.raises(TypeError, match="int64 or float64"):
        ops.scan_by_key_sorted(k, k.to(torch.float32))
    with pytest.raises(TypeError, match="keys must be int64"):
        ops.scan_by_key_sorted(k.to(torch.int32), k)
    with pytest.raises(ValueError, match="one value per key"):
        ops.scan_by_key_sorted(k, k[:-1])
    e = ops.scan_by_key_sorted(k[:0], k[:0].view(torch.float64), "max")
    assert e.numel() == 0 and e.dtype == torch.float64


@pytest.mark.parametrize("family", ["random_i64", "two_valued", "f64"])
@pytest.mark.parametrize("name", sorted(GCASES))
def test_return_perm_cpu(name, family):
    keys, vals, off = gc.case_data((GT, GR), name, family)
    _, exp_bits = gc.expected((GT, GR), name, family)
    plain = ops.sort_values_in_groups(keys, vals)
    assert isinstance(plain, torch.Tensor)
    out, perm = ops.sort_values_in_groups(keys, vals, return_perm=True)
    assert perm.dtype == torch.int64 and perm.numel() == vals.numel()
    assert gc.to_bits(out) == exp_bits == gc.to_bits(plain)
    assert gc.to_bits(vals[perm]) == exp_bits
    assert perm.tolist() == wc.oracle_perm(off, vals)
    # a stable np.lexsort on (key, order key) is the same order
    ok = np.array(gc.okeys(vals), dtype=np.uint64)
    ku = keys.numpy().view(np.uint64)
    assert perm.tolist() == np.lexsort((ok, ku)).tolist()


SESSION_CASES = {
    # (keys, times, gap) -> flags
    "gap_exact_and_plus_one": ([7, 7, 7, 7], [0, 10, 21, 31], 10,
                               [1, 0, 1, 0]),
    "full_span": ([1, 1], [gc.I64_MIN, gc.I64_MAX], gc.I64_MAX, [1, 1]),
    "full_span_one_less": ([1, 1], [gc.I64_MIN + 1, gc.I64_MAX - 1],
                           gc.I64_MAX, [1, 1]),
    "half_span": ([1, 1, 1], [gc.I64_MIN, -1, gc.I64_MAX - 1], gc.I64_MAX,
                  [1, 0, 0]),
    "gap_zero_duplicates": ([3, 3, 3, 3], [5, 5, 6, 6], 0, [1, 0, 1, 0]),
    "key_change_equal_times": ([3, 3, 4, 4], [9, 9, 9, 9], 100,
                               [1, 0, 1, 0]),
    "negative_times": ([2, 2, 2], [-50, -40, -29], 10, [1, 0, 1]),
}


@pytest.mark.parametrize("name", sorted(SESSION_CASES))
def test_session_flags_cpu(name):
    keys, times, gap, flags = SESSION_CASES[name]
    assert wc.oracle_session_flags(keys, times, gap) == flags
    k = torch.tensor(keys, dtype=torch.int64)
    t = torch.tensor(times, dtype=torch.int64)
    assert ops.session_flags(k, t, gap).tolist() == flags
    sk, so = ops.group_sessions(k, t, gap)
    ek, eo = wc.oracle_sessions(keys, times, gap)
    assert sk.tolist() == ek and so.tolist() == eo


def test_session_refusals_cpu():
    k = torch.zeros(3, dtype=torch.int64)
    with pytest.raises(TypeError, match="int64"):
        ops.session_flags(k, k.to(torch.float64), 5)
    with pytest.raises(ValueError, match="gap"):
        ops.session_flags(k, k, -1)
    with pytest.raises(ValueError, match="gap"):
        ops.session_flags(k, k, 2 ** 63)
    with pytest.raises(TypeError, match="gap"):
        ops.session_flags(k, k, 1.5)
    with pytest.raises(ValueError, match="one time per key"):
        ops.session_flags(k, k[:-1], 1)
    sk, so = ops.group_sessions(k[:0], k[:0], 3)
    assert sk.numel() == 0 and so.tolist() == [0]


# ------------------------------------------------------------ single rank

def check_result(res, keys, order, vals, world=1, rank=0):
    """The job's partition against the oracle, with its scans and
    sessions; -> the lists compared."""
    exp = wc.job_oracle(keys, order, vals, world, rank)
    got = wc.job_lists(res)
    assert got == exp
    uk, off, _, _ = exp
    lens = tuple(b - a for a, b in zip(off, off[1:]))
    assert res.counts().tolist() == list(lens)
    if vals is not None:
        assert res.values.dtype == vals.dtype
        f64 = vals.dtype == torch.float64
        for op in (("min", "max") if f64 else wc.OPS):
            run = res.scan(op)
            want = wc.oracle_scan(lens, res.values.cpu(), op)
            # rows that tie are interchangeable up to a zero's sign and a
            # NaN's payload: floats compare by order key
            assert gc.okeys(run) == [gc.okey(b, f64) for b in want], op
            if not f64:
                assert gc.to_bits(run) == want
    if order.dtype == torch.int64:
        times = res.order.cpu().tolist()
        gap = 3000
        rows, per_key = wc.oracle_job_sessions(got, times, gap)
        ses = res.sessions(gap)
        assert list(zip(gc.to_bits(ses.keys), ses.start.tolist(),
                        ses.end.tolist(), ses.count.tolist())) == rows
        assert ses.per_key.tolist() == per_key
        assert sum(per_key) > len(uk) or not uk
        host = ses.to_host()
        assert [len(r) for _, r in host] == per_key
        if vals is not None and vals.dtype == torch.int64:
            slens = tuple(r[3] for r in rows)
            assert sum(slens) == len(times)
            assert gc.to_bits(res.scan("sum", within_sessions=gap)) == \
                wc.oracle_scan(slens, res.values.cpu(), "sum")
    return got


@pytest.mark.parametrize("order_f64,vals_f64", [(False, False), (False, True),
                                                (True, False), (False, None)])
def test_window_job_single_rank(order_f64, vals_f64):
    keys, order, vals = wc.make_rows(23, 900, 60, order_f64, bool(vals_f64),
                                     hot=150)
    if vals_f64 is None:
        vals = None
    keep = [t.clone() for t in (keys, order.view(torch.int64))]
    res = WindowJob("cpu").run(keys, order, vals)
    got = check_result(res, keys, order, vals)
    assert len(got[0]) > 50
    assert res.order.dtype == order.dtype
    assert torch.equal(keys, keep[0])
    assert torch.equal(order.view(torch.int64), keep[1])
    host = res.to_host()
    assert [k & gc.M64 for k, _ in host] == got[0]
    if vals is None:
        assert res.values is None
        with pytest.raises(ValueError, match="value column"):
            res.scan("sum")
    else:
        assert all(isinstance(r, tuple) for _, rows in host for r in rows)
    # the order of the input rows does not matter
    p = torch.randperm(keys.numel(), generator=torch.Generator().manual_seed(1))
    res2 = WindowJob("cpu").run(keys[p], order[p],
                                None if vals is None else vals[p])
    assert wc.job_lists(res2) == got


def test_window_job_empty_and_refusals():
    e = torch.empty(0, dtype=torch.int64)
    res = WindowJob("cpu").run(e, e, e.view(torch.float64))
    assert res.keys.numel() == 0 and res.offsets.tolist() == [0]
    assert res.values.dtype == torch.float64
    assert res.scan("max").numel() == 0 and res.to_host() == []
    ses = res.sessions(5)
    assert ses.keys.numel() == 0 and ses.to_host() == []
    z = torch.zeros(3, dtype=torch.int64)
    with pytest.raises(TypeError, match="int64 or float64"):
        WindowJob("cpu").run(z, z.to(torch.float32))
    with pytest.raises(TypeError, match="int64 or float64"):
        WindowJob("cpu").run(z, z, z.to(torch.int32))
    with pytest.raises(ValueError, match="per key"):
        WindowJob("cpu").run(z, z[:-1])
    with pytest.raises(TypeError, match="int64"):
        WindowJob("cpu").run(z, z.to(torch.float64)).sessions(3)


# ------------------------------------------------------------- gloo world=2

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _rank_inputs(rank, starve):
    # the starved variant carries f64 values, the other i64
    keys, order, vals = wc.make_rows(400 + rank, 700, 50, False, starve,
                                     hot=90)
    if starve and rank == 1:  # this rank stages nothing
        keys, order, vals = keys[:0], order[:0], vals[:0]
    return keys, order, vals


def _ws2_worker(rank, world, port, starve):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.distributed.init_process_group("gloo", rank=rank, world_size=world)
    try:
        keys, order, vals = _rank_inputs(rank, starve)
        ins = [_rank_inputs(r, starve) for r in range(world)]
        allk, allo, allv = (torch.cat([i[c] for i in ins]) for c in range(3))
        for with_vals in (True, False):
            res = WindowJob("cpu").run(keys, order,
                                       vals if with_vals else None)
            # this rank's shard is its partition of all the rows, with its
            # scans and sessions
            mine = check_result(res, allk, allo,
                                allv if with_vals else None, world, rank)
            assert all((k * world) >> 64 == rank for k in mine[0])
            shards = [None] * world
            torch.distributed.all_gather_object(shards, mine)
            if rank == 0:
                # rank-major shards are the single-rank result over the
                # ranks' inputs together: independent of the world size
                uk, off, oo, vv = wc.job_oracle(
                    allk, allo, allv if with_vals else None)
                assert len(uk) > 40
                assert [x for s in shards for x in s[0]] == uk
                assert [x for s in shards for x in s[2]] == oo
                if with_vals:
                    assert [x for s in shards for x in s[3]] == vv
                lens = [b - a for s in shards
                        for a, b in zip(s[1], s[1][1:])]
                assert lens == [b - a for a, b in zip(off, off[1:])]
    finally:
        torch.distributed.destroy_process_group()


@pytest.mark.timeout(180)
@pytest.mark.parametrize("starve", [False, True])
def test_window_job_gloo_ws2(starve):
    torch.multiprocessing.spawn(
        _ws2_worker, args=(2, _free_port(), starve), nprocs=2, join=True)


# ---------------------------------------------------------- Server routing

ROLES = ("taskfn", "mapfn", "partitionfn", "reducefn", "finalfn")


def _fresh_sessions():
    import importlib

    import mapreduce_amd.examples.sessions as se
    from mapreduce_amd import job as jobmod
    importlib.reload(se)
    jobmod._module_cache.clear()
    jobmod._inited.clear()
    return se


def test_sessions_gpu_tier_equals_host_tier(monkeypatch):
    from mapreduce_amd import run_local
    from mapreduce_amd.parallel.coord import LocalCoordinator
    from mapreduce_amd.server import Server

    args = {"seed": 4, "n": 1500, "nusers": 20, "splits": 3, "parts": 4}
    monkeypatch.setenv("MR_GPU_TIER", "off")
    se = _fresh_sessions()
    srv = run_local({"fns": {r: se for r in ROLES}, "verbose": False,
                     "init_args": args}, nworkers=2)
    assert srv.finished and "tier" not in srv.stats
    host = dict(se.RESULTS)

    # the answer from the rows themselves
    groups = {}
    for u, ts in se.make_rows(4, 1500, 20):
        groups.setdefault(u, []).append(ts)
    exp = {}
    for u, ts in groups.items():
        ts.sort()
        rows = []
        for i, t in enumerate(ts):
            if i == 0 or t - ts[i - 1] > se.GAP:
                rows.append([t, t, 0])
            rows[-1][1] = t
            rows[-1][2] += 1
        exp[u] = [tuple(r) for r in rows]
    assert host == exp and len(exp) > 5
    gaps = {b - a for ts in groups.values() for a, b in zip(ts, ts[1:])}
    assert {se.GAP, se.GAP + 1} <= gaps
    assert max(len(r) for r in exp.values()) > 3

    monkeypatch.setenv("MR_GPU_TIER", "force")
    se = _fresh_sessions()
    srv2 = Server(coord=LocalCoordinator()).configure(
        {"fns": {r: se for r in ROLES}, "verbose": False,
         "init_args": args})
    assert srv2._gpu_engine_kind() == "window"
    srv2.loop()
    assert srv2.finished and srv2.stats["tier"] == "gpu"
    assert srv2.stats["engine"] == "window:sessions"
    assert dict(se.RESULTS) == host
    assert list(se.RESULTS) == sorted(se.RESULTS)
    doc, _ = srv2.coord.get_doc("task_gpu")
    assert doc is not None and doc["status"] == "FINISHED"


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
    ("cumsum", 3, [(1, [(10, 7), (10, 14)]),
                   (2, [(10, -3), (20, 6), (30, 10), (30, 15)]),
                   (3, [(0, 0)])]),
    ("cummin", 3, [(1, [(10, 7), (10, 7)]),
                   (2, [(10, -3), (20, -3), (30, -3), (30, -3)]),
                   (3, [(0, 0)])]),
    ("cummax", 3, [(1, [(10, 7), (10, 7)]),
                   (2, [(10, -3), (20, 9), (30, 9), (30, 9)]),
                   (3, [(0, 0)])]),
    ("sessions:10", 2, [(1, [(10, 10, 2)]), (2, [(10, 30, 4)]),
                        (3, [(0, 0, 1)])]),
    ("sessions:9", 2, [(1, [(10, 10, 2)]),
                       (2, [(10, 10, 1), (20, 20, 1), (30, 30, 2)]),
                       (3, [(0, 0, 1)])]),
    ("sessions:0", 2, [(1, [(10, 10, 2)]),
                       (2, [(10, 10, 1), (20, 20, 1), (30, 30, 2)]),
                       (3, [(0, 0, 1)])]),
])
def test_window_reducers_hand_finalfn_the_documented_pairs(name, cols, exp,
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
    assert srv.stats["engine"] == "window:" + name.split(":")[0]


def test_float_columns_stage_as_f64(monkeypatch):
    from mapreduce_amd.parallel.coord import LocalCoordinator
    from mapreduce_amd.server import Server

    monkeypatch.setenv("MR_GPU_TIER", "force")
    seen = []
    rows = lambda k, v: ([1, 1, 1], [0.1, 0.3, 0.2], [1.5, 2 ** -40, -4.0])
    srv = Server(coord=LocalCoordinator()).configure(
        {"fns": _toy_fns(seen, reducefn_gpu="cumsum", mapfn_gpu_pairs=rows),
         "verbose": False})
    srv.loop()
    assert seen == [(1, [(0.1, 1.5), (0.2, -2.5), (0.3, -2.5 + 2 ** -40)])]


@pytest.mark.parametrize("name", [
    "sessions", "sessions:-1", "sessions:1.5", "sessions:9223372036854775808",
    "cumsum:3", "sessions:", "sessions:x", "cummin:", "cummax:1"])
def test_malformed_window_reducers_are_refused(name, monkeypatch):
    from mapreduce_amd.parallel.coord import LocalCoordinator
    from mapreduce_amd.server import Server

    monkeypatch.setenv("MR_GPU_TIER", "force")
    with pytest.raises(ValueError) as e:
        Server(coord=LocalCoordinator()).configure(
            {"fns": _toy_fns([], reducefn_gpu=name), "verbose": False})
    assert repr(name) in str(e.value)
    assert Server.parse_window_reducer("sessions:9223372036854775807") == (
        "sessions", 2 ** 63 - 1)


@pytest.mark.parametrize("name,cols", [("cumsum", 2), ("sessions:5", 3)])
def test_wrong_arity_names_the_reducer(name, cols, monkeypatch):
    from mapreduce_amd.parallel.coord import LocalCoordinator
    from mapreduce_amd.server import Server

    monkeypatch.setenv("MR_GPU_TIER", "force")
    srv = Server(coord=LocalCoordinator()).configure(
        {"fns": _toy_fns([], cols, reducefn_gpu=name), "verbose": False})
    with pytest.raises(ValueError) as e:
        srv.loop()
    assert repr(name) in str(e.value) and "mapfn_gpu_pairs" in str(e.value)


def test_other_families_still_route_beside_window(monkeypatch):
    from mapreduce_amd.parallel.coord import LocalCoordinator
    from mapreduce_amd.server import Server

    monkeypatch.setenv("MR_GPU_TIER", "force")
    srv = Server(coord=LocalCoordinator()).configure(
        {"fns": _toy_fns([], 2, reducefn_gpu="sum", associative_reducer=True,
                         commutative_reducer=True), "verbose": False})
    assert srv._gpu_engine_kind() == "pairs"
    srv = Server(coord=LocalCoordinator()).configure(
        {"fns": _toy_fns([], 2, reducefn_gpu="median"), "verbose": False})
    assert srv._gpu_engine_kind() == "group"
    for name in ("cumsum", "cummin", "cummax", "sessions:1800"):
        assert Server.parse_group_reducer(name) is None
        srv = Server(coord=LocalCoordinator()).configure(
            {"fns": _toy_fns([], reducefn_gpu=name), "verbose": False})
        assert srv._gpu_engine_kind() == "window"
    for name in ("sum", "min", "max", "minmax", "median", "join", "sort"):
        assert Server.parse_window_reducer(name) is None
    # without the staging hook the name decides nothing
    fns = _toy_fns([], reducefn_gpu="cumsum")
    for r in fns.values():
        r.pop("mapfn_gpu_pairs", None)
    srv = Server(coord=LocalCoordinator()).configure(
        {"fns": fns, "verbose": False})
    assert srv._gpu_engine_kind() is None
