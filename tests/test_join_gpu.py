"""The join kernels, the op, JoinJob and the Server routing on the device.
Every comparison is exact: against the brute-force oracle of join_common
and against the CPU tier.  Sizes come from the extension (ops.join_caps):
T output rows per tile, S offsets staged in LDS."""

import os

import pytest
import torch

import join_common as jc
from mapreduce_amd import ops
from mapreduce_amd.ops import _cpu

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


PY_CAPS = (ops.JOIN_TILE, ops.JOIN_LDS_ROWS, ops.JOIN_BOUNDS_TILE,
           ops.JOIN_BOUNDS_WIN)


@pytest.fixture(scope="module")
def caps():
    return ops.join_caps() + ops.join_bounds_caps()


def test_caps_come_from_the_extension(caps):
    assert caps == (tuple(ops.ext().join_caps())
                    + tuple(ops.ext().join_bounds_caps()))
    T, S, _, _ = caps
    assert S + 7 <= T  # hot key B fits one tile yet overflows the LDS slice


# parametrised by name over the Python constants; the test checks they are
# the extension's, so the ids name the cases the device actually runs
@pytest.mark.parametrize("bounds", ["window", "row"])
@pytest.mark.parametrize("name", sorted(jc.cases(*PY_CAPS)))
def test_join_sorted_matches_oracle_and_cpu_tier(name, bounds, caps,
                                                 monkeypatch):
    assert caps == PY_CAPS
    if bounds == "row":  # read per call: the thread-per-row bounds kernel
        monkeypatch.setenv("MR_JOIN_BOUNDS_ROW", "1")
    lk, rk = jc.cases(*caps)[name]
    lbuf, rbuf, lv, rv = jc.baited(lk, rk, DEV)
    l0, r0 = lbuf.clone(), rbuf.clone()
    lc, rc = jc.to_i64(lk), jc.to_i64(rk)
    for how in jc.HOWS:
        got = jc.as_lists(ops.join_sorted(lv, rv, how), how)
        assert got == jc.expected(caps, name, how), how
        assert got == jc.as_lists(_cpu.join_sorted(lc, rc, how), how), how
        assert torch.equal(lbuf, l0) and torch.equal(rbuf, r0), how


def test_host_checks():
    lk = jc.to_i64([1, 2, 2, 3]).to(DEV)
    rk = jc.to_i64([2, 2, 3]).to(DEV)
    with pytest.raises(RuntimeError, match="int64"):
        ops.join_sorted(lk.to(torch.int32), rk)
    with pytest.raises(RuntimeError, match="int64"):
        ops.join_sorted(lk, rk.to(torch.int32))
    with pytest.raises(RuntimeError, match="GPU"):
        ops.join_sorted(lk, rk.cpu())
    with pytest.raises(RuntimeError, match="GPU"):
        ops.join_sorted(lk.cpu(), rk)
    with pytest.raises(ValueError, match="how"):
        ops.join_sorted(lk, rk, "outer")
    with pytest.raises(RuntimeError, match="contiguous"):
        ops.ext().join_bounds(torch.stack([lk, lk], 1)[:, 0], rk)
    with pytest.raises(RuntimeError, match="total"):
        ops.ext().join_expand(lk[:1], lk[:0], lk[:0], 3)


@pytest.mark.parametrize("how,total", [("inner", 5), ("left", 6)])
def test_max_rows(how, total):
    lk = jc.to_i64([1, 2, 2, 3]).to(DEV)
    rk = jc.to_i64([2, 2, 3]).to(DEV)
    li, _ = ops.join_sorted(lk, rk, how, max_rows=total)
    assert li.numel() == total
    with pytest.raises(ops.JoinTooLarge) as e:
        ops.join_sorted(lk, rk, how, max_rows=total - 1)
    assert e.value.total == total and e.value.max_rows == total - 1


# ------------------------------------------------------------------ JoinJob

@pytest.fixture(scope="module")
def relations():
    """(lk, lv, rk, rv) per value dtype, 5 000 x 3 000 rows, on the host;
    oracle rows are computed once per (dtype, how) and shared."""
    rel = {}
    for f64 in (False, True):
        lk, lv = jc.make_relation(31, 5000, 700, f64)
        rk, rv = jc.make_relation(32, 3000, 700, f64)
        rk[:1000] = lk[:1000]
        rel[f64] = (lk, lv, rk, rv)
    return rel


@pytest.fixture(scope="module")
def job_expected(relations):
    return {(f64, how): jc.job_oracle(*relations[f64], how)
            for f64 in relations for how in jc.HOWS}


@pytest.mark.parametrize("small_sort", [None, "1"])
@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("how", jc.HOWS)
def test_join_job_on_device(how, f64, small_sort, relations, job_expected,
                            monkeypatch):
    from mapreduce_amd.gpu.join import JoinJob

    if small_sort is not None:
        # read per call: the in-tree radix sort and the idx32 gather carry
        # the payloads even at this size
        monkeypatch.setenv("MR_SMALL_SORT_N", small_sort)
    cols = [t.to(DEV) for t in relations[f64]]
    keep = [t.clone() for t in cols]
    res = JoinJob(DEV, how=how).run(*cols)
    assert jc.job_lists(res) == job_expected[(f64, how)]
    assert len(job_expected[(f64, how)][0]) > 0
    assert res.lvals.dtype == cols[1].dtype
    for t, k in zip(cols, keep):
        assert torch.equal(t.view(torch.int64), k.view(torch.int64))


def test_join_job_default_limit_and_too_large(relations):
    from mapreduce_amd.gpu.join import ROW_BYTES, JoinJob

    job = JoinJob(DEV, how="inner")
    free, _ = torch.cuda.mem_get_info(torch.device(DEV))
    assert 0 < job._limit() <= free // ROW_BYTES
    cols = [t.to(DEV) for t in relations[False]]
    with pytest.raises(ops.JoinTooLarge):
        JoinJob(DEV, how="inner", max_rows=100).run(*cols)


@pytest.fixture()
def rccl_ws1(monkeypatch):
    assert torch.cuda.is_available()
    import torch.distributed as td

    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", "29587")  # this file's own
    torch.cuda.set_device(0)
    td.init_process_group("nccl", rank=0, world_size=1,
                          device_id=torch.device("cuda", 0))
    monkeypatch.setenv("MR_FORCE_COLLECTIVE", "1")
    try:
        yield td
    finally:
        td.destroy_process_group()


def test_join_job_through_real_rccl(rccl_ws1, relations, job_expected):
    """Every collective call site of the join — the packed count
    exchange, the four all-to-alls, the size all-gather — on RCCL at
    world 1 (self-exchange)."""
    from mapreduce_amd.gpu import dist as dx
    from mapreduce_amd.gpu.join import JoinJob

    assert dx.force_collectives()
    cols = [t.to(DEV) for t in relations[True]]
    res = JoinJob(DEV, how="inner").run(*cols)
    assert jc.job_lists(res) == job_expected[(True, "inner")]
    with pytest.raises(ops.JoinTooLarge):
        JoinJob(DEV, how="inner", max_rows=100).run(*cols)


# --------------------------------------------------------------- the Server

@pytest.mark.parametrize("how", ["inner", "left"])
def test_join_tables_on_hardware(how, monkeypatch):
    import importlib

    import mapreduce_amd.examples.join_tables as jt
    from mapreduce_amd import job as jobmod
    from mapreduce_amd.parallel.coord import LocalCoordinator
    from mapreduce_amd.server import Server

    monkeypatch.delenv("MR_GPU_TIER", raising=False)
    importlib.reload(jt)
    jobmod._module_cache.clear()
    jobmod._inited.clear()
    args = {"how": how, "seed": 8, "nl": 4000, "nr": 3000, "nkeys": 900,
            "splits": 4, "parts": 4}
    roles = ("taskfn", "mapfn", "partitionfn", "reducefn", "finalfn")
    srv = Server(coord=LocalCoordinator()).configure(
        {"fns": {r: jt for r in roles}, "verbose": False,
         "init_args": args})
    assert srv._gpu_engine_kind() == "join"
    srv.loop()
    assert srv.finished
    assert srv.stats["tier"] == "gpu" and srv.stats["engine"] == "join"
    # the oracle: right rows by key, walked in left row order
    left, right = jt.make_relations(8, 4000, 3000, 900)
    rows = {}
    for k, r in right:
        rows.setdefault(k, []).append(r)
    exp = {}
    for k, l in left:
        rs = rows.get(k)
        if rs:
            exp.setdefault(k, []).extend((l, r) for r in rs)
        elif how == "left":
            exp.setdefault(k, []).append((l, None))
    exp = {k: sorted(v, key=jt._order) for k, v in exp.items()}
    assert dict(jt.RESULTS) == exp
    assert list(jt.RESULTS) == sorted(jt.RESULTS)
