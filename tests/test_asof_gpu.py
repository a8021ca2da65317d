"""The as-of kernels, the op, AsofJoinJob and the Server routing on the
device.  Every comparison is exact: against the brute-force oracle of
asof_common and against the CPU tier.  Sizes come from the extension
(ops.asof_caps): T left rows per tile, W right rows of a window in LDS."""

import pytest
import torch

import asof_common as ac
from mapreduce_amd import ops
from mapreduce_amd.ops import _cpu

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

PY_CAPS = (ops.ASOF_TILE, ops.ASOF_WIN)


@pytest.fixture(scope="module")
def caps():
    return ops.asof_caps()


def test_caps_come_from_the_extension(caps):
    assert caps == tuple(ops.ext().asof_caps())
    assert caps == PY_CAPS


# parametrised by name over the Python constants; the test checks they are
# the extension's, so the ids name the cases the device actually runs
@pytest.mark.parametrize("kernel", ["window", "row"])
@pytest.mark.parametrize("name", sorted(ac.cases(*PY_CAPS)))
def test_asof_sorted_matches_oracle_and_cpu_tier(name, kernel, caps,
                                                 monkeypatch):
    assert caps == PY_CAPS
    if kernel == "row":  # read per call: the thread-per-row kernel
        monkeypatch.setenv("MR_ASOF_ROW", "1")
    else:
        monkeypatch.delenv("MR_ASOF_ROW", raising=False)
    case = ac.cases(*caps)[name]
    bufs, views = ac.baited(case, DEV)
    assert all(v.data_ptr() % 16 for v in views if v.numel())
    keep = [b.clone() for b in bufs]
    host = (ac.to_i64(case.lk), ac.times_tensor(case.lt, case.f64),
            ac.to_i64(case.rk), ac.times_tensor(case.rt, case.f64))
    for d, exact, tol in ac.modes(case):
        got = ops.asof_sorted(*views, direction=d, tolerance=tol,
                              allow_exact=exact)
        assert got.is_cuda and got.dtype == torch.int64
        got = got.cpu().tolist()
        assert got == ac.expected(caps, name, d, exact, tol), (d, exact, tol)
        assert got == _cpu.asof_sorted(*host, d, tol, exact).tolist(), (
            d, exact, tol)
    for b, k in zip(bufs, keep):
        assert torch.equal(b.view(torch.int64), k.view(torch.int64))


def test_host_checks():
    k = ac.to_i64([1, 2, 2, 3]).to(DEV)
    t = torch.tensor([1, 2, 3, 4], device=DEV)
    f = t.to(torch.float64)
    assert ops.asof_sorted(k, t, k, t).cpu().tolist() == [0, 1, 2, 3]
    assert ops.asof_sorted(k, f, k, f, "forward").cpu().tolist() == [
        0, 1, 2, 3]
    e = ops.ext().asof_sorted
    # dtype
    with pytest.raises(TypeError):
        ops.asof_sorted(k.to(torch.int32), t, k, t)
    with pytest.raises(TypeError):
        ops.asof_sorted(k, t.to(torch.int32), k, t.to(torch.int32))
    with pytest.raises(TypeError, match="dtype"):
        ops.asof_sorted(k, t, k, f)
    with pytest.raises(RuntimeError, match="lkeys must be int64"):
        e(k.to(torch.int32), t, k, t)
    with pytest.raises(RuntimeError, match="rtimes must be int64"):
        e(k, t, k, f)
    # device
    with pytest.raises(RuntimeError, match="rkeys must be on GPU"):
        ops.asof_sorted(k, t, k.cpu(), t)
    with pytest.raises(RuntimeError, match="ltimes must be on GPU"):
        ops.asof_sorted(k, t.cpu(), k, t)
    # contiguity
    with pytest.raises(RuntimeError, match="rtimes must be contiguous"):
        ops.asof_sorted(k, t, k, torch.stack([t, t], 1)[:, 0])
    with pytest.raises(RuntimeError, match="lkeys must be contiguous"):
        ops.asof_sorted(torch.stack([k, k], 1)[:, 0], t, k, t)
    # one time per key
    with pytest.raises(ValueError, match="one time per key"):
        ops.asof_sorted(k, t[:3], k, t)
    with pytest.raises(RuntimeError, match="one time per left key"):
        e(k, t[:3], k, t)
    with pytest.raises(RuntimeError, match="one time per right key"):
        e(k, t, k[:2], t)
    # the tolerance range
    for tol in (-1, 2 ** 63):
        with pytest.raises(ValueError, match="tolerance"):
            ops.asof_sorted(k, t, k, t, tolerance=tol)
    with pytest.raises(TypeError, match="tolerance"):
        ops.asof_sorted(k, f, k, f, tolerance=1)
    with pytest.raises(RuntimeError, match=r"tolerance must be in \[0, 2\^63"):
        e(k, t, k, t, tolerance=-1)
    with pytest.raises(RuntimeError, match="tolerance needs int64 times"):
        e(k, t, k, t, tolerance=1, f64=True)
    assert ops.asof_sorted(k, t, k, t, tolerance=2 ** 63 - 1).cpu().tolist() \
        == [0, 1, 2, 3]
    # a known direction
    with pytest.raises(ValueError, match="direction"):
        ops.asof_sorted(k, t, k, t, direction="sideways")
    for d in (-1, 3):
        with pytest.raises(RuntimeError, match="direction must be"):
            e(k, t, k, t, direction=d)


# -------------------------------------------------------------- AsofJoinJob

JOB_MODES = {False: ("nearest", 2, True), True: ("backward", None, False)}


@pytest.fixture(scope="module")
def relations():
    """Six columns per dtype (i64 times and values / f64 times and values),
    5 000 x 3 000 rows over 700 keys, on the host; the oracle rows are
    computed once per (dtype, how) and shared."""
    rel = {}
    for f64 in (False, True):
        lk, lt, lv = ac.make_relation(31, 5000, 700, f64, f64)
        rk, rt, rv = ac.make_relation(32, 3000, 700, f64, f64)
        rk[:1000] = lk[:1000]
        rel[f64] = (lk, lt, lv, rk, rt, rv)
    return rel


@pytest.fixture(scope="module")
def job_expected(relations):
    return {(f64, how): ac.job_oracle(*relations[f64], *JOB_MODES[f64], how)
            for f64 in relations for how in ("left", "inner")}


@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("how", ["left", "inner"])
def test_asof_job_on_device(how, f64, relations, job_expected):
    from mapreduce_amd.gpu.asof import AsofJoinJob

    cols = [t.to(DEV) for t in relations[f64]]
    keep = [t.clone() for t in cols]
    direction, tol, exact = JOB_MODES[f64]
    res = AsofJoinJob(DEV, direction=direction, tolerance=tol,
                      allow_exact=exact, how=how).run(*cols)
    exp = job_expected[(f64, how)]
    assert ac.job_rows(res) == exp
    assert any(r[5] for r in exp)
    assert (how == "inner") != any(not r[5] for r in exp)
    assert res.ltimes.dtype == res.rtimes.dtype == cols[1].dtype
    assert res.lvals.dtype == cols[2].dtype
    assert res.rvals.dtype == cols[5].dtype
    assert (res.matched is None) == (how == "inner")
    for t, k in zip(cols, keep):
        assert torch.equal(t.view(torch.int64), k.view(torch.int64))


# --------------------------------------------------------------- the Server

@pytest.mark.parametrize("opts", [
    {"direction": "backward"},
    {"direction": "nearest", "tolerance": 6, "strict": True, "inner": True},
], ids=("backward", "nearest_tol_strict_inner"))
def test_asof_quotes_on_hardware(opts, monkeypatch):
    import importlib

    import mapreduce_amd.examples.asof_quotes as aq
    from mapreduce_amd import job as jobmod
    from mapreduce_amd.parallel.coord import LocalCoordinator
    from mapreduce_amd.server import Server

    monkeypatch.delenv("MR_GPU_TIER", raising=False)
    importlib.reload(aq)
    jobmod._module_cache.clear()
    jobmod._inited.clear()
    args = dict(opts, seed=8, nl=4000, nr=3000, nkeys=300, splits=4, parts=4)
    roles = ("taskfn", "mapfn", "partitionfn", "reducefn", "finalfn")
    srv = Server(coord=LocalCoordinator()).configure(
        {"fns": {r: aq for r in roles}, "verbose": False,
         "init_args": args})
    assert srv._gpu_engine_kind() == "asof"
    srv.loop()
    assert srv.finished
    assert srv.stats["tier"] == "gpu" and srv.stats["engine"] == "asof"
    left, right = aq.make_relations(8, 4000, 3000, 300)
    exp = ac.brute_quotes(left, right, opts["direction"],
                          opts.get("tolerance"), opts.get("strict", False),
                          opts.get("inner", False))
    exp = {k: sorted(v, key=aq._order) for k, v in exp.items()}
    assert any(r[2] is not None for v in exp.values() for r in v)
    assert dict(aq.RESULTS) == exp
    assert list(aq.RESULTS) == sorted(aq.RESULTS)
