"""The in-tree multi-pass radix sort, called directly (ops.sort_pairs sends
everything under 2^20 keys to torch.sort, so the wrapper alone never reaches
it at test sizes): radix_sort_pairs with and without payload and
radix_sort_idx32 + gather_by_u32 against np.argsort(kind="stable") at tile
edges, for every key family and `bits` of radix_common, with the inputs
checked unchanged and unaliased after every call.  The wrapper's torch path
must give the identical result for keys below 2**bits.  The kernels that
MR_RADIX_V1=1 and MR_RS_ITEMS=4 select are read once per process, so each
runs in one fresh child."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import radix_common as rc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mapreduce_amd import ops
    ops.require_gpu_ext()
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def default_small_sort(monkeypatch):
    # ops.sort_pairs must take its default (torch) path at these sizes
    monkeypatch.delenv("MR_SMALL_SORT_N", raising=False)
    monkeypatch.delenv("MR_SMALL_SORT_TORCH", raising=False)


def test_process_runs_the_assumed_tile(dev):
    from mapreduce_amd import ops
    tile, direct = ops.ext().radix_sort_caps()
    assert tile == rc.T
    assert direct == (os.environ.get("MR_RADIX_V1", "")[:1] == "1")


@pytest.mark.parametrize("case", rc.FULL_CASES, ids=rc.case_id)
def test_full_sort_matches_stable_argsort(dev, case):
    rc.check_gpu_case(case, dev)


@pytest.mark.parametrize("bits", [1, 20, 64])
def test_empty_input(dev, bits):
    from mapreduce_amd import ops
    e = ops.ext()
    k = torch.empty(0, dtype=torch.int64, device=dev)
    sk, sv = e.radix_sort_pairs(k, k.clone(), bits)
    assert sk.numel() == 0 and sv.numel() == 0
    assert sk.dtype == torch.int64 and sv.dtype == torch.int64
    sk, perm = e.radix_sort_idx32(k, bits)
    assert sk.numel() == 0 and perm.numel() == 0
    assert sk.dtype == torch.int64 and perm.dtype == torch.int32
    g = e.gather_by_u32(k, perm)
    assert g.numel() == 0 and g.dtype == torch.int64
    sk, sv = ops.sort_pairs(k, k.clone(), bits=bits)
    assert sk.numel() == 0 and sv.numel() == 0


def test_payload_is_carried_not_regenerated(dev):
    """A payload that is not the iota: the sort must move the caller's
    values, whatever they are (negative and repeated ones included)."""
    from mapreduce_amd import ops
    case = ("dupes", 3 * rc.T + 17, 64)
    keys = rc.make_keys(case)
    col = rc.make_column(case)
    col[::5] = col[0]
    ek, order = rc.oracle(keys)
    k = torch.from_numpy(keys.view(np.int64).copy()).to(dev)
    v = torch.from_numpy(col.copy()).to(dev)
    sk, sv = ops.ext().radix_sort_pairs(k, v, 64)
    np.testing.assert_array_equal(rc.u64(sk), ek)
    np.testing.assert_array_equal(sv.cpu().numpy(), col[order])


def test_mismatched_payload_is_refused(dev):
    """The extension checks the payload before any launch: wrong length,
    dtype, device or layout raise instead of being read as n u64 values."""
    from mapreduce_amd import ops
    e = ops.ext()
    # the guards arrived together with radix_sort_caps: without them the
    # calls below would read out of bounds, so do not make them
    assert hasattr(e, "radix_sort_caps")
    n = rc.T + 1
    k = torch.arange(n, dtype=torch.int64, device=dev)
    bad = {
        "short": torch.zeros(n - 1, dtype=torch.int64, device=dev),
        "one": torch.zeros(1, dtype=torch.int64, device=dev),
        "long": torch.zeros(n + 1, dtype=torch.int64, device=dev),
        "int32": torch.zeros(n, dtype=torch.int32, device=dev),
        "float64": torch.zeros(n, dtype=torch.float64, device=dev),
        "host": torch.zeros(n, dtype=torch.int64),
        "strided": torch.zeros(2 * n, dtype=torch.int64, device=dev)[::2],
    }
    for name, v in bad.items():
        with pytest.raises(RuntimeError, match="vals must be"):
            e.radix_sort_pairs(k, v, 64)
    for bits in (0, 65, -8):
        with pytest.raises(RuntimeError, match="bits in"):
            e.radix_sort_pairs(k, k.clone(), bits)
        with pytest.raises(RuntimeError, match="bits in"):
            e.radix_sort_idx32(k, bits)
    with pytest.raises(RuntimeError, match="keys must be"):
        e.radix_sort_pairs(k.cpu(), k.clone(), 64)


# ------------------------------------------------------- kernel variants
CHILD = ("import sys; sys.path[:0] = [{root!r}, {tests!r}]; "
         "import radix_common; radix_common.child_main()")


def run_variant(var, value):
    env = dict(os.environ)
    for name in ("MR_RADIX_V1", "MR_RS_ITEMS"):
        env.pop(name, None)
    env[var] = value
    code = CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))
    out = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    report = json.loads(out.stdout.strip().splitlines()[-1])
    print(f"{var}={value}: {report}")
    return report


def test_variant_direct_scatter(dev):
    """MR_RADIX_V1=1: the direct-scatter kernel, 2048-record tiles."""
    r = run_variant("MR_RADIX_V1", "1")
    assert r["cases"] == len(rc.VARIANT_CASES) > 0
    assert r["scatter"] == "direct"
    assert r["tile"] == r["assumed_tile"] == 2048
    assert "no direct-scatter" in r["bucketize"]


def test_variant_half_tile(dev):
    """MR_RS_ITEMS=4: the LDS-staged scatter on 1024-record tiles."""
    r = run_variant("MR_RS_ITEMS", "4")
    assert r["cases"] == len(rc.VARIANT_CASES) > 0
    assert r["scatter"] == "lds-staged"
    assert r["tile"] == r["assumed_tile"] == 1024
    assert r["bucketize"] == "ran"
