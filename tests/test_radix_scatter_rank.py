"""The staged radix scatter that ranks once from registers (v3), called
through radix_bucketize and radix_sort_pairs directly and compared bit for
bit with a host reference: numpy's stable argsort on the digit, after
dropping all-ones keys where skip_empty is set.

The shapes sit on every boundary of the kernel's blocked mapping (wave w,
round r, lane l owns tile index (w*ITEMS + r)*64 + l): lane edges, one
wave's block of ITEMS*64 records for both ITEMS, tile edges.  The digit
patterns aim at the wave-private counts: one digit only (a cross-round count
of a whole tile in one cell; a missing wave-level ordering between rounds
shows here), all digits distinct per round, a digit seen by the last wave
only, two digits alternating per lane, random.  Payloads are distinct per
record, so a record in a wrong slot shows even among equal keys.

The same case list runs in this process (the default kernel), and in one
fresh child process each with MR_RADIX_V2=1 (the predecessor kernel, kept
for A/B) and MR_RS_ITEMS=4 (half tile): the switches are read once per
process."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

import radix_common as rc
from bucket_common import EMPTY

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = rc.T                # records per tile in this process
W = rc.ITEMS * 64       # one wave's share of a tile
SIZES = sorted({1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 2047, 2048,
                2049, 2 * 2048 + 1, T - 1, T, T + 1, 2 * T + 1})
PATTERNS = ("one", "cycle", "lastwave", "alternating", "random")
SHIFTS = (0, 56)
PAYLOADS = (None, np.int32, np.int64)
SKIP_LAYOUTS = ("wave_share", "middle_tile", "straddle", "all_pads",
                "scattered")


def digits(pattern, n, rng):
    i = np.arange(n)
    if pattern == "one":
        return np.full(n, 0xA7, dtype=np.uint64)
    if pattern == "cycle":
        return (i % 256).astype(np.uint64)
    if pattern == "lastwave":
        d = rng.integers(0, 200, size=n).astype(np.uint64)
        d[i % T >= T - W] = 201
        return d
    if pattern == "alternating":
        return np.where(i % 2 == 0, 3, 250).astype(np.uint64)
    return rng.integers(0, 256, size=n).astype(np.uint64)


def make_keys(pattern, n, shift, seed):
    """The pattern's digit at `shift`, noise in every other bit."""
    rng = np.random.default_rng(seed)
    noise = rng.integers(0, 2 ** 64 - 1, size=n, dtype=np.uint64,
                         endpoint=True)
    hole = np.uint64(~(0xFF << shift) & 0xFFFFFFFFFFFFFFFF)
    k = (noise & hole) | (digits(pattern, n, rng) << np.uint64(shift))
    k[k == EMPTY] = np.uint64(1)  # a pad only where a case puts one
    return k


def make_vals(n, dtype):
    if dtype is None:
        return None
    if dtype == np.int32:
        return (np.arange(n, dtype=np.int64) * 7 - 1000).astype(np.int32)
    return (np.arange(n, dtype=np.int64) << 20) - 12345


def skip_case(layout, seed):
    """-> keys with pads placed by `layout` (random digits at shift 56 and
    0 alike: the noise covers both)."""
    rng = np.random.default_rng(seed)
    n = 3 * T + 5
    k = make_keys("random", n, 56, seed)
    if layout == "wave_share":      # exactly wave 1 of tile 1
        k[T + W:T + 2 * W] = EMPTY
    elif layout == "middle_tile":   # all of tile 1
        k[T:2 * T] = EMPTY
    elif layout == "straddle":      # over a wave edge and over a tile edge
        k[W - 10:W + 23] = EMPTY
        k[2 * T - 5:2 * T + 70] = EMPTY
    elif layout == "all_pads":
        k[:] = EMPTY
    else:
        k[rng.random(n) < 0.17] = EMPTY
    return k


def reference(keys, vals, shift, skip):
    live = keys != EMPTY if skip else np.ones(keys.size, dtype=bool)
    lk = keys[live]
    d = ((lk >> np.uint64(shift)) & np.uint64(0xFF)).astype(np.int64)
    order = np.argsort(d, kind="stable")
    off = np.zeros(257, dtype=np.int64)
    np.cumsum(np.bincount(d, minlength=256), out=off[1:])
    return lk[order], (None if vals is None else vals[live][order]), off


def check_bucketize(dev, keys, vals, shift, skip):
    import torch
    from mapreduce_amd import ops
    k = torch.from_numpy(keys.view(np.int64).copy()).to(dev)
    v = (torch.empty(0, dtype=torch.int64, device=dev) if vals is None
         else torch.from_numpy(vals.copy()).to(dev))
    k0, v0 = k.clone(), v.clone()
    ok, ov, off = ops.ext().radix_bucketize(k, v, shift, skip)
    ek, ev, eoff = reference(keys, vals, shift, skip)
    what = f"n={keys.size} shift={shift} skip={skip}"
    np.testing.assert_array_equal(off.cpu().numpy(), eoff, err_msg=what)
    m = int(eoff[256])
    np.testing.assert_array_equal(rc.u64(ok)[:m], ek, err_msg=what)
    if vals is None:
        assert ov.numel() == 0
    else:
        assert ov.dtype == v.dtype
        np.testing.assert_array_equal(ov.cpu().numpy()[:m], ev, err_msg=what)
    assert torch.equal(k, k0), f"{what}: keys changed"
    assert torch.equal(v, v0), f"{what}: payload changed"


def run_plain(dev, pattern, shift, payload):
    for n in SIZES:
        keys = make_keys(pattern, n, shift, seed=n * 131 + shift)
        check_bucketize(dev, keys, make_vals(n, payload), shift, False)
    return len(SIZES)


def run_skip(dev, layout, shift, payload):
    keys = skip_case(layout, seed=SKIP_LAYOUTS.index(layout) + 77)
    check_bucketize(dev, keys, make_vals(keys.size, payload), shift, True)
    return 1


def run_full_sort(dev):
    """One 64-bit radix_sort_pairs over two tiles and a record, from a pool
    of 64 values so that equal keys abound, against the stable argsort."""
    import torch
    from mapreduce_amd import ops
    keys = rc.make_keys(("dupes", 2 * 2048 + 1, 64))
    ek, eorder = rc.oracle(keys)
    k = torch.from_numpy(keys.view(np.int64).copy()).to(dev)
    v = torch.arange(keys.size, dtype=torch.int64, device=dev)
    k0, v0 = k.clone(), v.clone()
    sk, sv = ops.ext().radix_sort_pairs(k, v, 64)
    np.testing.assert_array_equal(rc.u64(sk), ek)
    np.testing.assert_array_equal(sv.cpu().numpy(), eorder)
    assert torch.equal(k, k0) and torch.equal(v, v0)
    return 1


PLAIN = [(p, s, v) for p in PATTERNS for s in SHIFTS for v in PAYLOADS]
SKIPS = [(l, s, v) for l in SKIP_LAYOUTS for s in SHIFTS for v in PAYLOADS]


def plain_id(c):
    return f"{c[0]}-s{c[1]}-{'none' if c[2] is None else c[2].__name__}"


@pytest.fixture(scope="module")
def dev():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from mapreduce_amd import ops
    ops.require_gpu_ext()
    assert int(ops.ext().radix_sort_caps()[0]) == T
    return torch.device("cuda:0")


@pytest.mark.parametrize("case", PLAIN, ids=plain_id)
def test_bucketize_matches_stable_argsort(dev, case):
    run_plain(dev, *case)


@pytest.mark.parametrize("case", SKIPS, ids=plain_id)
def test_bucketize_skip_drops_pads(dev, case):
    run_skip(dev, *case)


def test_all_pads_leave_nothing(dev):
    import torch
    from mapreduce_amd import ops
    keys = skip_case("all_pads", 1)
    k = torch.from_numpy(keys.view(np.int64).copy()).to(dev)
    v = torch.arange(keys.size, dtype=torch.int64, device=dev)
    _, _, off = ops.ext().radix_bucketize(k, v, 56, True)
    assert not off.cpu().numpy().any()


def test_view_at_an_odd_element(dev):
    """Keys and payload that start 8 bytes into their storage: contiguous,
    but not 16-byte aligned, so no path may assume wider loads."""
    import torch
    from mapreduce_amd import ops
    n = 2 * T + 1
    keys = make_keys("random", n + 1, 56, seed=5)
    keys[7::11] = EMPTY
    vals = make_vals(n + 1, np.int64)
    k = torch.from_numpy(keys.view(np.int64).copy()).to(dev)[1:]
    v = torch.from_numpy(vals.copy()).to(dev)[1:]
    assert k.is_contiguous() and k.data_ptr() % 16 == 8
    for skip in (False, True):
        ok, ov, off = ops.ext().radix_bucketize(k, v, 56, skip)
        ek, ev, eoff = reference(keys[1:], vals[1:], 56, skip)
        m = int(eoff[256])
        np.testing.assert_array_equal(off.cpu().numpy(), eoff)
        np.testing.assert_array_equal(rc.u64(ok)[:m], ek)
        np.testing.assert_array_equal(ov.cpu().numpy()[:m], ev)


def test_full_sort_two_tiles_and_one(dev):
    run_full_sort(dev)


# ------------------------------------------------------- kernel variants
def child_main():
    """Body of a variant child: every case above, then one JSON line."""
    import torch
    from mapreduce_amd import ops
    ops.require_gpu_ext()
    dev = torch.device("cuda:0")
    tile = int(ops.ext().radix_sort_caps()[0])
    assert tile == T, (tile, T)
    calls = sum(run_plain(dev, *c) for c in PLAIN)
    calls += sum(run_skip(dev, *c) for c in SKIPS)
    calls += run_full_sort(dev)
    print(json.dumps({"calls": calls, "expected": EXPECTED_CALLS,
                      "tile": tile}))


CHILD = ("import sys; sys.path[:0] = [{root!r}, {tests!r}]; "
         "import test_radix_scatter_rank as t; t.child_main()")
EXPECTED_CALLS = len(PLAIN) * len(SIZES) + len(SKIPS) + 1


def run_variant(var, value):
    env = dict(os.environ)
    for name in ("MR_RADIX_V1", "MR_RADIX_V2", "MR_RS_ITEMS"):
        env.pop(name, None)
    env[var] = value
    code = CHILD.format(root=ROOT, tests=os.path.join(ROOT, "tests"))
    out = subprocess.run([sys.executable, "-c", code], env=env, cwd=ROOT,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-4000:])
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_variant_previous_kernel(dev):
    """MR_RADIX_V2=1: the scatter with per-round block barriers."""
    r = run_variant("MR_RADIX_V2", "1")
    assert r["tile"] == 2048
    assert r["calls"] == EXPECTED_CALLS > 0


def test_variant_half_tile(dev):
    """MR_RS_ITEMS=4: the same kernel on 1024-record tiles."""
    r = run_variant("MR_RS_ITEMS", "4")
    assert r["tile"] == 1024
    assert r["calls"] == r["expected"] > 0  # its SIZES follow its tile
