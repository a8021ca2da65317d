"""Shared pieces of the full radix-sort tests (not a test module): seeded
key families, the NumPy oracle, the case lists and the checker that the GPU
tests, the CPU self-check and the child-process variants all run.

Contract under test: for keys below 2**bits, radix_sort_pairs /
radix_sort_idx32 / ops.sort_pairs(..., bits=bits) all equal the full 64-bit
stable sort, np.argsort(keys_u64, kind="stable")."""

import json
import os
import zlib

import numpy as np

EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
ITEMS = 4 if os.environ.get("MR_RS_ITEMS") == "4" else 8
T = 256 * ITEMS  # records per radix tile in this process
SIZES = [1, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, 3 * T + 17,
         40 * T + 5]
BITS = [1, 8, 9, 16, 20, 33, 63, 64]
BACKGROUND = 0x5AC3A53C96E17B2D  # constant bytes of the single-live-byte
                                 # families: all eight differ


def _limit(bits):
    return (1 << bits) - 1  # largest key below 2**bits


def _rand(rng, n, bits):
    return rng.integers(0, _limit(bits), size=n, dtype=np.uint64,
                        endpoint=True)


def fam_random(rng, n, bits):
    """Full range below 2**bits; from 64 keys up, the top bit in use is
    pinned on in one key and off in another."""
    k = _rand(rng, n, bits)
    if n >= 64:
        top = np.uint64(1 << (bits - 1))
        k[n // 3] |= top
        k[n // 2] &= ~top
    return k


def fam_equal(rng, n, bits):
    """One value: a single digit run fills every tile and every wave's
    count lands in one bin per pass."""
    return np.full(n, int(_rand(rng, 1, bits)[0]) | 1, dtype=np.uint64)


def fam_alternating(rng, n, bits):
    """hi, lo, hi, lo, ...: the two values differ in every byte in use."""
    hi = _limit(bits) & 0xC3A5F00FE1D2B487 | 1 << (bits - 1)
    lo = _limit(bits) & ~hi
    k = np.empty(n, dtype=np.uint64)
    k[0::2] = hi
    k[1::2] = lo
    return k


def fam_sorted(rng, n, bits):
    return np.sort(_rand(rng, n, bits))


def fam_reverse(rng, n, bits):
    return np.sort(_rand(rng, n, bits))[::-1].copy()


def fam_ones(rng, n, bits):
    """~10 % of the keys are the all-ones pattern (the hash table's empty
    mark): the full sort has no skip, so they are data and sort last.
    64-bit only."""
    assert bits == 64
    k = _rand(rng, n, 64)
    k[rng.random(n) < 0.1] = EMPTY
    if n:
        k[n // 2] = EMPTY
    return k


def fam_dupes(rng, n, bits):
    """At most 64 distinct values spread over the bits in use, with the
    iota payload: the stability case."""
    pool = np.unique(np.concatenate(
        [_rand(rng, 62, bits), np.array([0, _limit(bits)], np.uint64)]))
    return pool[rng.integers(0, pool.size, size=n)]


def live_byte(p):
    def fam(rng, n, bits):
        """Random in byte p only, BACKGROUND elsewhere: pass p's shift is
        the only thing that orders the data.  64-bit only."""
        assert bits == 64
        keep = np.uint64(~(0xFF << 8 * p) & 0xFFFFFFFFFFFFFFFF)
        byte = rng.integers(0, 256, size=n, dtype=np.uint64)
        return (np.uint64(BACKGROUND) & keep) | (byte << np.uint64(8 * p))
    fam.__name__ = f"fam_live_byte{p}"
    return fam


FAMILIES = {
    "random": fam_random, "equal": fam_equal,
    "alternating": fam_alternating, "sorted": fam_sorted,
    "reverse": fam_reverse, "ones": fam_ones, "dupes": fam_dupes,
}
FAMILIES.update({f"byte{p}": live_byte(p) for p in range(8)})

# (family, n, bits).  Every size x every 64-bit family; the live-byte
# families at the tile edge and at several tiles; every partial `bits` x the
# families that can go wrong differently there x sizes on both sides of one
# tile.
FULL_CASES = (
    [(f, n, 64) for f in ("random", "equal", "alternating", "sorted",
                          "reverse", "ones", "dupes") for n in SIZES]
    + [(f"byte{p}", n, 64) for p in range(8)
       for n in (T - 1, T + 1, 3 * T + 17)]
    + [(f, n, b) for b in BITS if b != 64
       for f in ("random", "equal", "alternating", "dupes")
       for n in (257, T, T + 1, 3 * T + 17)]
    + [("random", 40 * T + 5, b) for b in (9, 20, 33)]
)
# what a child process with another kernel selected runs
VARIANT_CASES = [(f, n, b) for f in ("random", "equal", "dupes")
                 for n in (T - 1, T, T + 1, 3 * T + 17) for b in (20, 64)]


def case_id(case):
    f, n, b = case
    return f"{f}-n{n}-b{b}"


def make_keys(case):
    f, n, bits = case
    rng = np.random.default_rng(zlib.crc32(case_id(case).encode()))
    k = FAMILIES[f](rng, n, bits)
    assert k.dtype == np.uint64 and k.shape == (n,)
    return k


def make_column(case):
    """A random i64 column to carry through the idx32 permutation."""
    rng = np.random.default_rng(zlib.crc32(case_id(case).encode()) ^ 0x5EED)
    return rng.integers(-2 ** 63, 2 ** 63 - 1, size=case[1], dtype=np.int64)


def oracle(keys):
    """-> (sorted keys, permutation) of the full 64-bit stable sort."""
    order = np.argsort(keys, kind="stable")
    return keys[order], order.astype(np.int64)


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def _storage(t):
    return t.untyped_storage().data_ptr()


def check_gpu_case(case, dev, wrapper=True):
    """Run one case through radix_sort_pairs (with payload, keys only),
    radix_sort_idx32 + gather_by_u32 and, with `wrapper`, ops.sort_pairs;
    every result must equal the oracle, no input may change and, for
    n > 0, no output may alias an input."""
    import torch
    from mapreduce_amd import ops
    e = ops.ext()
    _, n, bits = case
    keys = make_keys(case)
    ek, eorder = oracle(keys)
    col = make_column(case)
    k = torch.from_numpy(keys.view(np.int64).copy()).to(dev)
    v = torch.arange(n, dtype=torch.int64, device=dev)
    c = torch.from_numpy(col.copy()).to(dev)
    empty = torch.empty(0, dtype=torch.int64, device=dev)
    k0, v0, c0 = k.clone(), v.clone(), c.clone()

    def same_inputs(what):
        assert torch.equal(k, k0), f"{what} changed its keys"
        assert torch.equal(v, v0), f"{what} changed its payload"
        assert torch.equal(c, c0), f"{what} changed the gathered column"

    def no_alias(what, *outs):
        ins = {_storage(k), _storage(v), _storage(c)}
        for o in outs:
            if o is not None and o.numel():
                assert _storage(o) not in ins, f"{what} aliases an input"

    sk, sv = e.radix_sort_pairs(k, v, bits)
    same_inputs("radix_sort_pairs")
    no_alias("radix_sort_pairs", sk, sv)
    assert sk.dtype == torch.int64 and sv.dtype == torch.int64
    np.testing.assert_array_equal(u64(sk), ek)
    np.testing.assert_array_equal(sv.cpu().numpy(), eorder)

    sk, sv = e.radix_sort_pairs(k, empty, bits)
    same_inputs("radix_sort_pairs (keys only)")
    no_alias("radix_sort_pairs (keys only)", sk)
    assert sv.numel() == 0
    np.testing.assert_array_equal(u64(sk), ek)

    sk, perm = e.radix_sort_idx32(k, bits)
    same_inputs("radix_sort_idx32")
    no_alias("radix_sort_idx32", sk, perm)
    assert perm.dtype == torch.int32
    np.testing.assert_array_equal(u64(sk), ek)
    np.testing.assert_array_equal(perm.cpu().numpy().astype(np.int64),
                                  eorder)
    g = e.gather_by_u32(c, perm)
    same_inputs("gather_by_u32")
    no_alias("gather_by_u32", g)
    np.testing.assert_array_equal(g.cpu().numpy(), col[eorder])

    if wrapper:
        sk, sv = ops.sort_pairs(k, v, bits=bits)
        same_inputs("ops.sort_pairs")
        no_alias("ops.sort_pairs", sk, sv)
        np.testing.assert_array_equal(u64(sk), ek)
        np.testing.assert_array_equal(sv.cpu().numpy(), eorder)
        sk, sv = ops.sort_pairs(k, None, bits=bits)
        assert sv is None
        np.testing.assert_array_equal(u64(sk), ek)


def child_main():
    """Body of a variant child process: VARIANT_CASES through the same
    checker, then one JSON line saying which kernels this process ran."""
    import torch
    from mapreduce_amd import ops
    ops.require_gpu_ext()
    dev = torch.device("cuda:0")
    for case in VARIANT_CASES:
        check_gpu_case(case, dev, wrapper=False)
    tile, direct = (int(x) for x in ops.ext().radix_sort_caps())
    k = torch.arange(8, dtype=torch.int64, device=dev)
    try:
        ops.ext().radix_bucketize(k, k, 56, False)
        bucketize = "ran"
    except RuntimeError as err:
        bucketize = str(err).splitlines()[0]
    print(json.dumps({"cases": len(VARIANT_CASES), "tile": tile,
                      "assumed_tile": T,
                      "scatter": "direct" if direct else "lds-staged",
                      "bucketize": bucketize}))
