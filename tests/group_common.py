"""Shared pieces of the group tests: a pure-Python oracle that shares no code
with the ops (sorted() per group on an order key written out here, integer
index arithmetic, len(set(...))), the case generators and the bait-flanked
input slices.

A case is a list of group lengths over key-sorted rows; a value family
fills the value column.  Values are compared through their int64 bit
patterns or their order keys, never through float ==.
"""

import functools
import random
import struct

import numpy as np
import torch

M64 = (1 << 64) - 1
SIGN = 1 << 63
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
FAMILIES = ("random_i64", "equal", "ascending", "descending", "two_valued",
            "f64")
COMBINES = (None, ("topk", 3), ("bottomk", 2), "distinct")


# ---- the order key, written out in Python ---------------------------------

def f64_bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def okey(bits, f64):
    """u64 order key of a value given as its u64 bit pattern."""
    if not f64:
        return bits ^ SIGN
    if bits in (0, SIGN):                      # +0.0 and -0.0: one key
        return SIGN
    if (bits & ~SIGN & M64) > 0x7FF0000000000000:   # every NaN: one key
        return M64
    return (bits ^ M64) if bits & SIGN else (bits ^ SIGN)


def to_bits(t):
    """i64 or f64 tensor -> list of u64 bit patterns."""
    return t.cpu().contiguous().view(torch.int64).numpy().view(
        np.uint64).tolist()


def okeys(t):
    f64 = t.dtype == torch.float64
    return [okey(b, f64) for b in to_bits(t)]


# ---- cases: lists of group lengths ----------------------------------------

@functools.lru_cache(maxsize=None)
def cases(C):
    """name -> tuple of group lengths; C = (T, R), T = ops.group_caps()[0]
    rows per tile, R = ops.group_rank_max() the longest group the tile
    kernel orders by rank counting."""
    T, R = C
    return {
        "n0": (),
        "n1": (1,),
        "n2_one": (2,),
        "n2_two": (1, 1),
        "singles": (1,) * (T + 3),
        "tile_exact": (T,),
        "straddle_by_one": (T - 1, 2),
        "last_row_start": (T - 1, 5),
        "threes": (3,) * T + (1,),              # 3T + 1 rows
        "long": (3 * T + 17,),
        "whole": (5 * T + 5,),
        "mix": (T - 1, 2, T, 1, 2 * T + 1, 5),
        # around the threshold between the tile kernel's two sorts
        "rank_max": (R,) * 3 + (R - 1, 1),
        "rank_over": (R, R + 1, R),
        # short groups beside one that leaves the tile: rank counting with
        # rows that are not the tile's to finish, on either side
        "short_then_long": (10, T, 7),
        "short_random": tuple(random.Random(5).randrange(1, 40)
                              for _ in range(300)),
    }


def offsets_of(lens):
    off = [0]
    for n in lens:
        off.append(off[-1] + n)
    return off


def straddler_rows(lens, T):
    """Rows in groups that cross a boundary between tiles of T rows."""
    off = offsets_of(lens)
    return sum(b - a for a, b in zip(off, off[1:])
               if a // T != (b - 1) // T)


def case_keys(lens):
    """Ascending u64 keys on both halves of the sign bit, one per group."""
    m = len(lens)
    ks = sorted({(i * 0x9E3779B97F4A7C15 + 12345) & M64 for i in range(m)})
    assert len(ks) == m
    if m >= 2:
        ks[0], ks[-1] = 0, M64
    return [k for k, n in zip(ks, lens) for _ in range(n)]


def to_i64(keys):
    return torch.from_numpy(
        np.array(list(keys), dtype=np.uint64).view(np.int64).copy())


F64_SPECIALS = (0.0, -0.0, float("inf"), float("-inf"), 5e-324, -5e-324,
                2.2250738585072014e-308, 1.5, -1.5)
NAN_BITS = (0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001,
            0xFFFFFFFFFFFFFFFF)


def case_values(family, n, seed=1):
    """The value column of a family: i64, or f64 for "f64"."""
    rng = random.Random(seed * 1000003 + n)
    if family == "f64":
        bits = []
        for i in range(n):
            r = i % 7
            if r == 0:
                bits.append(f64_bits(F64_SPECIALS[(i // 7)
                                                  % len(F64_SPECIALS)]))
            elif r == 3:
                bits.append(NAN_BITS[(i // 7) % len(NAN_BITS)])
            else:
                bits.append(f64_bits(rng.uniform(-1e6, 1e6)))
        rng.shuffle(bits)
        return to_i64(bits).view(torch.float64)
    if family == "random_i64":
        vals = [rng.randrange(I64_MIN, I64_MAX + 1) for _ in range(n)]
        for j, x in enumerate((I64_MIN, I64_MAX, 0, -1)):
            if j < n:
                vals[rng.randrange(n)] = x
    elif family == "equal":
        vals = [-7] * n
    elif family == "ascending":
        vals = [i - n // 2 for i in range(n)]
    elif family == "descending":
        vals = [n // 2 - i for i in range(n)]
    elif family == "two_valued":
        vals = [rng.choice((I64_MIN, 42)) for _ in range(n)]
    else:
        raise ValueError(family)
    return torch.tensor(vals, dtype=torch.int64)


@functools.lru_cache(maxsize=None)
def case_data(C, name, family):
    """(keys i64 tensor, vals tensor, offsets list), built once."""
    lens = cases(C)[name]
    n = sum(lens)
    return to_i64(case_keys(lens)), case_values(family, n), offsets_of(lens)


# ---- the oracle ------------------------------------------------------------

def oracle_sorted_okeys(off, vals):
    """Order keys of the value column ordered within each group."""
    ok = okeys(vals)
    out = []
    for a, b in zip(off, off[1:]):
        out.extend(sorted(ok[a:b]))
    return out


def oracle_sorted_bits(off, vals):
    """Bit patterns ordered within each group, equal order keys in input
    order (sorted() is stable) — what both tiers produce."""
    bits = to_bits(vals)
    f64 = vals.dtype == torch.float64
    out = []
    for a, b in zip(off, off[1:]):
        out.extend(sorted(bits[a:b], key=lambda x: okey(x, f64)))
    return out


@functools.lru_cache(maxsize=None)
def expected(C, name, family):
    _, vals, off = case_data(C, name, family)
    return oracle_sorted_okeys(off, vals), oracle_sorted_bits(off, vals)


def rank_index(num, den, higher, length):
    return (num * (length - 1) + (den - 1 if higher else 0)) // den


def oracle_quantiles(off, sorted_ok, specs):
    return [[sorted_ok[a + rank_index(n, d, h, b - a)] for n, d, h in specs]
            for a, b in zip(off, off[1:])]


def oracle_topk(off, sorted_ok, k, largest):
    """-> (order keys per group, padded with None), counts."""
    rows, cnt = [], []
    for a, b in zip(off, off[1:]):
        g = sorted_ok[a:b]
        g = g[::-1][:k] if largest else g[:k]
        cnt.append(len(g))
        rows.append(g + [None] * (k - len(g)))
    return rows, cnt


def oracle_distinct(off, vals):
    ok = okeys(vals)
    return [len(set(ok[a:b])) for a, b in zip(off, off[1:])]


def baited(keys, vals, device="cpu"):
    """-> (kbuf, vbuf, kview, vview): the columns as exact-size slices of
    larger tensors.  The flanks continue the first and the last group (same
    key) with values below and above everything inside, so a read outside
    [0, n) changes the answer."""
    n = keys.numel()
    kb = torch.empty(n + 2, dtype=torch.int64)
    kb[1:n + 1] = keys
    kb[0] = keys[0] if n else 0
    kb[n + 1] = keys[-1] if n else 0
    vb = torch.empty(n + 2, dtype=torch.int64)
    vb[1:n + 1] = vals.view(torch.int64)
    if vals.dtype == torch.float64:
        lo, hi = f64_bits(float("-inf")), f64_bits(float("inf"))
        vb[0], vb[n + 1] = to_i64([lo])[0], to_i64([hi])[0]
    else:
        vb[0], vb[n + 1] = I64_MIN, I64_MAX
    kb, vb = kb.to(device), vb.to(device).view(vals.dtype)
    return kb, vb, kb[1:n + 1], vb[1:n + 1]


# ---- GroupedValuesJob: unsorted rows ---------------------------------------

def make_rows(seed, n, nkeys, f64, hot=0):
    """n unsorted rows over nkeys keys on both halves of the sign bit, plus
    `hot` rows of one more key."""
    rng = random.Random(seed)
    pool = [rng.randrange(1 << 64) for _ in range(nkeys)] + [0, M64]
    keys = [rng.choice(pool) for _ in range(n)] + [pool[0] ^ 1] * hot
    rng.shuffle(keys)
    vals = case_values("f64" if f64 else "random_i64", len(keys), seed)
    if not f64:  # duplicates, so that distinct has something to drop
        vals = vals >> 60
    return to_i64(keys), vals


def trim(ok, combine):
    """One group's ascending order keys under a combine."""
    if combine is None:
        return ok
    if combine == "distinct":
        return sorted(set(ok))
    what, k = combine
    return ok[-k:] if what == "topk" else ok[:k]


def job_oracle(keys, vals, combine=None, world=1, rank=0):
    """-> (u64 keys ascending, offsets, order keys of the values) of the
    partition of `rank`."""
    groups = {}
    for k, o in zip(to_bits(keys), okeys(vals)):
        groups.setdefault(k, []).append(o)
    uk, off, out = [], [0], []
    for k in sorted(groups):
        if (k * world) >> 64 != rank:
            continue
        g = trim(sorted(groups[k]), combine)
        uk.append(k)
        out.extend(g)
        off.append(len(out))
    return uk, off, out


def job_lists(res):
    return (to_bits(res.keys), res.offsets.cpu().tolist(), okeys(res.values))
