"""Shared pieces of the join tests: a brute-force oracle that shares no code
with the ops (a dict from right key to its row indices, walked in left row
order), the case generators, and the bait-flanked input slices.

Keys are Python ints in [0, 2^64) here and i64 bit patterns in tensors.
"""

import functools
import random

import numpy as np
import torch

HOWS = ("inner", "left", "semi", "anti")
M64 = (1 << 64) - 1
SIGN_KEYS = (0, 1, (1 << 63) - 1, 1 << 63, M64)


def to_i64(keys):
    """u64 ints -> i64 tensor of the same bit patterns."""
    return torch.from_numpy(
        np.array(list(keys), dtype=np.uint64).view(np.int64).copy())


def to_u64(t):
    """i64 tensor -> list of u64 ints."""
    return t.cpu().numpy().view(np.uint64).tolist()


def oracle(lk, rk, how):
    """lk, rk: u64 ints, each ascending.  -> (li, ri) lists for inner and
    left, li for semi and anti."""
    rows = {}
    for j, k in enumerate(rk):
        rows.setdefault(k, []).append(j)
    li, ri = [], []
    for i, k in enumerate(lk):
        m = rows.get(k)
        if how == "semi":
            if m:
                li.append(i)
        elif how == "anti":
            if not m:
                li.append(i)
        elif m:
            li.extend([i] * len(m))
            ri.extend(m)
        elif how == "left":
            li.append(i)
            ri.append(-1)
    return (li, ri) if how in ("inner", "left") else li


# the row counts every side must see; filled in with the tile size T
def sizes(T):
    return [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17]


def _dup_keys(rng, n, pool):
    return sorted(rng.choice(pool) for _ in range(n))


@functools.lru_cache(maxsize=None)
def cases(T, S, BT, W):
    """name -> (lk, rk), u64 ints ascending.  T, S = ops.join_caps(),
    BT, W = ops.join_bounds_caps()."""
    rng = random.Random(20240521)
    out = {}
    # 64 distinct values on both halves of the sign bit: heavy duplicates
    pool = sorted(rng.randrange(1 << 64) for _ in range(62)) + [0, M64]
    sz = sizes(T)
    # a subset of the size product: every value on each side, and 0 x n,
    # n x 0 (every case runs under every how)
    pairs = [(n, sz[(i + 4) % len(sz)]) for i, n in enumerate(sz)]
    pairs += [(0, 0), (0, T + 1), (T + 1, 0), (3 * T + 17, 3 * T + 17)]
    for nl, nr in pairs:
        out[f"dup64_{nl}x{nr}"] = (_dup_keys(rng, nl, pool),
                                   _dup_keys(rng, nr, pool))
    # all distinct and disjoint: no match
    out["disjoint"] = ([2 * i for i in range(T + 1)],
                       [2 * i + 1 for i in range(65)])
    # identical columns of unique keys: 1:1
    uniq = sorted({rng.randrange(1 << 64) for _ in range(3 * T + 17)})
    out["identical"] = (uniq, list(uniq))
    # all rows equal on both sides: every left run crosses tile boundaries
    out["all_equal"] = ([7] * 300, [7] * 300)
    # hot key A: one left row matching 3T + 5 right rows (four tiles)
    out["hot_a"] = ([3, 50, 90],
                    [10, 20] + [50] * (3 * T + 5) + [60, 70])
    # hot key B: S + 7 distinct left rows, one match each, inside one
    # tile's reach: the slice of offsets no longer fits in LDS
    b = [5 * i + 1 for i in range(S + 7)]
    out["hot_b"] = (b, list(b))
    # the same with long gaps of unmatched left rows inside one tile: the
    # slice is many times the LDS capacity
    g = [3 * i for i in range(10 * S + 3)]
    out["hot_b_gaps"] = (g, sorted([g[0], g[S], g[-1]] + [g[7 * S]] * 5))
    # keys straddling the sign bit: signed compares would misorder these
    out["sign"] = ([0, 1, (1 << 63) - 1, 1 << 63, 1 << 63, M64],
                   [1, (1 << 63) - 1, 1 << 63, 1 << 63, M64, M64])
    out["sign_disjoint"] = ([(1 << 63) - 1, M64], [0, 1 << 63])
    # the windowed bounds pass: one tile of left rows whose window of
    # right keys is exactly the LDS capacity, and one key longer; then the
    # same with a second tile of left rows behind it
    for extra in (0, 1):
        r = [11 * i + 4 for i in range(W + extra)]
        out[f"window_{W + extra}"] = (r[0:-1:3][:BT - 1] + [r[-1]], r)
    r = [11 * i + 4 for i in range(3 * W)]
    out["window_tiles"] = (sorted(r[::2] + r[:BT // 2]), r)
    # unmatched rows first, last and in between
    out["unmatched"] = ([1, 2, 2, 5, 7, 9, 9, 11], [2, 2, 3, 7, 7, 7, 9])
    return out


@functools.lru_cache(maxsize=None)
def expected(caps, name, how):
    lk, rk = cases(*caps)[name]
    return oracle(lk, rk, how)


def baited(lk, rk, device="cpu"):
    """-> (lbuf, rbuf, lview, rview): the columns as exact-size slices of
    larger tensors whose flanking elements are bait — next to the right
    column sits the last left key, next to the left column a right key —
    so a read outside [0, n) changes the answer."""
    lbait = rk[-1] if rk else 0
    rbait = lk[-1] if lk else 0
    lbuf = to_i64([rk[0] if rk else 0] + list(lk) + [lbait]).to(device)
    rbuf = to_i64([rbait] + list(rk) + [rbait]).to(device)
    return lbuf, rbuf, lbuf[1:1 + len(lk)], rbuf[1:1 + len(rk)]


def as_lists(res, how):
    if how in ("inner", "left"):
        return res[0].cpu().tolist(), res[1].cpu().tolist()
    return res.cpu().tolist()


# ---- JoinJob: unsorted relations with values ------------------------------

F64_SPECIALS = (-0.0, float("nan"), float("inf"), float("-inf"), 0.0, 1.5)


def make_relation(seed, n, nkeys, f64):
    """n rows: u64 keys with duplicates on both halves of the sign bit,
    and one value each (i64, or f64 including -0.0, NaN and inf)."""
    rng = random.Random(seed)
    pool = [rng.randrange(1 << 64) for _ in range(nkeys)] + [0, M64]
    keys = [rng.choice(pool) for _ in range(n)]
    if f64:
        vals = [F64_SPECIALS[i % len(F64_SPECIALS)] if i % 5 == 0
                else rng.uniform(-1e6, 1e6) for i in range(n)]
        vt = torch.tensor(vals, dtype=torch.float64)
    else:
        vt = torch.tensor([rng.randrange(-2 ** 63, 2 ** 63)
                           for _ in range(n)], dtype=torch.int64)
    return to_i64(keys), vt


def bits(t):
    """value column -> list of its int64 bit patterns (None stays None)."""
    if t is None:
        return None
    return t.cpu().contiguous().view(torch.int64).tolist()


def job_oracle(lkeys, lvals, rkeys, rvals, how):
    """Rows of the join of two UNSORTED relations, by key ascending (u64),
    then left input order, then right input order.  -> (keys u64, lval
    bits, rval bits or None, matched or None)."""
    lk, rk = to_u64(lkeys), to_u64(rkeys)
    lv, rv = bits(lvals), bits(rvals)
    rows = {}
    for j, k in enumerate(rk):
        rows.setdefault(k, []).append(j)
    keys, lo, ro, ma = [], [], [], []
    for i in sorted(range(len(lk)), key=lk.__getitem__):  # stable
        m = rows.get(lk[i])
        if how == "semi" or how == "anti":
            if bool(m) == (how == "semi"):
                keys.append(lk[i])
                lo.append(lv[i])
            continue
        for j in m or ():
            keys.append(lk[i])
            lo.append(lv[i])
            ro.append(rv[j])
            ma.append(True)
        if not m and how == "left":
            keys.append(lk[i])
            lo.append(lv[i])
            ro.append(0)
            ma.append(False)
    if how in ("semi", "anti"):
        return keys, lo, None, None
    return keys, lo, ro, (ma if how == "left" else None)


def job_lists(res):
    """JoinResult -> the tuple shape of job_oracle."""
    return (to_u64(res.keys), bits(res.lvals), bits(res.rvals),
            res.matched.cpu().tolist() if res.matched is not None else None)
