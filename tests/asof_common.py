"""Shared pieces of the as-of join tests: a brute-force oracle that shares no
code with the ops (for each left row, a scan over ALL right rows, straight
from the definition of P and Q), the case generators, and the bait-flanked
input slices.

Keys are Python ints in [0, 2^64) here and i64 bit patterns in tensors;
times are Python ints (i64 cases) or floats (f64 cases).

The definition (ops.asof_sorted): with < on (key, okey(time)) pairs
lexicographic, P = the number of right rows < the left row, Q = the number
<= it; the backward candidate is Q - 1 (P - 1 strict), the forward one P (Q
strict); a candidate c is valid iff 0 <= c < nr, rk[c] == k and, with a
tolerance, the distance of the order keys is <= tol; nearest takes the valid
candidate at the smaller distance, the backward one on a tie.
"""

import functools
import random
import struct
from typing import NamedTuple

import numpy as np
import torch

M64 = (1 << 64) - 1
SIGN = 1 << 63
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
SIGN_KEYS = (0, 1, SIGN - 1, SIGN, M64)
DIRECTIONS = ("backward", "forward", "nearest")
TOL_MID = 7
TOLS = (None, 0, TOL_MID)
TOLS_EXTREME = (None, 0, 1, I64_MAX)
NAN = float("nan")
INF = float("inf")


class Case(NamedTuple):
    lk: tuple
    lt: tuple
    rk: tuple
    rt: tuple
    f64: bool
    tols: tuple


def f64_bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def okey(t, f64: bool) -> int:
    """The u64 order key of a time, from the wording of the contract: i64
    bits ^ 2^63; f64 -0.0 equals +0.0 and every NaN is one value above
    +inf."""
    if not f64:
        return t + SIGN
    if t != t:
        return M64
    if t == 0:
        return SIGN
    b = f64_bits(t)
    return b ^ M64 if b >> 63 else b | SIGN


def to_i64(keys):
    """u64 ints -> i64 tensor of the same bit patterns."""
    return torch.from_numpy(
        np.array(list(keys), dtype=np.uint64).view(np.int64).copy())


def to_u64(t):
    """i64 tensor -> list of u64 ints."""
    return t.cpu().contiguous().numpy().view(np.uint64).tolist()


def times_tensor(ts, f64: bool):
    return torch.tensor(list(ts), dtype=torch.float64 if f64 else torch.int64)


def bounds(lk, lo, rk, ro):
    """(P, Q) of every left row: one scan over all right rows per left
    row.  lk, rk u64 ints; lo, ro the order keys of the times."""
    rka = np.array(rk, dtype=np.uint64)
    roa = np.array(ro, dtype=np.uint64)
    P, Q = [], []
    for k, o in zip(lk, lo):
        k, o = np.uint64(k), np.uint64(o)
        same = rka == k
        below = rka < k
        P.append(int(np.count_nonzero(below | (same & (roa < o)))))
        Q.append(int(np.count_nonzero(below | (same & (roa <= o)))))
    return P, Q


def pick(lk, lo, rk, ro, P, Q, direction, exact, tol):
    """ri of every left row from its P and Q (Python ints throughout)."""
    nr = len(rk)
    out = []
    for i in range(len(lk)):
        def valid(c):
            return (0 <= c < nr and rk[c] == lk[i]
                    and (tol is None or abs(ro[c] - lo[i]) <= tol))
        cb = (Q[i] if exact else P[i]) - 1
        cf = P[i] if exact else Q[i]
        vb = direction != "forward" and valid(cb)
        vf = direction != "backward" and valid(cf)
        if vb and vf:
            out.append(cb if lo[i] - ro[cb] <= ro[cf] - lo[i] else cf)
        else:
            out.append(cb if vb else cf if vf else -1)
    return out


def _rel(rows, f64=False):
    """[(key, time)] -> (keys, times) sorted on (key, okey(time))."""
    rows = sorted(rows, key=lambda r: (r[0], okey(r[1], f64)))
    return tuple(r[0] for r in rows), tuple(r[1] for r in rows)


def _case(left, right, f64=False, tols=TOLS):
    if f64:
        tols = (None,)
    return Case(*_rel(left, f64), *_rel(right, f64), f64, tols)


# the row counts every side must see; filled in with the tile size T
def sizes(T):
    return [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17]


def _dup_rows(rng, n, pool):
    # times from a range that grows slowly with n: duplicates of (key, time)
    # at every size, and gaps that the mid tolerance both spans and misses
    span = 3 * (n // 40 + 4)
    return [(rng.choice(pool), rng.randrange(-span, span)) for _ in range(n)]


def _window_case(T, nwin, tail):
    """One key.  The first T left rows (tile 0) reach exactly nwin right
    rows: their first time is the first right time (P == 0) and their last
    one is placed so that Q + 1, clipped to nr, is nwin.  tail > 0 puts that
    many more right rows, and a second tile of left rows, behind them."""
    right = [(5, 10 * j) for j in range(nwin + tail)]
    last0 = 10 * (nwin - 1) if tail == 0 else 10 * (nwin - 2)
    mid = [(last0 * j // (T - 1)) + (3 if j % 4 == 1 else 0)
           for j in range(1, T - 1)]
    left = [(5, 0)] + [(5, min(t, last0)) for t in mid] + [(5, last0)]
    if tail:
        top = 10 * (nwin + tail)
        left += [(5, last0 + (top + 15 - last0) * j // 39) for j in range(40)]
    return _case(left, right)


@functools.lru_cache(maxsize=None)
def cases(T, W):
    """name -> Case.  T, W = ops.asof_caps()."""
    rng = random.Random(20241021)
    out = {}
    pool = sorted(rng.randrange(1 << 64) for _ in range(14)) + [0, M64]
    sz = sizes(T)
    # a subset of the size product: every value on each side, 0 x n, n x 0
    pairs = [(n, sz[(i + 4) % len(sz)]) for i, n in enumerate(sz)]
    pairs += [(0, 0), (0, T + 1), (T + 1, 0), (3 * T + 17, 3 * T + 17)]
    for nl, nr in pairs:
        out[f"dup_{nl}x{nr}"] = _case(_dup_rows(rng, nl, pool),
                                      _dup_rows(rng, nr, pool))
    # few keys, heavy duplicates of (key, time)
    out["heavy"] = _case(
        [(rng.choice((3, 4, SIGN)), rng.randrange(5)) for _ in range(500)],
        [(rng.choice((3, 4, SIGN)), rng.randrange(5)) for _ in range(400)])
    out["all_equal"] = _case([(7, 5)] * 300, [(7, 5)] * 300)
    out["disjoint"] = _case(
        [(2 * i, rng.randrange(9)) for i in range(T + 1)],
        [(2 * i + 1, rng.randrange(9)) for i in range(65)])
    rows = sorted({(rng.choice(pool), rng.randrange(-10 ** 6, 10 ** 6))
                   for _ in range(2 * T + 5)})
    out["identical"] = _case(rows, rows)
    # one tile of left rows over a window of exactly W right rows, and of
    # W + 1; then the same with a second tile behind it
    for extra in (0, 1):
        out[f"window_{W + extra}"] = _window_case(T, W + extra, 0)
        out[f"window_{W + extra}_tiles"] = _window_case(T, W + extra, 50)
    # one key with 3W + 5 right rows under three left rows: the window does
    # not fit, the tile searches global memory
    n = 3 * W + 5
    out["hot_fallback"] = _case(
        [(50, 2), (50, n), (50, 2 * n + 1)],
        [(10, 1), (20, 1)] + [(50, 2 * j) for j in range(n)]
        + [(60, 0), (70, 0)])
    # a run of equal (key, time) right rows across the end of tile 0's
    # window (Q of its last left row, + 1, takes in the run's first row
    # only); tile 1 starts on the run
    right = [(9, t) for t in range(101)] + [(9, 110)] * 50 + [(9, 120),
                                                              (9, 130)]
    left = [(9, 100 * j // (T - 1)) for j in range(T)]
    left += [(9, 110)] * 3 + [(9, 115), (9, 125), (9, 140)]
    out["run_across_window_end"] = _case(left, right)
    # keys across the sign bit
    out["sign_keys"] = _case(
        [(k, t) for k in SIGN_KEYS for t in (-4, 0, 3, 3, 9)],
        [(k, t) for k in SIGN_KEYS[1:] + (SIGN + 1,) for t in (-5, 0, 3, 3,
                                                               8)])
    # extreme times on both sides
    ext = (I64_MIN, -1, 0, I64_MAX)
    out["extreme_times"] = _case(
        [(k, t) for k in (1, SIGN) for t in ext + (I64_MIN + 1, I64_MAX - 1)],
        [(1, t) for t in ext] + [(SIGN, I64_MIN), (SIGN, I64_MAX)],
        tols=TOLS_EXTREME)
    # spans of 2^64 - 1 and exactly 2^63 (over every tolerance) and of
    # 2^63 - 1 (the largest tolerance alone), backward and forward
    out["extreme_span"] = _case(
        [(1, I64_MAX), (2, 0), (3, -1), (4, I64_MIN), (5, -1), (6, 0)],
        [(1, I64_MIN), (2, I64_MIN), (3, I64_MIN), (4, I64_MAX),
         (5, I64_MAX), (6, I64_MAX)], tols=TOLS_EXTREME)
    # differences of exactly the mid tolerance and one more
    m = TOL_MID
    out["tol_edge"] = _case(
        [(1, 100), (2, 100), (3, 100), (4, 100), (5, 100)],
        [(1, 100 - m), (2, 100 - m - 1), (3, 100 + m), (4, 100 + m + 1),
         (5, 100 - m), (5, 100 + m)])
    # a left key whose right run is empty, between two present keys
    out["empty_run"] = _case(
        [(10, 0), (10, 100), (20, 0), (20, 5), (20, 100), (30, 0), (30, 100)],
        [(10, 1), (10, 5), (10, 9), (30, 1), (30, 5), (30, 9)])
    # f64 times: -0.0 equals +0.0, the infinities, NaN above +inf
    sp = (-INF, -1.5, -0.0, 0.0, 2.5, INF, NAN)
    out["f64_specials"] = _case(
        [(k, t) for k in (1, SIGN) for t in sp + (1.0, -2.0)],
        [(1, t) for t in sp + (0.0, -0.0, NAN)]
        + [(SIGN, t) for t in (-0.0, INF)], f64=True)
    out["f64_random"] = _case(
        [(rng.choice(pool), rng.choice(sp + (rng.uniform(-9, 9),)))
         for _ in range(T + 1)],
        [(rng.choice(pool), rng.choice(sp + (rng.uniform(-9, 9),)))
         for _ in range(777)], f64=True)
    return out


@functools.lru_cache(maxsize=None)
def _case_bounds(caps, name):
    c = cases(*caps)[name]
    lo = [okey(t, c.f64) for t in c.lt]
    ro = [okey(t, c.f64) for t in c.rt]
    return lo, ro, bounds(c.lk, lo, c.rk, ro)


def window(caps, name, tile):
    """(wlo, whi) of a tile of the windowed kernel, from the oracle."""
    c = cases(*caps)[name]
    _, _, (P, Q) = _case_bounds(caps, name)
    t0 = tile * caps[0]
    t1 = min(t0 + caps[0], len(c.lk))
    return max(P[t0] - 1, 0), min(Q[t1 - 1] + 1, len(c.rk))


@functools.lru_cache(maxsize=None)
def expected(caps, name, direction, exact, tol):
    c = cases(*caps)[name]
    lo, ro, (P, Q) = _case_bounds(caps, name)
    return pick(c.lk, lo, c.rk, ro, P, Q, direction, exact, tol)


def modes(case):
    """Every (direction, allow_exact, tolerance) the case runs under."""
    return [(d, e, t) for d in DIRECTIONS for e in (True, False)
            for t in case.tols]


def baited(case, device="cpu"):
    """-> (bufs, views): the four columns (lkeys, ltimes, rkeys, rtimes) as
    exact-size slices, one element into larger tensors, so no view is
    16-byte aligned.  The flanking rows are bait: beside the right columns
    sit the first and the last left row, beside the left columns the first
    and the last right row, so a read outside [0, n) finds a row that
    matches."""
    def flank(keys, times, fk, ft):
        z = 0.0 if case.f64 else 0
        first = (fk[0], ft[0]) if fk else (0, z)
        last = (fk[-1], ft[-1]) if fk else (0, z)
        kb = to_i64((first[0],) + tuple(keys) + (last[0],))
        tb = times_tensor((first[1],) + tuple(times) + (last[1],), case.f64)
        return kb.to(device), tb.to(device)
    lkb, ltb = flank(case.lk, case.lt, case.rk, case.rt)
    rkb, rtb = flank(case.rk, case.rt, case.lk, case.lt)
    bufs = (lkb, ltb, rkb, rtb)
    nl, nr = len(case.lk), len(case.rk)
    views = (lkb[1:1 + nl], ltb[1:1 + nl], rkb[1:1 + nr], rtb[1:1 + nr])
    return bufs, views


# ---- AsofJoinJob: unsorted relations with values --------------------------

F64_SPECIALS = (-0.0, NAN, INF, -INF, 0.0, 1.5)


def make_relation(seed, n, nkeys, tf64, vf64):
    """n rows in random order: u64 keys with duplicates on both halves of
    the sign bit, a time each from a small range (duplicates of (key, time)
    are common) and a value each."""
    rng = random.Random(seed)
    pool = [rng.randrange(1 << 64) for _ in range(nkeys)] + [0, M64]

    def col(f64, wide):
        if f64:
            return torch.tensor(
                [F64_SPECIALS[i % len(F64_SPECIALS)] if i % 7 == 0
                 else float(rng.randrange(-wide, wide)) / 2
                 for i in range(n)], dtype=torch.float64)
        return torch.tensor([rng.randrange(-wide, wide) for _ in range(n)],
                            dtype=torch.int64)
    keys = to_i64(rng.choice(pool) for _ in range(n))
    return keys, col(tf64, 12), col(vf64, 2 ** 40)


def bits(t):
    """column -> list of its int64 bit patterns."""
    return t.cpu().contiguous().view(torch.int64).tolist()


def _vals(t):
    return t.cpu().tolist()


def job_oracle(lkeys, ltimes, lvals, rkeys, rtimes, rvals, direction="backward",
               tol=None, exact=True, how="left"):
    """Rows of the as-of join of two UNSORTED relations: each side arranged
    by (key, okey(time), okey(value)), stably; one row per left row (the
    matched ones only under how="inner").  -> list of (key u64, ltime bits,
    lval bits, rtime bits, rval bits, matched); unmatched rows carry 0, 0."""
    def arrange(keys, times, vals):
        k = to_u64(keys)
        tf, vf = times.dtype == torch.float64, vals.dtype == torch.float64
        to = [okey(t, tf) for t in _vals(times)]
        vo = [okey(v, vf) for v in _vals(vals)]
        order = sorted(range(len(k)), key=lambda i: (k[i], to[i], vo[i]))
        tb, vb = bits(times), bits(vals)
        return ([k[i] for i in order], [to[i] for i in order],
                [tb[i] for i in order], [vb[i] for i in order])
    lk, lo, ltb, lvb = arrange(lkeys, ltimes, lvals)
    rk, ro, rtb, rvb = arrange(rkeys, rtimes, rvals)
    P, Q = bounds(lk, lo, rk, ro)
    ri = pick(lk, lo, rk, ro, P, Q, direction, exact, tol)
    rows = []
    for i, j in enumerate(ri):
        if j >= 0:
            rows.append((lk[i], ltb[i], lvb[i], rtb[j], rvb[j], True))
        elif how == "left":
            rows.append((lk[i], ltb[i], lvb[i], 0, 0, False))
    return rows


def job_rows(res):
    """AsofResult -> the row shape of job_oracle."""
    n = res.keys.numel()
    ma = res.matched.cpu().tolist() if res.matched is not None else [True] * n
    return list(zip(to_u64(res.keys), bits(res.ltimes), bits(res.lvals),
                    bits(res.rtimes), bits(res.rvals), ma))


def canonical(rows, tf64, lvf64, rvf64):
    """Rows with every time and value replaced by its order key: equal rows
    compare equal whatever the sign of a zero or the payload of a NaN."""
    def ok(b, f64):
        if not f64:
            return b + SIGN
        return okey(struct.unpack("<d", struct.pack("<q", b))[0], True)
    return [(k, ok(lt, tf64), ok(lv, lvf64),
             ok(rt, tf64) if m else None, ok(rv, rvf64) if m else None, m)
            for k, lt, lv, rt, rv, m in rows]


# ---- examples/asof_quotes --------------------------------------------------

def brute_quotes(left, right, direction, tol, strict, inner):
    """The example's answer from the relations themselves, every quote of
    the symbol scanned for every trade."""
    quotes = {}
    for rk, rt, rv in right:
        quotes.setdefault(rk, []).append((rt, rv))
    exp = {}
    for k, t, v in left:
        mine = quotes.get(k, ())
        back = [(rt, rv) for rt, rv in mine
                if (rt < t or (rt == t and not strict))
                and (tol is None or t - rt <= tol)]
        fwd = [(rt, rv) for rt, rv in mine
               if (rt > t or (rt == t and not strict))
               and (tol is None or rt - t <= tol)]
        b = max(back) if back and direction != "forward" else None
        f = min(fwd) if fwd and direction != "backward" else None
        if b and f:
            hit = b if t - b[0] <= f[0] - t else f
        else:
            hit = b or f
        if hit or not inner:
            exp.setdefault(k, []).append((t, v) + (hit or (None, None)))
    return exp
