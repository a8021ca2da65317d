"""Shared pieces of the frame tests: case generators and oracles that share no
code with the ops.  Frames come from the definition (bisect on (key, order
key) tuples, or index arithmetic on segment lengths); every frame is then
aggregated on its own: math.fsum for f64 sums, integers masked to 64 bits
for i64, the first occurrence of the winning order key for min / max.  The
wide cases slice numpy arrays per row so they stay within seconds.

T, W, R below are ops.frame_caps(): rows per tile of the window bounds
kernel, rows of a window staged in LDS, rows per tile of the reduce
kernels.
"""

import bisect
import functools
import math
import random

import numpy as np
import torch

import group_common as gc

M64, SIGN = gc.M64, gc.SIGN
I64_MIN, I64_MAX = gc.I64_MIN, gc.I64_MAX
OPS = ("sum", "min", "max")
ROLLING = ("sum", "min", "max", "count", "mean")
# family -> the ops it is reduced under
FAMILIES = {"i64_full": OPS, "f64_int": OPS, "f64_special": ("min", "max")}


# ---- frames from the definition ---------------------------------------------

def oracle_range_frames(kbits, times, pre, fol):
    """kbits: u64 keys; times: Python ints (i64); rows ascending on (key,
    time).  -> (lo, hi) lists."""
    rows = [(k, t + SIGN) for k, t in zip(kbits, times)]   # the i64 order key
    assert rows == sorted(rows)
    lo, hi = [], []
    for k, o in rows:
        lo.append(bisect.bisect_left(rows, (k, max(o - pre, 0))))
        hi.append(bisect.bisect_right(rows, (k, min(o + fol, M64))))
    return lo, hi


def oracle_row_frames(off, pre, fol):
    lo, hi = [], []
    for a, b in zip(off, off[1:]):
        for i in range(a, b):
            lo.append(max(a, i - pre))
            hi.append(min(b, i + fol + 1))
    return lo, hi


# ---- aggregates, one frame at a time -----------------------------------------

def oracle_reduce(vals, lo, hi, op):
    """-> the aggregate of vals[lo[i]:hi[i]] per row as u64 bit patterns.
    f64 sums are math.fsum: exact inputs only, or compare within a bound."""
    f64 = vals.dtype == torch.float64
    bits = np.array(gc.to_bits(vals), dtype=np.uint64)
    out = []
    if op == "sum" and f64:
        fl = vals.numpy()
        for a, b in zip(lo, hi):
            out.append(gc.f64_bits(math.fsum(fl[a:b])))
    elif op == "sum":
        with np.errstate(over="ignore"):
            for a, b in zip(lo, hi):
                out.append(int(np.add.reduce(bits[a:b])) & M64)   # wraps
    else:
        ok = np.array([gc.okey(int(x), f64) for x in bits], dtype=np.uint64)
        pick = np.argmin if op == "min" else np.argmax   # first occurrence
        for a, b in zip(lo, hi):
            out.append(int(bits[a + int(pick(ok[a:b]))]))
    return out


def oracle_mean(vals, lo, hi):
    """i64 values: the wrapped sum as a signed integer, as f64, over the
    count; -> floats."""
    out = []
    for s, a, b in zip(oracle_reduce(vals, lo, hi, "sum"), lo, hi):
        if vals.dtype == torch.float64:
            out.append(gc.to_i64([s]).view(torch.float64).item() / (b - a))
        else:
            out.append(float(s - (1 << 64) if s & SIGN else s) / float(b - a))
    return out


# ---- bounds cases --------------------------------------------------------------

def _keys(lens):
    return gc.case_keys(lens)   # ascending, both halves of the sign bit


@functools.lru_cache(maxsize=None)
def bounds_cases(T, W, R):
    """name -> (u64 keys, i64 times, ((preceding, following), ...)), rows
    ascending on (key, time)."""
    big = 2 ** 63 - 1
    rng = random.Random(23)
    out = {"n0": ([], [], ((3, 2),)), "n1": ([5], [-9], ((0, 0), (big, big)))}
    n = T + 3
    out["singles"] = (_keys((1,) * n), [rng.randrange(-50, 50)
                                        for _ in range(n)], ((5, 5), (big, 0)))
    n = 3 * R + 17
    out["one_key_ticks"] = (
        [7] * n, list(range(-5, n - 5)),
        tuple((p, f) for p in (0, 1, 63, 64, T - 1, T, n, big)
              for f in (0, 1, T)))
    # a run of W + 50 equal times from row T - 100 on: it lies across the
    # tile edge at T and pushes hi of the first tile's rows beyond W rows
    run = W + 50
    times = list(range(T - 100)) + [T] * run + list(range(T + 1, T + 300))
    out["peers_over_W"] = ([M64] * len(times), times, ((0, 0), (1, 1)))
    # one key one tick apart: the window of an inner tile is T + p + f rows
    d = W - T
    out["window_W"] = ([9] * (5 * T), list(range(5 * T)),
                       ((d, 0), (d + 1, 0), (0, d), (0, d + 1),
                        (d // 2, d - d // 2), (d // 2 + 1, d - d // 2)))
    lens = tuple(rng.randrange(1, 40) for _ in range(120))
    times = []
    for m in lens:
        times.extend(sorted(rng.randrange(0, 8) for _ in range(m)))
    out["ties"] = (_keys(lens), times, ((0, 0), (1, 0), (0, 2)))
    out["saturate"] = ([SIGN | 3] * 4, [I64_MIN, -1, 0, I64_MAX],
                       ((big, big), (big, 0), (0, big), (1, 1)))
    # the key changes at rows T - 1, T and T + 1, equal times on both sides
    lens = (T - 1, 1, 1, T)
    out["key_change_at_tile_edge"] = (_keys(lens), [7] * sum(lens),
                                      ((5, 5), (0, 0), (big, big)))
    return out


@functools.lru_cache(maxsize=None)
def expected_bounds(T, W, R, name, pre, fol):
    k, t, _ = bounds_cases(T, W, R)[name]
    return oracle_range_frames(k, t, pre, fol)


# ---- reduce cases: explicit frames with lo <= i < hi --------------------------

@functools.lru_cache(maxsize=None)
def reduce_cases(R):
    """name -> (lo, hi) as tuples."""
    out = {}

    def add(name, n, f):
        fr = [f(i, n) for i in range(n)]
        assert all(0 <= a <= i < b <= n for i, (a, b) in enumerate(fr)), name
        out[name] = (tuple(a for a, _ in fr), tuple(b for _, b in fr))

    add("n1", 1, lambda i, n: (0, 1))
    add("own_row", 70, lambda i, n: (i, i + 1))
    # inside one 64-row chunk; more than one block
    add("in_chunk", R + 70, lambda i, n: (max(i // 64 * 64, i - 3),
                                          min(i // 64 * 64 + 64, i + 4, n)))
    # across chunk edges and, near row R, one tile edge
    add("cross_chunk", R + 70, lambda i, n: (max(0, i - 40), min(n, i + 41)))
    # at most R rows: one tile edge, never a whole tile between
    add("one_tile_edge", 2 * R + 9, lambda i, n: (max(0, i - (R - 1)), i + 1))
    # exactly one whole tile between for the rows behind it
    add("one_whole_tile", 3 * R + 11,
        lambda i, n: (max(0, i - R - R // 2), min(n, i + R // 2)))
    add("tile_exact_whole", R, lambda i, n: (0, n))
    add("tile_plus_one_whole", R + 1, lambda i, n: (0, n))
    # 10 tiles, the last partial.  Every eighth row reaches back over up to
    # 9 R rows, 0..7 whole tiles between from every start, and the rows of
    # the last tile start in tile 0 or 1 (8 whole tiles, or 7 from an even
    # one); the rows between them keep the oracle short
    add("nine_tiles", 9 * R + 5,
        lambda i, n: (i - (9 - i % 2) * R if i >= 9 * R else
                      max(0, i - (i // 8 % 10) * R - i % 7) if i % 8 == 0
                      else i - i % 5, min(n, i + 1 + i % 5)))
    return out


def whole_tiles(lo, hi, R):
    """(first whole tile, count) of every frame that leaves its first tile."""
    return [(a // R + 1, (b - 1) // R - a // R - 1)
            for a, b in zip(lo, hi) if a // R != (b - 1) // R]


def values(family, n, seed=3):
    rng = random.Random(seed * 7919 + n)
    if family == "i64_full":
        return gc.case_values("random_i64", n, seed)
    if family == "f64_int":
        # integer-valued, |v| <= 2^20: every partial sum of fewer than 2^22
        # rows is exact in any association
        return torch.tensor([float(rng.randrange(-2 ** 20, 2 ** 20 + 1))
                             for _ in range(n)], dtype=torch.float64)
    if family == "f64_special":
        # -0.0 / +0.0, infinities and NaNs of four payloads, each repeated
        return gc.case_values("f64", n, seed)
    if family == "f64_general":
        return torch.tensor([rng.uniform(-1e6, 1e6) * 10 ** rng.randrange(6)
                             for _ in range(n)], dtype=torch.float64)
    raise ValueError(family)


@functools.lru_cache(maxsize=None)
def reduce_data(R, name, family):
    return values(family, len(reduce_cases(R)[name][0]))


@functools.lru_cache(maxsize=None)
def expected_reduce(R, name, family, op):
    lo, hi = reduce_cases(R)[name]
    return oracle_reduce(reduce_data(R, name, family), lo, hi, op)


# ---- OrderedRows.rolling --------------------------------------------------------

def oracle_rolling(off, order, vals, op, pre, fol, unit):
    """off: offsets; order: the ordered i64 order column as Python ints (any
    list for unit="rows"); vals: the ordered value column on the host, or
    None.  -> u64 bit patterns (floats for mean, ints for count)."""
    if unit == "rows":
        lo, hi = oracle_row_frames(off, pre, fol)
    else:
        seg = [s for s, (a, b) in enumerate(zip(off, off[1:]))
               for _ in range(a, b)]
        lo, hi = oracle_range_frames(seg, order, pre, fol)
    if op == "count":
        return [b - a for a, b in zip(lo, hi)]
    if op == "mean":
        return oracle_mean(vals, lo, hi)
    return oracle_reduce(vals, lo, hi, op)


def check_rolling(res, f64_vals, i64_order):
    """All five ops and both units against the oracle, on the rows as the
    job arranged them (checked by the window tests)."""
    off = res.offsets.cpu().tolist()
    order = res.order.cpu().tolist()
    hv = res.values.cpu()
    units = [("rows", 0, 0), ("rows", 3, 0), ("rows", 2, 5),
             ("rows", 0, 2 ** 31 - 1)]
    if i64_order:
        units += [("range", 0, 0), ("range", 3000, 0), ("range", 1000, 2000),
                  ("range", 2 ** 63 - 1, 2 ** 63 - 1)]
    for unit, p, f in units:
        fr = res.frames(p, f, unit)
        for op in ROLLING:
            if f64_vals and op in ("sum", "mean"):
                continue   # NaNs and infinities: the bits of a sum are free
            want = oracle_rolling(off, order, hv, op, p, f, unit)
            got = res.rolling(op, p, f, unit)
            shared = res.rolling(op, frames=fr)
            assert gc.to_bits(got) == gc.to_bits(shared), (op, unit)
            if op == "count":
                assert got.dtype == torch.int64
                assert got.cpu().tolist() == want, (unit, p, f)
            elif op == "mean":
                assert got.dtype == torch.float64
                assert got.cpu().tolist() == want, (unit, p, f)
            else:
                assert got.dtype == hv.dtype
                assert gc.to_bits(got) == want, (op, unit, p, f)
