"""Shared pieces of the window tests: a pure-Python oracle that walks the rows
one at a time and shares no code with the ops (the order key and the bit
helpers are those written out in group_common), the segment layouts and the
value families.

A layout is a list of segment lengths over grouped rows; a value family
fills the value column.  Values are compared through their int64 bit
patterns or their order keys, never through float ==.
"""

import functools
import random

import torch

import group_common as gc

M64 = gc.M64
SIZES = lambda S: (0, 1, 2, 63, 64, 65, S - 1, S, S + 1, 3 * S + 17)
OPS = ("sum", "min", "max")
# family -> the ops it is scanned under
FAMILIES = {"i64_full": OPS, "f64_int": OPS, "f64_special": ("min", "max")}


# ---- layouts: lists of segment lengths -------------------------------------

@functools.lru_cache(maxsize=None)
def layouts(S):
    """name -> tuple of segment lengths; S = ops.seg_scan_caps()[0] rows per
    tile.  The smallest shapes at which a carry can go wrong."""
    out = {"n0": ()}
    for n in SIZES(S)[1:]:
        out[f"singles_{n}"] = (1,) * n
        out[f"one_{n}"] = (n,)          # the carry passes through every tile
        out[f"pairs_{n}"] = (2,) * (n // 2) + (1,) * (n % 2)
    out["head_at_S"] = (S, S // 2)      # the carry must be dropped
    out["head_at_S_minus_1"] = (S - 1, S // 2 + 1)
    out["middle_tile_headless"] = (S // 2, 2 * S, S // 2)
    rng = random.Random(17)
    out["random"] = tuple(rng.randrange(1, 3 * S + 1) for _ in range(7))
    return out


def second_chunk_layout(S, C):
    """(C + 1) * S rows in three long segments: the one-block carry pass
    takes a second chunk, and the last segment carries across the chunk
    boundary."""
    a = C * S // 3
    return (a + 5, a, (C + 1) * S - 2 * a - 5)


def offsets_of(lens):
    return gc.offsets_of(lens)


def heads_of(lens):
    return gc.offsets_of(lens)[:-1]


def headless_tiles(lens, S):
    """The tiles of S rows that hold no segment head."""
    n = sum(lens)
    with_head = {h // S for h in heads_of(lens)}
    return [t for t in range((n + S - 1) // S) if t not in with_head]


def layout_keys(lens):
    """One u64 key per segment, distinct and NOT ascending: segments need
    only be grouped."""
    ks = [((s + 1) * 0x9E3779B97F4A7C15 + 12345) & M64
          for s in range(len(lens))]
    assert len(set(ks)) == len(ks)
    return gc.to_i64([k for k, n in zip(ks, lens) for _ in range(n)])


# ---- value families --------------------------------------------------------

def values(family, n, seed=3):
    rng = random.Random(seed * 7919 + n)
    if family == "i64_full":
        return gc.case_values("random_i64", n, seed)
    if family == "f64_int":
        # integer-valued, |v| <= 2^20: with n <= 2^22 every partial sum is
        # below 2^43 in magnitude and exact in any association
        return torch.tensor([float(rng.randrange(-2 ** 20, 2 ** 20 + 1))
                             for _ in range(n)], dtype=torch.float64)
    if family == "f64_special":
        return gc.case_values("f64", n, seed)
    if family == "f64_general":
        return torch.tensor([rng.uniform(-1e6, 1e6) * 10 ** rng.randrange(6)
                             for _ in range(n)], dtype=torch.float64)
    raise ValueError(family)


@functools.lru_cache(maxsize=None)
def layout_data(S, name, family):
    """(keys i64 tensor, vals tensor), built once."""
    lens = layouts(S)[name]
    return layout_keys(lens), values(family, sum(lens))


# ---- the oracle: one row at a time ------------------------------------------

def from_bits(bits, dtype):
    return gc.to_i64(bits).view(dtype)


def oracle_scan(lens, vals, op):
    """-> the running column as u64 bit patterns."""
    f64 = vals.dtype == torch.float64
    bits = gc.to_bits(vals)
    fl = vals.tolist() if f64 else None
    out = []
    i = 0
    for n in lens:
        for j in range(n):
            b = bits[i]
            if j == 0:
                acc = b
                facc = fl[i] if f64 else None
            elif op == "sum":
                if f64:
                    facc = facc + fl[i]      # left to right; exact inputs
                    acc = gc.f64_bits(facc)
                else:
                    acc = (acc + b) & M64    # wraps
            else:
                ka, kb = gc.okey(acc, f64), gc.okey(b, f64)
                if (kb < ka) if op == "min" else (kb > ka):
                    acc = b                  # ties keep the earlier row
            out.append(acc)
            i += 1
    return out


@functools.lru_cache(maxsize=None)
def expected_scan(S, name, family, op):
    _, vals = layout_data(S, name, family)
    return oracle_scan(layouts(S)[name], vals, op)


def oracle_session_flags(keys_bits, times, gap):
    """times: Python ints, ascending within each key."""
    out = []
    for i, (k, t) in enumerate(zip(keys_bits, times)):
        out.append(1 if i == 0 or keys_bits[i - 1] != k
                   or t - times[i - 1] > gap else 0)
    return out


def oracle_sessions(keys_bits, times, gap):
    """-> (session keys, session offsets)."""
    flags = oracle_session_flags(keys_bits, times, gap)
    heads = [i for i, f in enumerate(flags) if f]
    return [keys_bits[h] for h in heads], heads + [len(times)]


def oracle_perm(off, vals):
    """The stable order on (segment, order key, input row)."""
    ok = gc.okeys(vals)
    out = []
    for a, b in zip(off, off[1:]):
        out.extend(sorted(range(a, b), key=lambda i: (ok[i], i)))
    return out


# ---- WindowJob: unsorted rows ----------------------------------------------

def make_rows(seed, n, nkeys, order_f64, vals_f64, hot=0, span=50):
    """n unsorted rows over nkeys keys on both halves of the sign bit plus
    `hot` rows of one more key; the order column takes few distinct values,
    so there are ties for the value column to break."""
    rng = random.Random(seed)
    pool = [rng.randrange(1 << 64) for _ in range(nkeys)] + [0, M64]
    keys = [rng.choice(pool) for _ in range(n)] + [pool[0] ^ 1] * hot
    rng.shuffle(keys)
    m = len(keys)
    if order_f64:
        marks = [float("-inf"), -0.0, 0.0, 1.5, float("nan"), float("inf")]
        order = torch.tensor(
            [rng.choice(marks) if rng.random() < 0.2
             else float(rng.randrange(-span, span)) / 4 for _ in range(m)],
            dtype=torch.float64)
    else:
        order = torch.tensor([rng.randrange(-span, span) * 1000
                              for _ in range(m)], dtype=torch.int64)
    vals = gc.case_values("f64" if vals_f64 else "random_i64", m, seed)
    if not vals_f64:
        vals = vals >> 58   # repeated values: whole rows tie
    return gc.to_i64(keys), order, vals


def job_oracle(keys, order, vals=None, world=1, rank=0):
    """-> (u64 keys ascending, offsets, order keys of the order column,
    order keys of the values or None) of the partition of `rank`; the rows
    of a key ascend by (order key of order, order key of value)."""
    ok_o = gc.okeys(order)
    ok_v = gc.okeys(vals) if vals is not None else [0] * len(ok_o)
    groups = {}
    for k, o, v in zip(gc.to_bits(keys), ok_o, ok_v):
        groups.setdefault(k, []).append((o, v))
    uk, off, oo, vv = [], [0], [], []
    for k in sorted(groups):
        if (k * world) >> 64 != rank:
            continue
        g = sorted(groups[k])
        uk.append(k)
        oo.extend(o for o, _ in g)
        vv.extend(v for _, v in g)
        off.append(len(oo))
    return uk, off, oo, (vv if vals is not None else None)


def job_lists(res):
    return (gc.to_bits(res.keys), res.offsets.cpu().tolist(),
            gc.okeys(res.order),
            gc.okeys(res.values) if res.values is not None else None)


def oracle_job_sessions(res_lists, order_dtype_i64_values, gap):
    """Sessions of an ordered i64 time column: [(key, start, end, count)]
    and the number of sessions per key."""
    uk, off, _, _ = res_lists
    times = order_dtype_i64_values
    rows, per_key = [], []
    for k, a, b in zip(uk, off, off[1:]):
        m = 0
        for i in range(a, b):
            if i == a or times[i] - times[i - 1] > gap:
                rows.append([k, times[i], times[i], 0])
                m += 1
            rows[-1][2] = times[i]
            rows[-1][3] += 1
        per_key.append(m)
    return [tuple(r) for r in rows], per_key
