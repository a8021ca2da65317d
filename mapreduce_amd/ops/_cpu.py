"""CPU reference implementations of the HIP ops.

Test tier only: lets the distributed engine run end-to-end on CPU (gloo,
world_size > 1) in environments without a GPU, and doubles as the numerics
oracle the HIP kernels are tested against.  On a machine with a GPU these
are never silently used (ops.require_gpu_ext)."""

from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from ..utils.tuple import FNV64_OFFSET, FNV64_PRIME

_MASK64 = (1 << 64) - 1
HT_EMPTY = _MASK64
_WS = frozenset(b" \t\n\v\f\r")


def _u64(t: torch.Tensor) -> np.ndarray:
    return t.numpy().view(np.uint64)


def _from_u64(a: np.ndarray, like: Optional[torch.Tensor] = None):
    return torch.from_numpy(a.astype(np.uint64, copy=False).view(np.int64))


def tokenize_words(text: torch.Tensor):
    data = bytes(text.numpy().tobytes())
    hashes = []
    pos = []
    n = len(data)
    i = 0
    while i < n:
        if data[i] in _WS:
            i += 1
            continue
        j = i
        h = FNV64_OFFSET
        while j < n and data[j] not in _WS:
            h = ((h ^ data[j]) * FNV64_PRIME) & _MASK64
            j += 1
        hashes.append(h)
        pos.append((i << 16) | min(j - i, 0xFFFF))
        i = j
    k = _from_u64(np.array(hashes, dtype=np.uint64))
    p = _from_u64(np.array(pos, dtype=np.uint64))
    return k, p, len(hashes)


class CpuHashTable:
    def __init__(self, capacity: int, device=None, exemplar: bool = True):
        self._counts = {}
        self._exm = {} if exemplar else None

    def tokenize_count(self, text: torch.Tensor, pos_base: int,
                       nwords: torch.Tensor):
        k, p, n = tokenize_words(text)
        if pos_base:
            pu = _u64(p) + (np.uint64(pos_base) << np.uint64(16))
            p = _from_u64(pu)
        self.insert_count(k, p)
        nwords += n

    def insert_count(self, keys: torch.Tensor, pos: Optional[torch.Tensor]):
        ku = _u64(keys)
        pu = _u64(pos) if pos is not None and pos.numel() else None
        for i, k in enumerate(ku.tolist()):
            k = HT_EMPTY - 1 if k == HT_EMPTY else k
            if k not in self._counts:
                self._counts[k] = 0
                if self._exm is not None and pu is not None:
                    self._exm[k] = int(pu[i])
            self._counts[k] += 1

    def insert_sum(self, keys: torch.Tensor, vals: torch.Tensor):
        for k, v in zip(_u64(keys).tolist(), vals.tolist()):
            k = HT_EMPTY - 1 if k == HT_EMPTY else k
            self._counts[k] = self._counts.get(k, 0) + v

    def extract(self):
        ks = np.array(list(self._counts.keys()), dtype=np.uint64)
        vs = torch.tensor(list(self._counts.values()), dtype=torch.int64)
        if self._exm is not None:
            ps = np.array([self._exm.get(int(k), 0) for k in ks],
                          dtype=np.uint64)
            return _from_u64(ks), vs, _from_u64(ps)
        return _from_u64(ks), vs, torch.empty(0, dtype=torch.int64)


def sort_pairs(keys: torch.Tensor, vals: Optional[torch.Tensor], bits: int):
    ku = _u64(keys)
    order = np.argsort(ku, kind="stable")
    sk = _from_u64(ku[order])
    if vals is None:
        return sk, None
    return sk, vals[torch.from_numpy(order.astype(np.int64))]


def reduce_by_key_sorted(keys, vals, aux, op="sum"):
    ku = _u64(keys)
    ukeys, idx = np.unique(ku, return_index=True)
    if op == "min":
        # fmin/fmax (NaN-ignoring) to match the GPU tier's atomicMin/Max
        # scatter, which never lets a NaN displace an ordered value
        uv = torch.from_numpy(np.fmin.reduceat(vals.numpy(), idx))
    elif op == "max":
        uv = torch.from_numpy(np.fmax.reduceat(vals.numpy(), idx))
    elif vals is None:
        sums = np.add.reduceat(np.ones(len(ku), dtype=np.int64), idx)
        uv = torch.from_numpy(sums)
    else:
        uv = torch.from_numpy(np.add.reduceat(vals.numpy(), idx))
    ua = None
    if aux is not None:
        ua = _from_u64(_u64(aux)[idx])
    return _from_u64(ukeys), uv, ua, len(ukeys)


def segment_boundaries(keys):
    ku = _u64(keys)
    if len(ku) == 0:
        return torch.empty(0, dtype=torch.int64), 0
    flags = np.ones(len(ku), dtype=np.int64)
    flags[1:] = ku[1:] != ku[:-1]
    seg = np.cumsum(flags)
    return torch.from_numpy(seg), int(seg[-1])


def partition_counts(keys: torch.Tensor, nparts: int) -> torch.Tensor:
    ku = _u64(keys)
    out = np.zeros(nparts, dtype=np.int64)
    for k in ku.tolist():
        out[(k * nparts) >> 64] += 1
    return torch.from_numpy(out)


def _strings(text: torch.Tensor, pos: torch.Tensor):
    data = bytes(text.contiguous().numpy().tobytes())
    return [data[p >> 16:(p >> 16) + (p & 0xFFFF)]
            for p in _u64(pos.contiguous()).tolist()]


def lex_order(text: torch.Tensor, pos: torch.Tensor) -> torch.Tensor:
    words = _strings(text, pos)
    order = sorted(range(len(words)), key=words.__getitem__)  # stable
    return torch.tensor(order, dtype=torch.int64)


def lex_lower_bound(text: torch.Tensor, pos: torch.Tensor,
                    perm: torch.Tensor, queries) -> torch.Tensor:
    import bisect
    words = _strings(text, pos)
    ordered = [words[j] for j in perm.tolist()]
    return torch.tensor([bisect.bisect_left(ordered, bytes(q))
                         for q in queries], dtype=torch.int64)


def extract_words(text: torch.Tensor, pos: torch.Tensor):
    data = bytes(text.numpy().tobytes())
    pu = _u64(pos).tolist()
    lens = []
    chunks = []
    for p in pu:
        start, ln = p >> 16, p & 0xFFFF
        lens.append(ln)
        chunks.append(data[start:start + ln])
    blob = b"".join(chunks)
    return (torch.tensor(lens, dtype=torch.int64),
            torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy())
            if blob else torch.empty(0, dtype=torch.uint8))


def postings_search(keys, doc_offsets, docs, tf, weights, qkeys, qoff,
                    k: int, mode: int):
    """NumPy form of the postings_search kernel (same outputs, bit for
    bit): per query, AND/OR of the terms' doc lists, score = sum of
    tf * weight over the terms present (wrapping i64), best k by score
    descending then doc ascending.  mode: 0 = AND, 1 = OR."""
    ku = _u64(keys.contiguous())
    offs = doc_offsets.contiguous().numpy()
    dn = docs.contiguous().numpy()
    tn = tf.contiguous().numpy()
    wn = weights.contiguous().numpy() if weights.numel() else None
    qk = _u64(qkeys.contiguous())
    qo = qoff.contiguous().numpy()
    nq = len(qo) - 1
    out_docs = np.full((nq, k), -1, dtype=np.int64)
    out_scores = np.zeros((nq, k), dtype=np.int64)
    out_n = np.zeros(nq, dtype=np.int64)
    out_hits = np.zeros(nq, dtype=np.int64)
    for q in range(nq):
        lists = []  # per term (docs, tf * weight); unknown term = empty
        for h in qk[qo[q]:qo[q + 1]]:
            r = int(np.searchsorted(ku, h))
            if r < len(ku) and ku[r] == h:
                a, b = int(offs[r]), int(offs[r + 1])
                w = np.int64(wn[r] if wn is not None else 1)
                lists.append((dn[a:b], tn[a:b] * w))
            else:
                lists.append((dn[:0], tn[:0]))
        if not lists:
            continue
        if mode == 0:
            lens = [len(d) for d, _ in lists]
            cand = lists[lens.index(min(lens))][0]
        else:
            cand = np.unique(np.concatenate([d for d, _ in lists]))
        keep = np.ones(len(cand), dtype=bool)
        score = np.zeros(len(cand), dtype=np.int64)
        for d, s in lists:
            if len(d) == 0:
                found = np.zeros(len(cand), dtype=bool)
            else:
                p = np.minimum(np.searchsorted(d, cand), len(d) - 1)
                found = d[p] == cand
                score = score + np.where(found, s[p], 0)
            if mode == 0:
                keep &= found
        cand, score = cand[keep], score[keep]
        # score descending (~s = -s - 1: no overflow), doc ascending on ties
        order = np.lexsort((cand, ~score))
        n = min(k, len(cand))
        out_hits[q] = len(cand)
        out_n[q] = n
        out_docs[q, :n] = cand[order[:n]]
        out_scores[q, :n] = score[order[:n]]
    return (torch.from_numpy(out_docs), torch.from_numpy(out_scores),
            torch.from_numpy(out_n), torch.from_numpy(out_hits))


def token_ordinals(text: torch.Tensor, pos: torch.Tensor,
                   starts: torch.Tensor):
    """NumPy form of the token_ordinals kernels (same outputs): per
    occurrence pos = off << 16 | len, doc = index of the last starts[]
    entry <= off (-1 if none) and ord = word starts in [starts[doc], off),
    a word start being a non-whitespace byte at offset 0 or after a
    whitespace byte.  -> (doc i64[n], ord i32[n])."""
    data = np.frombuffer(bytes(text.contiguous().numpy().tobytes()),
                         dtype=np.uint8)
    n = len(data)
    ws = (data == 32) | ((data >= 9) & (data <= 13))
    prev_ws = np.ones(n, dtype=bool)
    prev_ws[1:] = ws[:-1]
    before = np.zeros(n + 1, dtype=np.int64)  # before[x] = starts at < x
    np.cumsum(~ws & prev_ws, out=before[1:])
    off = (_u64(pos.contiguous()) >> np.uint64(16)).astype(np.int64)
    sn = starts.contiguous().numpy()
    doc = np.searchsorted(sn, off, side="right") - 1
    at = np.clip(sn[np.maximum(doc, 0)], 0, n)
    ordn = before[np.clip(off, 0, n)] - before[at]
    return (torch.from_numpy(doc.astype(np.int64)),
            torch.from_numpy(ordn.astype(np.int32)))


def postings_phrase(keys, doc_offsets, docs, tf, pos_offsets, positions,
                    qkeys, qoff, k: int):
    """NumPy form of the postings_phrase kernel (same outputs, bit for
    bit): per query of ordered terms h_0..h_{T-1} (duplicates kept), the
    documents holding every term with some s >= 0 such that s + i is a
    position of h_i for all i; score = the number of such s; best k by
    score descending then doc ascending."""
    ku = _u64(keys.contiguous())
    offs = doc_offsets.contiguous().numpy()
    dn = docs.contiguous().numpy()
    tn = tf.contiguous().numpy()
    po = pos_offsets.contiguous().numpy()
    pn = positions.contiguous().numpy().astype(np.int64)
    qk = _u64(qkeys.contiguous())
    qo = qoff.contiguous().numpy()
    nq = len(qo) - 1
    out_docs = np.full((nq, k), -1, dtype=np.int64)
    out_scores = np.zeros((nq, k), dtype=np.int64)
    out_n = np.zeros(nq, dtype=np.int64)
    out_hits = np.zeros(nq, dtype=np.int64)
    for q in range(nq):
        rows = []  # per term (first posting, end posting); unknown = empty
        for h in qk[qo[q]:qo[q + 1]]:
            r = int(np.searchsorted(ku, h))
            if r < len(ku) and ku[r] == h:
                rows.append((int(offs[r]), int(offs[r + 1])))
            else:
                rows.append((0, 0))
        if not rows:
            continue
        lens = [b - a for a, b in rows]
        drv = lens.index(min(lens))
        cand = dn[rows[drv][0]:rows[drv][1]]
        keep = np.ones(len(cand), dtype=bool)
        where = []  # per term: posting index of each candidate doc
        for a, b in rows:
            d = dn[a:b]
            if len(d) == 0:
                keep[:] = False
                where.append(np.zeros(len(cand), dtype=np.int64))
                continue
            p = np.minimum(np.searchsorted(d, cand), len(d) - 1)
            keep &= d[p] == cand
            where.append(a + p)
        found, score = [], []
        for c in np.flatnonzero(keep):
            j = int(where[drv][c])
            s = pn[po[j]:po[j] + tn[j]] - drv
            s = s[s >= 0]
            for i, w in enumerate(where):
                if i == drv or len(s) == 0:
                    continue
                j = int(w[c])
                s = s[np.isin(s + i, pn[po[j]:po[j] + tn[j]])]
            if len(s):
                found.append(cand[c])
                score.append(len(s))
        found = np.array(found, dtype=np.int64)
        score = np.array(score, dtype=np.int64)
        order = np.lexsort((found, ~score))
        n = min(k, len(found))
        out_hits[q] = len(found)
        out_n[q] = n
        out_docs[q, :n] = found[order[:n]]
        out_scores[q, :n] = score[order[:n]]
    return (torch.from_numpy(out_docs), torch.from_numpy(out_scores),
            torch.from_numpy(out_n), torch.from_numpy(out_hits))


def join_bounds(lkeys: torch.Tensor, rkeys: torch.Tensor):
    """-> (lo i64[nl], cnt i64[nl]): the start and the length of each left
    key's run of equal right keys, both columns sorted in u64 bit order."""
    if lkeys.dtype != torch.int64 or rkeys.dtype != torch.int64:
        raise TypeError("join: key columns must be int64")
    lk = _u64(lkeys.contiguous())
    rk = _u64(rkeys.contiguous())
    lo = np.searchsorted(rk, lk, side="left").astype(np.int64)
    cnt = np.searchsorted(rk, lk, side="right").astype(np.int64) - lo
    return torch.from_numpy(lo), torch.from_numpy(cnt)


def join_sorted(lkeys: torch.Tensor, rkeys: torch.Tensor, how: str,
                max_rows: Optional[int] = None, bounds=None):
    """NumPy form of ops.join_sorted (same outputs, row for row):
    np.searchsorted gives each left key its run of equal right keys,
    np.repeat and range arithmetic expand the runs."""
    lo, cnt = bounds if bounds is not None else join_bounds(lkeys, rkeys)
    lo, cnt = lo.numpy(), cnt.numpy()
    if how == "semi":
        return torch.from_numpy(np.flatnonzero(cnt > 0).astype(np.int64))
    if how == "anti":
        return torch.from_numpy(np.flatnonzero(cnt == 0).astype(np.int64))
    per = cnt if how == "inner" else np.maximum(cnt, 1)
    total = int(per.sum())
    if max_rows is not None and total > max_rows:
        from . import JoinTooLarge
        raise JoinTooLarge(total, max_rows)
    li = np.repeat(np.arange(len(cnt), dtype=np.int64), per)
    off = np.cumsum(per) - per
    ri = lo[li] + (np.arange(total, dtype=np.int64) - off[li])
    ri[cnt[li] == 0] = -1
    return torch.from_numpy(li), torch.from_numpy(ri)


# ---- per-key order statistics ---------------------------------------------

_SIGN = np.uint64(1 << 63)
_ONES = np.uint64(_MASK64)


def group_order_keys(vals: torch.Tensor) -> np.ndarray:
    """u64 order key of each i64 / f64 value: i64 bits ^ 2^63; f64 the
    sign-flip transform with -0.0 keyed as +0.0 and every NaN keyed above
    +inf (all ones)."""
    if vals.dtype == torch.int64:
        return _u64(vals.contiguous()) ^ _SIGN
    if vals.dtype != torch.float64:
        raise TypeError(f"vals must be int64 or float64, got {vals.dtype}")
    b = _u64(vals.contiguous().view(torch.int64)).copy()
    b[(b << np.uint64(1)) == 0] = 0
    nan = (b & ~_SIGN) > np.uint64(0x7FF0000000000000)
    ok = b ^ np.where((b & _SIGN) != 0, _ONES, _SIGN)
    ok[nan] = _ONES
    return ok


def group_by_key_sorted(keys: torch.Tensor):
    ku = _u64(keys.contiguous())
    n = len(ku)
    heads = np.flatnonzero(np.concatenate(
        [np.ones(min(n, 1), dtype=bool), ku[1:] != ku[:-1]]))
    offsets = np.concatenate([heads, [n]]).astype(np.int64)
    return _from_u64(ku[heads]), torch.from_numpy(offsets)


def sort_values_in_groups(keys: torch.Tensor, vals: torch.Tensor,
                          return_perm: bool = False):
    """np.lexsort (stable) on (key, order key): equal values keep their
    input order, as on the device."""
    order = np.lexsort((group_order_keys(vals), _u64(keys.contiguous())))
    perm = torch.from_numpy(order.astype(np.int64))
    return (vals[perm], perm) if return_perm else vals[perm]


def group_pick(offsets: torch.Tensor, vals: torch.Tensor, specs):
    off = offsets.numpy()
    start, length = off[:-1], off[1:] - off[:-1]
    out = torch.zeros((len(start), len(specs)), dtype=vals.dtype)
    for q, (num, den, higher) in enumerate(specs):
        idx = (num * (length - 1) + (den - 1 if higher else 0)) // den
        ok = length > 0
        out[torch.from_numpy(ok), q] = vals[torch.from_numpy(
            (start + idx)[ok])]
    return out


def group_distinct_flags(keys: torch.Tensor, vals: torch.Tensor):
    ku = _u64(keys.contiguous())
    ok = group_order_keys(vals)
    flags = np.ones(len(ku), dtype=np.int64)
    flags[1:] = (ku[1:] != ku[:-1]) | (ok[1:] != ok[:-1])
    return torch.from_numpy(flags)


# ---- per-key running aggregates and sessions -------------------------------

def scan_by_key_sorted(keys: torch.Tensor, vals: torch.Tensor, op: str):
    """Inclusive scan within runs of equal keys, one run at a time: sums
    left to right (i64 wrapping); min / max by order key, the earlier row's
    bits kept among equal order keys."""
    ku = _u64(keys.contiguous())
    n = len(ku)
    v = vals.contiguous()
    out = torch.empty_like(v)
    if n == 0:
        return out
    heads = np.flatnonzero(np.concatenate([[True], ku[1:] != ku[:-1]]))
    ends = np.concatenate([heads[1:], [n]])
    if op == "sum":
        src = v.numpy() if v.dtype == torch.float64 else _u64(v)
        dst = out.numpy() if v.dtype == torch.float64 else _u64(out)
        with np.errstate(all="ignore"):
            for a, b in zip(heads.tolist(), ends.tolist()):
                np.cumsum(src[a:b], out=dst[a:b])
        return out
    ok = group_order_keys(v)
    bits = _u64(v.view(torch.int64))
    dst = _u64(out.view(torch.int64))
    for a, b in zip(heads.tolist(), ends.tolist()):
        g = ok[a:b]
        best = (np.minimum if op == "min" else np.maximum).accumulate(g)
        new = np.ones(b - a, dtype=bool)  # a strictly better row
        new[1:] = g[1:] < best[:-1] if op == "min" else g[1:] > best[:-1]
        src = np.maximum.accumulate(np.where(new, np.arange(b - a), 0))
        dst[a:b] = bits[a:b][src]
    return out


def session_flags(keys: torch.Tensor, times: torch.Tensor, gap: int):
    ku = _u64(keys.contiguous())
    ok = group_order_keys(times)
    flags = np.ones(len(ku), dtype=np.int64)
    flags[1:] = (ku[1:] != ku[:-1]) | ((ok[1:] - ok[:-1]) > np.uint64(gap))
    return torch.from_numpy(flags)


# ---- as-of join ------------------------------------------------------------

def asof_sorted(lkeys: torch.Tensor, ltimes: torch.Tensor,
                rkeys: torch.Tensor, rtimes: torch.Tensor, direction: str,
                tolerance: Optional[int], allow_exact: bool):
    """NumPy form of ops.asof_sorted (same output, row for row).  The
    (key, order key) pairs of both sides are ranked together (np.lexsort,
    equal pairs sharing a rank), so one np.searchsorted of the left ranks in
    the right ones, per side, gives P and Q; the candidates are then checked
    column-wise."""
    lk, rk = _u64(lkeys.contiguous()), _u64(rkeys.contiguous())
    lo, ro = group_order_keys(ltimes), group_order_keys(rtimes)
    nl, nr = len(lk), len(rk)
    out = np.full(nl, -1, dtype=np.int64)
    if nl == 0 or nr == 0:
        return torch.from_numpy(out)
    k, o = np.concatenate([lk, rk]), np.concatenate([lo, ro])
    order = np.lexsort((o, k))
    sk, so = k[order], o[order]
    step = np.ones(nl + nr, dtype=np.int64)
    step[1:] = (sk[1:] != sk[:-1]) | (so[1:] != so[:-1])
    rank = np.empty(nl + nr, dtype=np.int64)
    rank[order] = np.cumsum(step)
    p = np.searchsorted(rank[nl:], rank[:nl], side="left")
    q = np.searchsorted(rank[nl:], rank[:nl], side="right")

    def check(c, back):
        ok = (c >= 0) & (c < nr)
        cc = np.clip(c, 0, nr - 1)
        ok &= rk[cc] == lk
        dist = lo - ro[cc] if back else ro[cc] - lo  # u64; read where ok
        if tolerance is not None:
            ok &= dist <= np.uint64(tolerance)
        return ok, dist

    cb = (q if allow_exact else p) - 1
    cf = p if allow_exact else q
    if direction == "backward":
        ok, _ = check(cb, True)
        out[ok] = cb[ok]
    elif direction == "forward":
        ok, _ = check(cf, False)
        out[ok] = cf[ok]
    else:
        vb, db = check(cb, True)
        vf, df = check(cf, False)
        out[vf] = cf[vf]
        back = vb & (~vf | (db <= df))
        out[back] = cb[back]
    return torch.from_numpy(out)


# ---- per-key rolling aggregates --------------------------------------------

def frame_bounds(keys: torch.Tensor, times: torch.Tensor, preceding: int,
                 following: int):
    """Range frames from the definition: within each run of equal keys the
    order keys ascend, so np.searchsorted of the two saturated ends, left
    for lo and right for hi, gives the frame."""
    ku = _u64(keys.contiguous())
    ok = group_order_keys(times)
    n = len(ku)
    lo = np.empty(n, dtype=np.int64)
    hi = np.empty(n, dtype=np.int64)
    if n:
        pre, fol = np.uint64(preceding), np.uint64(following)
        tlo = np.where(ok >= pre, ok - pre, np.uint64(0))
        thi = ok + fol
        thi[thi < ok] = _ONES
        heads = np.flatnonzero(np.concatenate([[True], ku[1:] != ku[:-1]]))
        ends = np.concatenate([heads[1:], [n]])
        for a, b in zip(heads.tolist(), ends.tolist()):
            lo[a:b] = a + np.searchsorted(ok[a:b], tlo[a:b], side="left")
            hi[a:b] = a + np.searchsorted(ok[a:b], thi[a:b], side="right")
    return torch.from_numpy(lo), torch.from_numpy(hi)


def frame_reduce(vals: torch.Tensor, lo: torch.Tensor, hi: torch.Tensor,
                 op: str):
    """Every frame aggregated on its own, lo clamped to [0, i] and hi to
    [i + 1, n] first: i64 sums wrap, f64 sums are math.fsum (non-finite
    frames by np.sum, which gives the IEEE inf / NaN), min / max take the
    first row of the frame with the winning order key."""
    import math
    v = vals.contiguous()
    n = v.numel()
    out = torch.empty_like(v)
    if n == 0:
        return out
    i = np.arange(n, dtype=np.int64)
    l = np.clip(lo.numpy(), 0, i).tolist()
    h = np.clip(hi.numpy(), i + 1, n).tolist()
    if op == "sum" and v.dtype == torch.float64:
        src, dst = v.numpy(), out.numpy()
        finite = np.isfinite(src)
        with np.errstate(all="ignore"):
            for r in range(n):
                w = src[l[r]:h[r]]
                dst[r] = (math.fsum(w) if finite[l[r]:h[r]].all()
                          else np.sum(w))
        return out
    if op == "sum":
        src, dst = _u64(v), _u64(out)
        run = np.concatenate([[np.uint64(0)], np.cumsum(src)])  # mod 2^64
        dst[:] = run[h] - run[l]
        return out
    ok = group_order_keys(v)
    bits = _u64(v.view(torch.int64))
    dst = _u64(out.view(torch.int64))
    pick = np.argmin if op == "min" else np.argmax  # first occurrence
    for r in range(n):
        dst[r] = bits[l[r] + int(pick(ok[l[r]:h[r]]))]
    return out


_GRAPH_IDENTITY = {"sum": 0, "min": np.iinfo(np.int64).max,
                   "max": np.iinfo(np.int64).min}


def graph_propagate(offsets: torch.Tensor, src: torch.Tensor,
                    x: torch.Tensor, op: str):
    """Every row aggregated on its own over its in-edges: i64 sums wrap,
    f64 sums are math.fsum (rows holding a non-finite value by np.sum, which
    gives the IEEE inf / NaN), min / max are the signed i64 ones.  A src
    outside [0, n) contributes the identity; offsets are clamped to [0, m]
    and a row's end to its start, so every answer is defined."""
    import math
    xv = x.contiguous()
    n, m = xv.numel(), src.numel()
    f64 = xv.dtype == torch.float64
    ident = 0.0 if f64 else _GRAPH_IDENTITY[op]
    out = torch.full((n,), ident, dtype=xv.dtype)
    if n == 0 or m == 0:
        return out
    off = np.clip(offsets.numpy(), 0, m)
    lo, hi = off[:-1], np.maximum(off[1:], off[:-1])
    s = src.numpy().astype(np.int64)
    ok = (s >= 0) & (s < n)
    g = np.where(ok, xv.numpy()[np.where(ok, s, 0)],
                 np.asarray(ident, dtype=xv.numpy().dtype))
    rows = np.nonzero(hi > lo)[0]
    dst = out.numpy()
    if f64:
        finite = np.isfinite(g)
        with np.errstate(all="ignore"):
            for r in rows.tolist():
                w = g[lo[r]:hi[r]]
                dst[r] = (math.fsum(w) if finite[lo[r]:hi[r]].all()
                          else np.sum(w))
        return out
    if op == "sum":
        run = np.concatenate([[np.uint64(0)],
                              np.cumsum(g.view(np.uint64))])  # mod 2^64
        dst.view(np.uint64)[rows] = run[hi[rows]] - run[lo[rows]]
        return out
    pick = np.min if op == "min" else np.max
    for r in rows.tolist():
        dst[r] = pick(g[lo[r]:hi[r]])
    return out


def pagerank_update(sums: torch.Tensor, old: torch.Tensor,
                    inv_out: torch.Tensor, damping: float,
                    dangling: torch.Tensor):
    """-> (new, contrib, partials f64[1, 2]) in plain torch."""
    n = sums.numel()
    new = (1.0 - damping) / max(n, 1) + damping * (sums + dangling / max(n, 1))
    contrib = new * inv_out
    partials = torch.stack([(new - old).abs().sum(),
                            new[inv_out == 0].sum()]).reshape(1, 2)
    return new, contrib, partials
