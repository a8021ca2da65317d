"""High-level wrappers over the CDNA4 HIP kernels (mapreduce_amd._hip_ops).

The HIP path is mandatory on GPU: if the extension is missing on a machine
with a visible GPU we raise immediately instead of silently falling back to
eager PyTorch (the fallbacks in this package exist only for CPU-only test
environments).
"""

from __future__ import annotations

import math
import os
from typing import Optional

import torch

_ext = None
_ext_err: Optional[BaseException] = None
try:
    from mapreduce_amd import _hip_ops as _ext  # built by setup.py, in-tree
except Exception as e:  # pragma: no cover
    _ext_err = e


def have_ext() -> bool:
    return _ext is not None


# Tokenizer switches whose kernels were removed.  Setting one used to pick
# another kernel; an A/B that silently compares a build with itself is worse
# than an error, so they fail loudly.
RETIRED_SWITCHES = (
    "MR_TOKENIZE_V4", "MR_TOKENIZE_V5", "MR_TOK_BSPILL", "MR_TOK_CACHE",
    "MR_TOK_TILE", "MR_TOK_BLOCK", "MR_SPILL_CHUNK")


def check_retired_switches(environ=None) -> None:
    env = os.environ if environ is None else environ
    for name in RETIRED_SWITCHES:
        if name in env:
            raise RuntimeError(
                f"{name} is set, but it was removed together with the kernel "
                "it selected; unset it")


_switches_checked = False


def ext():
    # once per process here (ext() sits on the per-job host path, which the
    # sequential benchmark sees); require_gpu_ext() checks every time
    global _switches_checked
    if not _switches_checked:
        check_retired_switches()
        _switches_checked = True
    if _ext is None:
        raise ImportError(
            "mapreduce_amd._hip_ops is not built; run "
            "`PYTORCH_ROCM_ARCH=gfx950 python setup.py build_ext --inplace`. "
            f"(import error: {_ext_err})")
    return _ext


def require_gpu_ext() -> None:
    """Loud failure when a GPU is present but the HIP extension is not —
    GPU runs must never silently use an eager fallback."""
    check_retired_switches()
    if torch.cuda.is_available():
        ext()


def _next_pow2(n: int) -> int:
    return 1 << max(4, math.ceil(math.log2(max(n, 2))))


# ---------------------------------------------------------------------------
# tokenizer (K2/K3)
# ---------------------------------------------------------------------------


def tokenize_words(text: torch.Tensor):
    """text: uint8 tensor -> (hashes i64[n], pos i64[n], n).

    A word needs >=1 byte + separator, so capacity (len+1)//2 + 1 never
    overflows.  Synchronizes once to read back the word count.
    """
    if not text.is_cuda:
        from . import _cpu
        return _cpu.tokenize_words(text)
    cap = text.numel() // 2 + 16
    h, p, c = ext().tokenize(text, cap)
    n = int(c.item())
    assert n <= cap
    return h[:n], p[:n], n


# ---------------------------------------------------------------------------
# hash-table combiner (K5 aggregation form)
# ---------------------------------------------------------------------------


class HashTable:
    """Open-addressing (u64 key -> i64 sum) table with optional exemplar
    tracking.  Lives in HBM; sized as next_pow2(2 * expected_uniques)."""

    def __init__(self, capacity: int, device, exemplar: bool = True):
        cap = _next_pow2(2 * capacity)
        opts = dict(device=device, dtype=torch.int64)
        self.tkeys = torch.full((cap,), -1, **opts)  # -1 bits == HT_EMPTY
        self.tvals = torch.zeros((cap,), **opts)
        self.texm = torch.zeros((cap if exemplar else 0,), **opts)
        self.cap = cap

    def tokenize_count(self, text: torch.Tensor, pos_base: int,
                       nwords: torch.Tensor):
        """Fused map+combine: tokenize `text` (a split, offset pos_base in
        the rank corpus) straight into the table; nwords (i64[1] on device)
        accumulates the word count without a host sync."""
        ext().tokenize_count(text, pos_base, self.tkeys, self.tvals,
                             self.texm, nwords)

    def insert_count(self, keys: torch.Tensor, pos: Optional[torch.Tensor]):
        n = keys.numel()
        if n == 0:
            return
        p = pos if pos is not None else torch.empty(0, dtype=torch.int64,
                                                    device=keys.device)
        ext().hash_insert_count(keys, p, self.tkeys, self.tvals, self.texm, n)

    def insert_sum(self, keys: torch.Tensor, vals: torch.Tensor):
        n = keys.numel()
        if n == 0:
            return
        ext().hash_insert_sum_i64(keys, vals, self.tkeys, self.tvals, n)

    def extract(self):
        """-> (keys, vals, pos) compacted, unsorted.  One sync for count.

        Large tables use the chunked-compaction kernel (the per-wave
        shared-counter atomic serializes cross-XCD — measured 6.3 ms on a
        2^25-slot scan) and mask out its HT_EMPTY chunk padding here;
        small tables keep the padding-free path."""
        import os
        v2_min = int(os.environ.get("MR_EXTRACT_V2_MIN", 1 << 22))
        if self.cap >= v2_min:
            k, v, p, c = ext().hash_extract_v2(self.tkeys, self.tvals,
                                               self.texm)
            n = int(c.item())
            k = k[:n]
            real = k != -1
            k = k[real]
            v = v[:n][real]
            p = p[:n][real] if p.numel() else p
            return k, v, p
        k, v, p, c = ext().hash_extract(self.tkeys, self.tvals, self.texm)
        n = int(c.item())
        return k[:n], v[:n], (p[:n] if p.numel() else p)


# ---------------------------------------------------------------------------
# radix sort (K1)
# ---------------------------------------------------------------------------


def make_table(capacity: int, device, exemplar: bool = True):
    """Hash-table combiner for the given device (GPU: HIP kernels; CPU:
    test-tier dict)."""
    if torch.device(device).type == "cuda":
        return HashTable(capacity, device, exemplar)
    from ._cpu import CpuHashTable
    return CpuHashTable(capacity, device, exemplar)


_SMALL_SORT_N = 1 << 20  # below this, one stable torch.sort dispatch
                         # (rocPRIM segmented radix) beats 8 host-driven
                         # hist+scan+scatter passes on launch overhead


def sort_pairs(keys: torch.Tensor, vals: Optional[torch.Tensor] = None,
               bits: int = 64):
    """Stable sort of u64 keys (bit-pattern order) w/ payload.

    Contract: every key is below 2**bits.  Then the result is the full
    64-bit stable sort (np.argsort(kind="stable") of the u64 view) on
    every path, and the inputs are never written.  `bits` only lets the
    radix sort skip passes that cannot reorder such keys; it is not a
    mask.  For keys with bits set at or above `bits` the paths differ and
    the result is unspecified: the in-tree radix sort (and sort_idx32)
    orders by the low 8 * ceil(bits / 8) bits alone, while the torch path
    below the small-sort threshold and the CPU tier order by all 64."""
    if not keys.is_cuda:
        from . import _cpu
        return _cpu.sort_pairs(keys, vals, bits)
    import os
    thresh = int(os.environ.get("MR_SMALL_SORT_N", _SMALL_SORT_N))
    if keys.numel() < thresh:
        if os.environ.get("MR_SMALL_SORT_TORCH", "1") == "1":
            # unsigned order via sign-bit flip; stable to preserve the
            # LSD composite-sort contract (inverted index doc pass)
            sk = keys ^ (-1 << 63)
            _, perm = torch.sort(sk, stable=True)
            k = keys.index_select(0, perm)
            return (k, vals.index_select(0, perm)
                    if vals is not None else None)
    empty = torch.empty(0, dtype=torch.int64, device=keys.device)
    k, v = ext().radix_sort_pairs(keys.contiguous(),
                                  vals.contiguous() if vals is not None
                                  else empty, bits)
    return (k, v if vals is not None else None)


def sort_idx32(keys: torch.Tensor, bits: int = 64):
    """Sort u64-bit-order keys carrying a 4-byte iota payload; returns
    (sorted_keys, perm int32).  ~25% less traffic per radix pass than a
    u64 payload; gather real payloads ONCE via gather_by_u32.  GPU,
    n < 2^31, above the small-sort threshold only (callers check)."""
    return ext().radix_sort_idx32(keys.contiguous(), bits)


def gather_by_u32(vals: torch.Tensor, perm32: torch.Tensor) -> torch.Tensor:
    """out[i] = vals[perm32[i]] — one streaming pass, u32 indices."""
    return ext().gather_by_u32(vals.contiguous(), perm32)


def sort_by_key(keys: torch.Tensor, *others: torch.Tensor, bits: int = 64):
    """Sort keys; reorder any number of same-length tensors alongside.

    Large CUDA arrays ride the idx32 permutation sort: the 4-byte iota
    payload (instead of 8) cuts per-pass traffic ~25% and the payload
    columns are gathered once at the end — measured win grows with
    payload count (the inverted index carries 3)."""
    if not others:
        k, _ = sort_pairs(keys, None, bits)
        return (k,)
    import os
    thresh = int(os.environ.get("MR_SMALL_SORT_N", _SMALL_SORT_N))
    if (keys.is_cuda and keys.numel() >= thresh
            and keys.numel() < 2 ** 31
            and os.environ.get("MR_SORT_IDX32", "1") == "1"):
        k, perm32 = sort_idx32(keys, bits)
        return (k,) + tuple(gather_by_u32(t.contiguous(), perm32)
                            for t in others)
    idx = torch.arange(keys.numel(), device=keys.device, dtype=torch.int64)
    k, perm = sort_pairs(keys, idx, bits)
    return (k,) + tuple(t.index_select(0, perm) for t in others)


# ---------------------------------------------------------------------------
# segmented reduce-by-key over sorted keys (K4+K5 sorted form)
# ---------------------------------------------------------------------------


def reduce_by_key_sorted(keys: torch.Tensor,
                         vals: Optional[torch.Tensor] = None,
                         aux: Optional[torch.Tensor] = None,
                         op: str = "sum"):
    """keys sorted (u64 bit order); vals i64/f64 or None (=count 1s);
    aux: optional per-element u64 whose first value per segment is kept
    (exemplar positions).  op: "sum"/"min"/"max" (i64 or f64) — the
    canonical associative+commutative(+idempotent) reducers the
    fast-path property flags admit (job.lua:104-106).
    NaN semantics: f64 min/max IGNORES NaNs on both tiers whenever a
    segment holds at least one ordered value (GPU atomicMin/Max never
    lets a NaN displace an ordered value; the CPU oracle uses
    np.fmin/fmax to match).  An all-NaN segment is tier-dependent:
    GPU returns the init identity (+inf for min, -inf for max), CPU
    returns NaN — don't rely on it.
    Returns (ukeys, reduced, uaux?, nseg)."""
    if op not in ("sum", "min", "max"):
        raise ValueError(f"unsupported op {op!r}")
    if op != "sum" and (vals is None or
                        vals.dtype not in (torch.int64, torch.float64)):
        raise TypeError("min/max reduction needs i64 or f64 vals")
    if op != "sum" and vals.numel() != keys.numel():
        raise ValueError("min/max reduction needs one value per key")
    if not keys.is_cuda:
        from . import _cpu
        return _cpu.reduce_by_key_sorted(keys, vals, aux, op)
    n = keys.numel()
    if n == 0:
        z = torch.empty(0, dtype=torch.int64, device=keys.device)
        zv = torch.empty(0, dtype=vals.dtype if vals is not None
                         else torch.int64, device=keys.device)
        return z, zv, (z if aux is not None else None), 0
    flags = ext().head_flags(keys)
    seg = torch.cumsum(flags, 0)
    nseg = int(seg[-1].item())
    if op != "sum":
        fn = (ext().seg_reduce_i64_minmax if vals.dtype == torch.int64
              else ext().seg_reduce_f64_minmax)
        uk, uv = fn(keys, vals, seg, nseg, op == "min")
    elif vals is None or vals.dtype == torch.int64:
        v = vals if vals is not None else torch.empty(
            0, dtype=torch.int64, device=keys.device)
        uk, uv = ext().seg_reduce_i64(keys, v, seg, nseg)
    elif vals.dtype == torch.float64:
        uk, uv = ext().seg_reduce_f64(keys, vals, seg, nseg)
    else:
        raise TypeError(f"unsupported value dtype {vals.dtype}")
    ua = ext().seg_first_u64(aux, seg, nseg) if aux is not None else None
    return uk, uv, ua, nseg


def segment_boundaries(keys: torch.Tensor):
    """-> (seg i64[n] 1-based segment ids, nseg). keys sorted."""
    if not keys.is_cuda:
        from . import _cpu
        return _cpu.segment_boundaries(keys)
    flags = ext().head_flags(keys)
    seg = torch.cumsum(flags, 0)
    nseg = int(seg[-1].item()) if keys.numel() else 0
    return seg, nseg


# ---------------------------------------------------------------------------
# partitioning (K2) — send layout for the RCCL all-to-all
# ---------------------------------------------------------------------------


def partition_counts(keys: torch.Tensor, nparts: int) -> torch.Tensor:
    """Histogram of partition_of(h) = mulhi(h, nparts).  When keys are
    sorted, partitions are contiguous, so cumsum(hist) gives the slice
    offsets for all-to-all send buffers."""
    if not keys.is_cuda:
        from . import _cpu
        return _cpu.partition_counts(keys, nparts)
    return ext().partition_hist(keys, nparts)


# ---------------------------------------------------------------------------
# dictionary extraction (K7/K8)
# ---------------------------------------------------------------------------


def extract_words(text: torch.Tensor, pos: torch.Tensor):
    """-> (lens i64[n], blob u8[sum lens]): the exemplar word bytes packed
    back-to-back, for the hash -> string dictionary."""
    if not text.is_cuda:
        from . import _cpu
        return _cpu.extract_words(text, pos)
    lens = ext().pos_len(pos)
    if pos.numel() == 0:
        return lens, torch.empty(0, dtype=torch.uint8, device=text.device)
    offs = torch.cumsum(lens, 0) - lens
    total = int((offs[-1] + lens[-1]).item())
    blob = ext().gather_bytes(text, pos, offs, total)
    return lens, blob


def gather_words(text: torch.Tensor, pos: torch.Tensor, offs: torch.Tensor,
                 total: int) -> torch.Tensor:
    """The blob of extract_words for callers that already hold the
    exclusive scan `offs` of the word lengths and its `total`: one gather,
    no scan and no host sync."""
    if not text.is_cuda:
        from . import _cpu
        return _cpu.extract_words(text, pos)[1]
    if pos.numel() == 0:
        return torch.empty(0, dtype=torch.uint8, device=text.device)
    return ext().gather_bytes(text, pos, offs, int(total))


# ---------------------------------------------------------------------------
# table -> sorted, packed result (the word-count job's post-drain tail)
# ---------------------------------------------------------------------------

# caps of the extract_sorted kernels (ops/hip/extract_sorted.hip): keys one
# wave ranks in LDS (a longer bin takes the composed path), lens per block
# of the offsets scan
EXTRACT_SORTED_RANK_M = 512
EXTRACT_SORTED_SCAN_TILE = 2048


def extract_sorted_caps():
    """-> (RANK_M, SCAN_TILE): the extension's own values on a GPU machine,
    the Python constants above on the CPU tier."""
    if torch.cuda.is_available():
        return tuple(int(c) for c in ext().extract_sorted_caps())
    return EXTRACT_SORTED_RANK_M, EXTRACT_SORTED_SCAN_TILE


def _extract_sorted_composed(table):
    """extract_sorted through the general ops: extract + sort_by_key +
    pos_len + cumsum.  The oracle of the native op, its fallback, and the
    CPU tier."""
    k, v, p = table.extract()
    if p.numel():
        sk, sv, sp = sort_by_key(k, v, p)
    else:
        sk, sv = sort_by_key(k, v)
        sp = p
    if sp.numel():
        if sp.is_cuda:
            lens = ext().pos_len(sp)
        else:
            lens = sp & 0xFFFF
        offs = torch.cumsum(lens, 0) - lens
        total = int((offs[-1] + lens[-1]).item())
    else:
        lens = offs = sp
        total = 0
    return sk, sv, sp, lens, offs, total, torch.cat([sk, sv, lens])


def extract_sorted(table):
    """-> (keys, counts, pos, lens, offs, total_bytes, packed): the table's
    occupied slots in ascending u64 key order.  counts are the slots'
    values, pos their exemplars, lens = pos & 0xFFFF, offs the exclusive
    prefix sum of lens and total_bytes its end; packed is the contiguous
    i64 buffer [keys | counts | lens] that keys, counts and lens view.
    Without exemplar tracking pos, lens and offs are empty and total_bytes
    is 0.

    GPU tables below MR_EXTRACT_V2_MIN slots take the native op: a handful
    of kernels and ONE host sync (the [n, total_bytes, overflow] readback).
    A key set the rank kernel cannot hold (over EXTRACT_SORTED_RANK_M keys
    sharing their top bits), larger tables, MR_EXTRACT_SORTED=0 and the
    CPU tier compose the general ops instead, with identical results."""
    import os
    tkeys = getattr(table, "tkeys", None)
    if (tkeys is None or not tkeys.is_cuda
            or os.environ.get("MR_EXTRACT_SORTED", "1") == "0"
            or table.cap >= int(os.environ.get("MR_EXTRACT_V2_MIN",
                                               1 << 22))):
        return _extract_sorted_composed(table)
    packed, pos, offs, meta = ext().extract_sorted(table.tkeys, table.tvals,
                                                   table.texm)
    n, total, overflow = (int(x) for x in meta.tolist())
    if overflow:
        return _extract_sorted_composed(table)
    has_pos = pos.numel() > 0
    packed = packed[:(3 if has_pos else 2) * n]
    return (packed[:n], packed[n:2 * n], pos[:n],
            packed[2 * n:3 * n] if has_pos else pos[:0],
            offs[:n], total, packed)


# ---------------------------------------------------------------------------
# lexicographic order of the dictionary (sorted-result guarantee, prefix
# queries) — runs at the finalfn / serving boundary, never in the timed job
# ---------------------------------------------------------------------------

_LEX_ROUNDS = 8  # device refinement rounds (8 bytes each) before the
                 # still-tied residue is finished on the host; a bound on
                 # launches, not a tuned value (MR_LEX_ROUNDS overrides)


def _lex_host_residue(text, pos, perm, slots, seg, skip: int) -> None:
    """Finish the strings still tied after `skip` shared bytes on the host:
    pull only their tails, sort each tied segment, write the order back
    into the same slots of perm.  Python's sort is stable and bytes
    compare memcmp-then-length, which is the ordering rule."""
    idx = perm.index_select(0, slots)
    p = pos.index_select(0, idx)
    tail = (((p >> 16) + skip) << 16) | ((p & 0xFFFF) - skip)
    lens, blob = extract_words(text, tail)
    raw = bytes(blob.cpu().numpy().tobytes())
    idx_h = idx.cpu().tolist()
    seg_h = seg.cpu().tolist()
    tails = []
    off = 0
    for L in lens.cpu().tolist():
        tails.append(raw[off:off + L])
        off += L
    out = []
    a = 0
    m = len(idx_h)
    while a < m:
        b = a
        while b < m and seg_h[b] == seg_h[a]:
            b += 1
        out.extend(idx_h[j] for j in sorted(range(a, b),
                                            key=tails.__getitem__))
        a = b
    perm.index_copy_(0, slots, torch.tensor(out, dtype=torch.int64,
                                            device=perm.device))


def lex_order(text: torch.Tensor, pos: torch.Tensor) -> torch.Tensor:
    """-> perm i64[n] with string(perm[0]) <= string(perm[1]) <= ... in
    byte-string lexicographic order (memcmp over the common length, then
    the shorter first); equal strings keep ascending index order.  Strings
    are text[off : off + len] for pos = off << 16 | len; len == 0 is legal.

    MSD refinement over 8-byte big-endian chunks: a length pre-sort, one
    full sort on chunk 0, then only elements of still-tied segments are
    re-sorted by (segment, next chunk).  Zero-padded chunks cannot tell
    b"a" from b"a\\x00"; the length pre-sort plus stable sorts do (see
    NOTES.md).  One host sync per round; after MR_LEX_ROUNDS rounds
    (default 8 = 64 shared bytes) the residue finishes on the host, so
    one 64 KB token cannot force thousands of sorts."""
    if not text.is_cuda:
        from . import _cpu
        return _cpu.lex_order(text, pos)
    import os
    n = pos.numel()
    dev = pos.device
    pos = pos.contiguous()
    iota = torch.arange(n, dtype=torch.int64, device=dev)
    if n < 2:
        return iota
    rounds = max(1, int(os.environ.get("MR_LEX_ROUNDS", _LEX_ROUNDS)))
    e = ext()
    empty = torch.empty(0, dtype=torch.int64, device=dev)
    # 1. length order first: every later sort is stable, so strings whose
    # padded chunks all tie stay shortest-first
    lens = e.pos_len(pos)
    _, perm = sort_by_key(lens, iota, bits=16)
    # 2. round 0 over everything
    keys = e.lex_chunk_keys(text, pos, perm, 0)
    keys, perm = sort_by_key(keys, perm)
    flags = e.head_flags(keys)
    more = lens.index_select(0, perm) > 8
    slots = None  # active slots of perm (None: all of them)
    d = 0
    while True:
        # a segment is length-ascending, so its unfinished strings are a
        # contiguous suffix; only runs of >= 2 of them are still unordered
        head = flags != 0
        prev_tied = torch.zeros_like(more)
        prev_tied[1:] = more[:-1] & ~head[1:]
        next_tied = torch.zeros_like(more)
        next_tied[:-1] = more[1:] & ~head[1:]
        act = more & (prev_tied | next_tied)
        sel = act.nonzero().squeeze(1)  # the round's one host sync
        m = sel.numel()
        if m == 0:
            return perm
        seg_bits = max(1, int(flags.numel()).bit_length())  # seg <= size
        seg = torch.cumsum(flags, 0).index_select(0, sel)
        slots = sel if slots is None else slots.index_select(0, sel)
        d += 1
        if d >= rounds:
            _lex_host_residue(text, pos, perm, slots, seg, 8 * d)
            return perm
        # 3. next chunk of the active set: stable by chunk, then by segment
        idx = perm.index_select(0, slots)
        keys = e.lex_chunk_keys(text, pos, idx, d)
        keys, idx, seg = sort_by_key(keys, idx, seg)
        seg, keys, idx = sort_by_key(seg, keys, idx, bits=seg_bits)
        perm.index_copy_(0, slots, idx)
        flags, more = e.lex_refine(seg, keys, pos, idx, d)
        more = more != 0


def lex_lower_bound(text: torch.Tensor, pos: torch.Tensor,
                    perm: torch.Tensor, queries) -> torch.Tensor:
    """-> i64[nq]: for each byte-string query the smallest j with
    string(perm[j]) >= query (n if none), perm from lex_order."""
    queries = [bytes(q) for q in queries]
    if not text.is_cuda:
        from . import _cpu
        return _cpu.lex_lower_bound(text, pos, perm, queries)
    dev = pos.device
    offs = [0]
    for q in queries:
        offs.append(offs[-1] + len(q))
    blob = b"".join(queries)
    qblob = (torch.frombuffer(bytearray(blob), dtype=torch.uint8).to(dev)
             if blob else torch.empty(0, dtype=torch.uint8, device=dev))
    qoff = torch.tensor(offs, dtype=torch.int64, device=dev)
    return ext().lex_lower_bound(text, pos.contiguous(), perm.contiguous(),
                                 qblob, qoff)


def prefix_succ(p: bytes) -> Optional[bytes]:
    """Smallest byte string greater than every string starting with p:
    strip trailing 0xFF, increment the last byte; None = no upper bound."""
    p = bytes(p).rstrip(b"\xff")
    if not p:
        return None
    return p[:-1] + bytes([p[-1] + 1])


def lex_prefix_range(text: torch.Tensor, pos: torch.Tensor,
                     perm: torch.Tensor, p: bytes):
    """-> (lo, hi): perm[lo:hi] are exactly the strings starting with p."""
    hi_q = prefix_succ(p)
    qs = [bytes(p)] if hi_q is None else [bytes(p), hi_q]
    lb = lex_lower_bound(text, pos, perm, qs).tolist()
    return lb[0], (lb[1] if hi_q is not None else int(perm.numel()))


# ---------------------------------------------------------------------------
# ranked multi-term search over the inverted index (serving path, never in
# the timed job)
# ---------------------------------------------------------------------------

# caps of the postings_search kernel (ops/hip/postings_query.hip): terms per
# query, k, LDS candidate buffer.  The CPU tier has no such limits of its
# own; it keeps the same interface so both tiers accept the same queries.
POSTINGS_TMAX = 16
POSTINGS_KMAX = 256
POSTINGS_BUF = 2048

_POSTINGS_MODES = {"and": 0, "or": 1}


def postings_search_caps():
    """-> (TMAX, KMAX, BUF): the extension's own values on a GPU machine,
    the Python constants above on the CPU tier."""
    if torch.cuda.is_available():
        return tuple(int(c) for c in ext().postings_search_caps())
    return POSTINGS_TMAX, POSTINGS_KMAX, POSTINGS_BUF


def postings_search(keys: torch.Tensor, doc_offsets: torch.Tensor,
                    docs: torch.Tensor, tf: torch.Tensor,
                    weights: Optional[torch.Tensor], qkeys: torch.Tensor,
                    qoff: torch.Tensor, k: int, mode: str = "and"):
    """Ranked search of a batch of queries over the CSR index (keys sorted
    u64 bits, doc_offsets[nwords + 1] into docs/tf, docs ascending and
    unique per word).  Query q is the term hashes qkeys[qoff[q]:qoff[q+1]].

    mode "and": docs in every term's list (unknown term or no terms: none);
    "or": docs in at least one.  score = sum over the query's terms present
    of tf * weights[term row] (weights None or empty: all 1), i64.  Order:
    score descending, doc ascending on equal score.

    -> (docs i64[nq, k], scores i64[nq, k], n i64[nq] = min(k, hits),
    hits i64[nq]); unused slots hold doc = -1, score = 0.

    qkeys/qoff may live on the host: they are checked there and uploaded
    (two uploads); device-resident ones cost one readback of qoff for the
    check.  Nothing else synchronizes."""
    tmax, kmax, _ = postings_search_caps()
    if mode not in _POSTINGS_MODES:
        raise ValueError(f"mode must be 'and' or 'or', got {mode!r}")
    k = int(k)
    if not 1 <= k <= kmax:
        raise ValueError(f"k must be in [1, {kmax}], got {k}")
    if qoff.numel() < 1:
        raise ValueError("qoff holds nq + 1 offsets")
    qo = qoff.cpu()
    if qo.numel() > 1:
        per = qo[1:] - qo[:-1]
        if int(per.min()) < 0 or int(qo[0]) < 0 \
                or int(qo[-1]) > qkeys.numel():
            raise ValueError("qoff must ascend within qkeys")
        if int(per.max()) > tmax:
            raise ValueError(
                f"at most {tmax} terms per query, got {int(per.max())}")
    dev = keys.device
    if weights is None:
        weights = torch.empty(0, dtype=torch.int64, device=dev)
    if not keys.is_cuda:
        from . import _cpu
        return _cpu.postings_search(keys, doc_offsets, docs, tf, weights,
                                    qkeys.cpu(), qo, k,
                                    _POSTINGS_MODES[mode])
    return tuple(ext().postings_search(
        keys.contiguous(), doc_offsets.contiguous(), docs.contiguous(),
        tf.contiguous(), weights.contiguous(),
        qkeys.to(dev).contiguous(), qoff.to(dev).contiguous(), k,
        _POSTINGS_MODES[mode]))


# ---------------------------------------------------------------------------
# positional index: token ordinals and exact-phrase search
# ---------------------------------------------------------------------------

TOKEN_ORDINALS_GRANULE = 64  # text bytes per counted granule (HIP kernel)


def token_ordinals_caps():
    """-> (GRANULE,): the extension's own value on a GPU machine, the
    Python constant above on the CPU tier."""
    if torch.cuda.is_available():
        return tuple(int(c) for c in ext().token_ordinals_caps())
    return (TOKEN_ORDINALS_GRANULE,)


def token_ordinals(text: torch.Tensor, pos: torch.Tensor,
                   starts: torch.Tensor):
    """Document and 0-based token ordinal of each word occurrence.

    text u8; pos i64[n], the tokenizer's off << 16 | len of each
    occurrence; starts i64[ndocs + 1], the documents' byte offsets plus
    the end.  doc = searchsorted(starts, off, right) - 1 (the build's own
    rule); ord = the number of word starts in [starts[doc], off), a word
    start being a non-whitespace byte at offset 0 or after a whitespace
    byte, so a split that begins mid-word holds no start for the fragment.
    -> (doc i64[n], ord i32[n]).  Texts below 2^31 bytes; the occurrences
    need no order; no host sync."""
    if text.numel() >= 2 ** 31:
        raise ValueError(
            f"token_ordinals: text of {text.numel()} bytes; ordinals are "
            "32-bit")
    if starts.numel() < 1:
        raise ValueError("starts holds ndocs + 1 offsets")
    if not text.is_cuda:
        from . import _cpu
        return _cpu.token_ordinals(text, pos, starts)
    return tuple(ext().token_ordinals(text.contiguous(), pos.contiguous(),
                                      starts.contiguous()))


def postings_phrase(keys: torch.Tensor, doc_offsets: torch.Tensor,
                    docs: torch.Tensor, tf: torch.Tensor,
                    pos_offsets: torch.Tensor, positions: torch.Tensor,
                    qkeys: torch.Tensor, qoff: torch.Tensor, k: int):
    """Exact-phrase search of a batch of queries over the positional index:
    the CSR arrays of postings_search plus pos_offsets i64[np + 1] into
    positions i32[nocc], posting j owning the ascending token ordinals
    positions[pos_offsets[j] : pos_offsets[j] + tf[j]].  Query q is the
    ORDERED term hashes qkeys[qoff[q]:qoff[q+1]], duplicates kept.

    A document matches iff every term has a posting for it and some s >= 0
    has s + i among term i's positions for every i; score = the number of
    such s (tf for one term).  No terms or an unknown term: no matches.
    Order: score descending, doc ascending on equal score.

    -> (docs i64[nq, k], scores i64[nq, k], n i64[nq] = min(k, hits),
    hits i64[nq]); unused slots hold doc = -1, score = 0.  Checks, caps
    and uploads are those of postings_search."""
    tmax, kmax, _ = postings_search_caps()
    k = int(k)
    if not 1 <= k <= kmax:
        raise ValueError(f"k must be in [1, {kmax}], got {k}")
    if qoff.numel() < 1:
        raise ValueError("qoff holds nq + 1 offsets")
    if pos_offsets.numel() != docs.numel() + 1:
        raise ValueError("pos_offsets holds one offset per posting + 1")
    if positions.dtype != torch.int32:
        raise ValueError("positions must be int32")
    qo = qoff.cpu()
    if qo.numel() > 1:
        per = qo[1:] - qo[:-1]
        if int(per.min()) < 0 or int(qo[0]) < 0 \
                or int(qo[-1]) > qkeys.numel():
            raise ValueError("qoff must ascend within qkeys")
        if int(per.max()) > tmax:
            raise ValueError(
                f"at most {tmax} terms per query, got {int(per.max())}")
    dev = keys.device
    if not keys.is_cuda:
        from . import _cpu
        return _cpu.postings_phrase(keys, doc_offsets, docs, tf, pos_offsets,
                                    positions, qkeys.cpu(), qo, k)
    return tuple(ext().postings_phrase(
        keys.contiguous(), doc_offsets.contiguous(), docs.contiguous(),
        tf.contiguous(), pos_offsets.contiguous(), positions.contiguous(),
        qkeys.to(dev).contiguous(), qoff.to(dev).contiguous(), k))


# ---------------------------------------------------------------------------
# equi-join of two key-sorted columns (the join step of the reduce-side join)
# ---------------------------------------------------------------------------

# caps of the join_expand kernel (ops/hip/join.hip): output rows per tile,
# offsets staged in LDS per tile.  The CPU tier has no tiles; it reports the
# same values so tests size their cases alike on both tiers.
JOIN_TILE = 2048
JOIN_LDS_ROWS = 1024
# caps of the windowed bounds kernel: left rows per tile, right keys of a
# tile's window staged in LDS
JOIN_BOUNDS_TILE = 1024
JOIN_BOUNDS_WIN = 2048

_JOIN_HOWS = ("inner", "left", "semi", "anti")


class JoinTooLarge(ValueError):
    """The join would produce more than max_rows output rows."""

    def __init__(self, total: int, max_rows: int):
        super().__init__(
            f"join produces {total} rows, over the limit of {max_rows} "
            "(max_rows)")
        self.total = int(total)
        self.max_rows = int(max_rows)


def join_caps():
    """-> (JOIN_TILE, JOIN_LDS_ROWS): the extension's own values on a GPU
    machine, the Python constants above on the CPU tier."""
    if torch.cuda.is_available():
        return tuple(int(c) for c in ext().join_caps())
    return JOIN_TILE, JOIN_LDS_ROWS


def join_bounds_caps():
    """-> (JOIN_BOUNDS_TILE, JOIN_BOUNDS_WIN), as join_caps."""
    if torch.cuda.is_available():
        return tuple(int(c) for c in ext().join_bounds_caps())
    return JOIN_BOUNDS_TILE, JOIN_BOUNDS_WIN


def join_bounds(lkeys: torch.Tensor, rkeys: torch.Tensor):
    """Pass 1 of join_sorted: (lo i64[nl], cnt i64[nl]), the start and the
    length of each left key's run of equal right keys.  No host sync, so a
    caller can size (or refuse) the output before it is expanded.
    MR_JOIN_BOUNDS_ROW=1 (read per call) runs the thread-per-row kernel
    instead of the block-window one, for A/B."""
    if not lkeys.is_cuda and not rkeys.is_cuda:
        from . import _cpu
        return _cpu.join_bounds(lkeys, rkeys)
    import os
    window = os.environ.get("MR_JOIN_BOUNDS_ROW", "0") != "1"
    return tuple(ext().join_bounds(lkeys.contiguous(), rkeys.contiguous(),
                                   window))


def join_sorted(lkeys: torch.Tensor, rkeys: torch.Tensor,
                how: str = "inner", max_rows: Optional[int] = None,
                bounds=None):
    """Equi-join of two key columns, each sorted ascending in u64 bit order
    (i64 tensors holding u64 bit patterns).  Sortedness is the caller's
    contract and is not checked; the inputs are never written.

    how "inner" / "left": -> (li i64[total], ri i64[total]), row indices
    into the two inputs, ordered by li then ri; under "left" an unmatched
    left row appears once, in its place, with ri == -1.
    how "semi" / "anti": -> li i64[m] ascending, the left rows with / without
    a match.

    max_rows: raise JoinTooLarge before allocating the output when it would
    hold more rows.  bounds: the pair join_bounds returned for these
    columns, when the caller already holds it.  One host sync (the output
    size); semi and anti sync in torch.nonzero instead."""
    if how not in _JOIN_HOWS:
        raise ValueError(f"how must be one of {_JOIN_HOWS}, got {how!r}")
    if not lkeys.is_cuda and not rkeys.is_cuda:
        from . import _cpu
        return _cpu.join_sorted(lkeys, rkeys, how, max_rows, bounds)
    lo, cnt = bounds if bounds is not None else join_bounds(lkeys, rkeys)
    if how == "semi":
        return torch.nonzero(cnt > 0).squeeze(1)
    if how == "anti":
        return torch.nonzero(cnt == 0).squeeze(1)
    per = cnt if how == "inner" else cnt.clamp(min=1)
    off = torch.zeros(cnt.numel() + 1, dtype=torch.int64, device=cnt.device)
    torch.cumsum(per, 0, out=off[1:])
    total = int(off[-1].item())  # the op's only host sync
    if max_rows is not None and total > max_rows:
        raise JoinTooLarge(total, max_rows)
    return tuple(ext().join_expand(off, lo, cnt, total))


# ---------------------------------------------------------------------------
# as-of join of two relations sorted on (key, time)
# ---------------------------------------------------------------------------

# caps of the windowed as-of kernel (ops/hip/asof.hip): left rows per tile,
# right rows of a tile's window staged in LDS.  The CPU tier has no tiles; it
# reports the same values so tests size their cases alike on both tiers.
ASOF_TILE = 1024
ASOF_WIN = 2048

_ASOF_DIRECTIONS = {"backward": 0, "forward": 1, "nearest": 2}


def asof_caps():
    """-> (ASOF_TILE, ASOF_WIN): the extension's own values on a GPU
    machine, the Python constants above on the CPU tier."""
    if torch.cuda.is_available():
        return tuple(int(c) for c in ext().asof_caps())
    return ASOF_TILE, ASOF_WIN


def _asof_tolerance(tolerance):
    if tolerance is None:
        return None
    if isinstance(tolerance, bool) or not isinstance(tolerance, int):
        raise TypeError(f"tolerance must be an int or None, got {tolerance!r}")
    if not 0 <= tolerance < 2 ** 63:
        raise ValueError(f"tolerance must be in [0, 2^63), got {tolerance}")
    return tolerance


def asof_sorted(lkeys: torch.Tensor, ltimes: torch.Tensor,
                rkeys: torch.Tensor, rtimes: torch.Tensor,
                direction: str = "backward", tolerance: Optional[int] = None,
                allow_exact: bool = True) -> torch.Tensor:
    """As-of join of two relations, each sorted ascending on (key, order key
    of the time): keys are i64 tensors holding u64 bit patterns, times are
    i64 or f64 (one dtype on both sides) ordered by group_order_keys.
    Sortedness is the caller's contract and is not checked; the inputs are
    never written.  -> ri i64[nl]: for every left row the index of the right
    row it matches, or -1.  No host sync.

    With P / Q the number of right rows < / <= the left row's (key, time):
    "backward" takes row Q - 1, the latest right row of the key at or before
    the time (P - 1, strictly before, when allow_exact is False); "forward"
    takes row P, the earliest at or after it (Q, strictly after);
    "nearest" takes the closer of the two, the backward one on a tie.  A
    candidate of another key never matches.  In a run of right rows with
    equal (key, time), backward takes the last and forward the first.

    tolerance (i64 times only, 0 <= tolerance < 2^63): a candidate further
    than this from the left time does not match.  The distance is the u64
    difference of the two order keys, as in session_flags, so it cannot
    overflow whatever the span.

    Device path (ops/hip/asof.hip): a block per tile of ASOF_TILE left rows
    searches the window of right rows its tile can reach, staged in LDS when
    it holds at most ASOF_WIN rows.  MR_ASOF_ROW=1 (read per call) runs the
    thread-per-row kernel over the whole right side instead, for A/B."""
    if direction not in _ASOF_DIRECTIONS:
        raise ValueError(
            f"direction must be one of {tuple(_ASOF_DIRECTIONS)}, "
            f"got {direction!r}")
    tolerance = _asof_tolerance(tolerance)
    if lkeys.dtype != torch.int64 or rkeys.dtype != torch.int64:
        raise TypeError("asof: key columns must be int64")
    if ltimes.dtype != rtimes.dtype:
        raise TypeError(
            "asof: both sides need one time dtype, got "
            f"{ltimes.dtype} and {rtimes.dtype}")
    lt, f64 = _group_vals_i64(ltimes, "ltimes")
    rt, _ = _group_vals_i64(rtimes, "rtimes")
    if f64 and tolerance is not None:
        raise TypeError("asof: a tolerance needs int64 times, got float64")
    if ltimes.numel() != lkeys.numel() or rtimes.numel() != rkeys.numel():
        raise ValueError("one time per key required on each side")
    if not any(t.is_cuda for t in (lkeys, ltimes, rkeys, rtimes)):
        from . import _cpu
        return _cpu.asof_sorted(lkeys, ltimes, rkeys, rtimes, direction,
                                tolerance, bool(allow_exact))
    row = os.environ.get("MR_ASOF_ROW", "0") == "1"
    return ext().asof_sorted(lkeys, lt, rkeys, rt,
                             _ASOF_DIRECTIONS[direction], tolerance,
                             bool(allow_exact), f64, row)


# ---------------------------------------------------------------------------
# per-key order statistics over key-sorted rows (K4/K5 for reducers that
# need the whole value list of a key: quantiles, top-k, distinct counts)
# ---------------------------------------------------------------------------

# caps of the group kernels (ops/hip/group.hip): rows per LDS-sorted tile,
# rank specifications per pick launch.  The CPU tier has no tiles; it
# reports the same values so tests size their cases alike on both tiers.
GROUP_TILE = 2048
GROUP_QMAX = 8
# the tile kernel orders a tile whose segments are all this short by rank
# counting and runs the bitonic network otherwise; tests size cases by it
GROUP_RANK_MAX = 256
GROUP_MAX_DEN = 10 ** 6
GROUP_MAX_ROWS = 2 ** 31


def group_caps():
    """-> (GROUP_TILE, GROUP_QMAX): the extension's own values on a GPU
    machine, the Python constants above on the CPU tier."""
    if torch.cuda.is_available():
        return tuple(int(c) for c in ext().group_caps())
    return GROUP_TILE, GROUP_QMAX


def group_rank_max() -> int:
    """-> GROUP_RANK_MAX, from the extension on a GPU machine."""
    if torch.cuda.is_available():
        return int(ext().group_rank_max())
    return GROUP_RANK_MAX


def _group_vals_i64(vals: torch.Tensor, name: str = "vals"):
    """-> (int64 view, is f64) of an i64 or f64 value column."""
    if vals.dtype == torch.float64:
        return vals.view(torch.int64), True
    if vals.dtype == torch.int64:
        return vals, False
    raise TypeError(f"{name} must be int64 or float64, got {vals.dtype}")


def _group_check_rows(n: int) -> None:
    if n >= GROUP_MAX_ROWS:
        raise ValueError(f"group ops take fewer than 2^31 rows, got {n}")


def group_order_keys(vals: torch.Tensor) -> torch.Tensor:
    """The u64 order key of each i64 or f64 value, as an i64 bit pattern:
    i64 bits ^ 2^63; f64 the sign-flip transform with -0.0 keyed as +0.0
    and every NaN keyed above +inf.  Values with equal order keys are equal
    to every group op."""
    v, f64 = _group_vals_i64(vals)
    if not vals.is_cuda:
        from . import _cpu
        return _cpu._from_u64(_cpu.group_order_keys(vals))
    return ext().group_order_keys(v.contiguous(), f64)


def group_by_key_sorted(keys: torch.Tensor):
    """keys sorted (u64 bit order) -> (ukeys i64[nseg], offsets
    i64[nseg + 1]): segment s is rows offsets[s]:offsets[s + 1].  One host
    sync (the segment count)."""
    _group_check_rows(keys.numel())
    if not keys.is_cuda:
        from . import _cpu
        return _cpu.group_by_key_sorted(keys)
    keys = keys.contiguous()
    return _group_offsets(keys, ext().head_flags(keys))


def _group_offsets(keys, flags):
    n = keys.numel()
    heads = torch.nonzero(flags).squeeze(1)
    offsets = torch.empty(heads.numel() + 1, dtype=torch.int64,
                          device=keys.device)
    offsets[:-1] = heads
    offsets[-1] = n
    return keys.index_select(0, heads), offsets


def _group_two_sort(keys, v, f64, return_perm=False):
    """The composition: sort by order key, then stably by key."""
    ok = ext().group_order_keys(v, f64)
    cols = [keys, v]
    if return_perm:  # -> (values, input rows)
        cols.append(torch.arange(keys.numel(), device=keys.device))
    cols = sort_by_key(*sort_by_key(ok, *cols)[1:])[1:]
    return cols if return_perm else cols[0]


def group_straddlers(offsets: torch.Tensor, tile: int):
    """-> (sidx i64[ns], rows): the segments that cross a boundary between
    tiles of `tile` rows (start // tile != (end - 1) // tile) and the
    number of rows they hold.  One host sync."""
    st, en = offsets[:-1], offsets[1:]
    smask = torch.div(st, tile, rounding_mode="floor") != torch.div(
        en - 1, tile, rounding_mode="floor")
    sidx = torch.nonzero(smask).squeeze(1)
    rows = int((en - st).index_select(0, sidx).sum().item()) \
        if sidx.numel() else 0
    return sidx, rows


def sort_values_in_groups(keys_sorted: torch.Tensor, vals: torch.Tensor,
                          offsets: Optional[torch.Tensor] = None,
                          return_perm: bool = False):
    """The value column ordered within every key: keys_sorted ascending in
    u64 bit order (the caller's contract), vals i64 or f64, one per key; the
    dtype is kept and the inputs are never written.  Order is that of
    group_order_keys; values with equal order keys keep their input order.
    offsets: what group_by_key_sorted returned for these keys, when the
    caller holds it.  return_perm=True: -> (sorted_vals, perm) with perm
    i64[n] and sorted_vals == vals[perm] bit for bit; perm is the one stable
    order on (key, order key of the value, input row), so a second column
    can be carried through the ordering.

    Device path: every tile of GROUP_TILE rows is sorted in LDS by (segment,
    order key) — by rank counting where the tile's segments are at most
    GROUP_RANK_MAX long, by a bitonic network otherwise — which finishes the
    segments inside one tile; the rows of
    segments that cross a tile boundary are compacted, sorted with
    sort_by_key (order key, then stably their segment number, a pass or two
    since few segments are that long) and copied over their slots; when
    every row is in such a segment the tile pass is skipped.  This path
    measured faster than the composition at every share of such rows
    (profiles/grouped.md), so nothing dispatches on the share.  Under
    MR_GROUP_TWO_SORT=1 (read per call) the composition runs instead: sort
    by order key, then stably by key.  Two host syncs (the segments, the
    straddlers)."""
    n = keys_sorted.numel()
    if vals.numel() != n:
        raise ValueError("one value per key required")
    _group_check_rows(n)
    v, f64 = _group_vals_i64(vals)
    if not keys_sorted.is_cuda and not vals.is_cuda:
        if keys_sorted.dtype != torch.int64:
            raise TypeError("keys must be int64")
        from . import _cpu
        return _cpu.sort_values_in_groups(keys_sorted, vals, return_perm)
    import os
    keys = keys_sorted.contiguous()
    v = v.contiguous()
    if os.environ.get("MR_GROUP_TWO_SORT", "0") == "1":
        if return_perm:
            out, perm = _group_two_sort(keys, v, f64, True)
            return out.view(vals.dtype), perm
        return _group_two_sort(keys, v, f64).view(vals.dtype)
    if n == 0:
        ext().group_tile_sort(keys, v, f64)  # the host checks still run
        return (vals.clone(), v.clone()) if return_perm else vals.clone()
    e = ext()
    flags = e.head_flags(keys)
    seg = torch.cumsum(flags, 0)
    if offsets is None:
        _, offsets = _group_offsets(keys, flags)
    tile = group_caps()[0]
    sidx, rows = group_straddlers(offsets, tile)
    # all rows in straddlers: every slot is overwritten below.  The tile
    # pass writes out and perm at the same slots, and the straddlers' slots
    # it leaves unwritten are overwritten in both columns
    perm = None
    if rows == n:
        out = torch.empty_like(v)
        if return_perm:
            perm = torch.empty_like(v)
    elif return_perm:
        out, perm = e.group_tile_sort_perm(seg, v, f64)
    else:
        out = e.group_tile_sort(seg, v, f64)
    if rows:
        ns = sidx.numel()
        sst = offsets.index_select(0, sidx)
        slen = offsets.index_select(0, sidx + 1) - sst
        first = torch.cumsum(slen, 0) - slen  # of each straddler, compacted
        snum = torch.repeat_interleave(
            torch.arange(ns, device=keys.device), slen, output_size=rows)
        ridx = (torch.arange(rows, device=keys.device)
                + (sst - first).index_select(0, snum))
        # [straddler number, value(, input row)]
        cols = [snum, v.index_select(0, ridx)] + ([ridx] if return_perm
                                                  else [])
        cols = sort_by_key(e.group_order_keys(cols[1], f64), *cols)[1:]
        cols = sort_by_key(*cols, bits=max(1, (ns - 1).bit_length()))
        out.index_copy_(0, ridx, cols[1])
        if return_perm:
            perm.index_copy_(0, ridx, cols[2])
    out = out.view(vals.dtype)
    return (out, perm) if return_perm else out


def _group_rank_specs(fracs, interpolation: str):
    """-> [(num, den, higher)] after the checks of group_quantiles."""
    import fractions
    if interpolation not in ("lower", "higher"):
        raise ValueError("interpolation must be 'lower' or 'higher', got "
                         f"{interpolation!r}")
    fracs = list(fracs)
    qmax = group_caps()[1]
    if not 1 <= len(fracs) <= qmax:
        raise ValueError(f"Q must be in [1, {qmax}], got {len(fracs)}")
    specs = []
    for f in fracs:
        if isinstance(f, fractions.Fraction):
            num, den = f.numerator, f.denominator
        elif (isinstance(f, (tuple, list)) and len(f) == 2
              and all(isinstance(x, int) and not isinstance(x, bool)
                      for x in f)):
            num, den = f
        else:
            raise TypeError(
                "fracs must be (num, den) integer pairs or Fractions, got "
                f"{f!r}: a float's index is not exact")
        if not 1 <= den <= GROUP_MAX_DEN:
            raise ValueError(f"den must be in [1, 10^6], got {den}")
        if not 0 <= num <= den:
            raise ValueError(f"num must be in [0, den], got {num}/{den}")
        specs.append((int(num), int(den), interpolation == "higher"))
    return specs


def _group_check_offsets(offsets: torch.Tensor) -> None:
    if offsets.dtype != torch.int64:
        raise TypeError("offsets must be int64")
    if offsets.numel() < 1:
        raise ValueError("offsets holds nseg + 1 entries")


def group_quantiles(offsets: torch.Tensor, sorted_vals: torch.Tensor, fracs,
                    interpolation: str = "lower") -> torch.Tensor:
    """-> [nseg, Q] in the values' dtype: for each segment of the ordered
    value column (sort_values_in_groups) and each fraction num/den the value
    at index (num * (len - 1) + (den - 1 if higher else 0)) // den, in exact
    integer arithmetic.  fracs: (num, den) integer pairs or
    fractions.Fraction, 0 <= num <= den <= 10^6, at most GROUP_QMAX of them;
    floats are refused.  No host sync."""
    specs = _group_rank_specs(fracs, interpolation)
    _group_check_offsets(offsets)
    _group_check_rows(sorted_vals.numel())
    v, _ = _group_vals_i64(sorted_vals, "sorted_vals")
    if not offsets.is_cuda and not sorted_vals.is_cuda:
        from . import _cpu
        return _cpu.group_pick(offsets, sorted_vals, specs)
    out = ext().group_pick(offsets.contiguous(), v.contiguous(),
                           [s[0] for s in specs], [s[1] for s in specs],
                           [s[2] for s in specs])
    return out.view(sorted_vals.dtype)


def group_topk(offsets: torch.Tensor, sorted_vals: torch.Tensor, k: int,
               largest: bool = True):
    """-> (vals [nseg, k], n i64[nseg] = min(k, len)): the k largest values
    of each ordered segment, descending (NaN first), or the k smallest,
    ascending.  Unused slots hold 0.  No host sync."""
    k = int(k)
    if k < 1:
        raise ValueError(f"k must be at least 1, got {k}")
    _group_check_offsets(offsets)
    _group_check_rows(sorted_vals.numel())
    _group_vals_i64(sorted_vals, "sorted_vals")
    st, en = offsets[:-1], offsets[1:]
    lens = en - st
    j = torch.arange(k, device=offsets.device)
    pos = (en - 1).unsqueeze(1) - j if largest else st.unsqueeze(1) + j
    used = j < lens.unsqueeze(1)
    if sorted_vals.numel():
        out = sorted_vals[pos.clamp(0, sorted_vals.numel() - 1)]
        out = torch.where(used, out, torch.zeros_like(out))
    else:
        out = torch.zeros(pos.shape, dtype=sorted_vals.dtype,
                          device=sorted_vals.device)
    return out, lens.clamp(max=k)


def group_distinct_flags(keys_sorted: torch.Tensor,
                         sorted_vals: torch.Tensor) -> torch.Tensor:
    """flags i64[n]: 1 where a row starts a segment or its order key
    differs from the previous row's (values ordered within each key)."""
    if sorted_vals.numel() != keys_sorted.numel():
        raise ValueError("one value per key required")
    _group_check_rows(keys_sorted.numel())
    v, f64 = _group_vals_i64(sorted_vals, "sorted_vals")
    if not keys_sorted.is_cuda and not sorted_vals.is_cuda:
        from . import _cpu
        return _cpu.group_distinct_flags(keys_sorted, sorted_vals)
    return ext().group_distinct_flags(keys_sorted.contiguous(),
                                      v.contiguous(), f64)


def group_distinct(keys_sorted: torch.Tensor,
                   sorted_vals: torch.Tensor) -> torch.Tensor:
    """-> counts i64[nseg]: the number of distinct values (order keys) of
    each key; +0.0 and -0.0 count once, all NaNs count once."""
    flags = group_distinct_flags(keys_sorted, sorted_vals)
    return reduce_by_key_sorted(keys_sorted, flags, op="sum")[1]


# ---------------------------------------------------------------------------
# per-key running aggregates and sessions over grouped rows (K4/K5 for
# reducers whose answer is as long as their input)
# ---------------------------------------------------------------------------

# caps of the scan kernels (ops/hip/seg_scan.hip): rows per tile, tiles per
# loop trip of the one-block carry pass.  The CPU tier has no tiles; it
# reports the same values so tests size their cases alike on both tiers.
SEG_SCAN_TILE = 2048
SEG_CARRY_CHUNK = 1024

_SEG_SCAN_OPS = {"sum": 0, "min": 1, "max": 2}


def seg_scan_caps():
    """-> (SEG_SCAN_TILE, CARRY_CHUNK): the extension's own values on a GPU
    machine, the Python constants above on the CPU tier."""
    if torch.cuda.is_available():
        return tuple(int(c) for c in ext().seg_scan_caps())
    return SEG_SCAN_TILE, SEG_CARRY_CHUNK


def scan_by_key_sorted(keys: torch.Tensor, vals: torch.Tensor,
                       op: str = "sum") -> torch.Tensor:
    """The running sum, minimum or maximum within each segment: row i holds
    op over the rows of its segment up to and including i.  A row starts a
    segment when it is row 0 or its key differs from the previous row's, so
    keys need only be grouped, not sorted.  vals is i64 or f64, one per key;
    the result has its dtype and length and the inputs are never written.

    i64 sums wrap modulo 2^64.  f64 sums are IEEE in the kernel's own
    association (tiles, waves, rounds of 64 rows; not left to right): exact
    whenever every partial sum is representable.  min / max compare by
    group_order_keys (-0.0 equals +0.0, NaN is the largest value) and keep
    the stored bits of the earlier row among equal order keys.

    Device path (ops/hip/seg_scan.hip): reduce-then-scan over tiles of
    SEG_SCAN_TILE rows, three launches ordered by their boundaries alone,
    no host sync, fewer than 2^31 rows."""
    if op not in _SEG_SCAN_OPS:
        raise ValueError(f"op must be 'sum', 'min' or 'max', got {op!r}")
    v, f64 = _group_vals_i64(vals)
    if not keys.is_cuda and not vals.is_cuda:
        if keys.dtype != torch.int64:
            raise TypeError("keys must be int64")
        if vals.numel() != keys.numel():
            raise ValueError("one value per key required")
        _group_check_rows(keys.numel())
        from . import _cpu
        return _cpu.scan_by_key_sorted(keys, vals, op)
    return ext().scan_by_key_sorted(keys, v, _SEG_SCAN_OPS[op],
                                    f64).view(vals.dtype)


def _session_gap(gap) -> int:
    if isinstance(gap, bool) or not isinstance(gap, int):
        raise TypeError(f"gap must be an int, got {gap!r}")
    if not 0 <= gap < 2 ** 63:
        raise ValueError(f"gap must be in [0, 2^63), got {gap}")
    return gap


def session_flags(keys_sorted: torch.Tensor, sorted_times: torch.Tensor,
                  gap: int) -> torch.Tensor:
    """flags i64[n]: 1 where a row starts a key, or where its time exceeds
    the previous row's by more than gap.  Times are i64, ascending within
    each key (f64 is refused); 0 <= gap < 2^63.  The difference is taken
    between the order keys in u64 arithmetic and compared to gap as u64, so
    it cannot overflow whatever the span.  No host sync."""
    gap = _session_gap(gap)
    if sorted_times.dtype != torch.int64:
        raise TypeError(
            f"session times must be int64, got {sorted_times.dtype}")
    if not keys_sorted.is_cuda and not sorted_times.is_cuda:
        if keys_sorted.dtype != torch.int64:
            raise TypeError("keys must be int64")
        if sorted_times.numel() != keys_sorted.numel():
            raise ValueError("one time per key required")
        _group_check_rows(keys_sorted.numel())
        from . import _cpu
        return _cpu.session_flags(keys_sorted, sorted_times, gap)
    return ext().session_flags(keys_sorted, sorted_times, gap)


def group_sessions(keys_sorted: torch.Tensor, sorted_times: torch.Tensor,
                   gap: int):
    """-> (skeys i64[nsess], soffsets i64[nsess + 1]): the key of every
    session and the sessions' offsets into the rows; session s is rows
    soffsets[s]:soffsets[s + 1].  One host sync (the session count)."""
    flags = session_flags(keys_sorted, sorted_times, gap)
    return _group_offsets(keys_sorted, flags)


# ---------------------------------------------------------------------------
# per-key rolling aggregates over (key, time)-sorted rows: every row gets a
# frame of rows of its own key and an aggregate over it
# ---------------------------------------------------------------------------

# caps of the frame kernels (ops/hip/frame.hip): rows per tile of the window
# bounds kernel, rows of a tile's window staged in LDS, rows per tile of the
# reduce kernels.  The CPU tier has no tiles; it reports the same values so
# tests size their cases alike on both tiers.
FRAME_TILE = 1024
FRAME_WIN = 2048
FRAME_RTILE = 2048
FRAME_MAX_ROW_EXTENT = 2 ** 31
# which bounds kernel runs when MR_FRAME_ROW is unset: the measured winner
# on the benchmark shapes (profiles/rolling.md)
_FRAME_ROW_DEFAULT = "1"


def frame_caps():
    """-> (FRAME_TILE, FRAME_WIN, FRAME_RTILE): the extension's own values
    on a GPU machine, the Python constants above on the CPU tier."""
    if torch.cuda.is_available():
        return tuple(int(c) for c in ext().frame_caps())
    return FRAME_TILE, FRAME_WIN, FRAME_RTILE


def frame_tree_levels(ntiles: int):
    """The node counts of the tree frame_reduce builds over ntiles tile
    aggregates, level 0 (the tiles) first: level l holds the ntiles >> l
    nodes whose 2^l tiles all exist.  ext().frame_tree returns the levels
    one behind the other."""
    out = []
    while ntiles >= 1:
        out.append(ntiles)
        ntiles >>= 1
    return out


def _frame_extent(x, name: str, limit: int, limit_name: str) -> int:
    if isinstance(x, bool) or not isinstance(x, int):
        raise TypeError(f"{name} must be an int, got {x!r}")
    if not 0 <= x < limit:
        raise ValueError(f"{name} must be in [0, {limit_name}), got {x}")
    return x


def frame_bounds(keys_sorted: torch.Tensor, sorted_times: torch.Tensor,
                 preceding: int, following: int = 0):
    """Range frames of a relation sorted ascending on (key, order key of the
    time), the contract of asof_sorted: keys are i64 tensors holding u64 bit
    patterns, times are i64 (f64 is refused with a TypeError, as for
    session_flags).  Sortedness is the caller's contract and is not checked;
    the inputs are never written.  -> (lo, hi), i64[n] each: the frame of
    row i is the rows lo[i] <= j < hi[i], with lo[i] <= i < hi[i].  No host
    sync.

    preceding and following are Python ints in [0, 2^63).  With T the order
    key of row i's time, the frame holds every row of i's key whose order
    key lies in [sat(T - preceding), sat(T + following)], both ends
    inclusive and computed in u64, saturating at 0 and 2^64 - 1, so no span
    can overflow.  This is SQL's RANGE BETWEEN preceding PRECEDING AND
    following FOLLOWING: rows with the time of row i (its peers) are always
    in its frame, those behind it too, so an aggregate over a range frame
    depends on the multiset of (time, value) alone.  lo and hi are
    non-decreasing along the rows and a frame never crosses a key.

    Device path (ops/hip/frame.hip): a thread per row brackets each end by
    an exponential search outward from the row itself, then bisects the
    bracket.  MR_FRAME_ROW=0 (read per call) runs the block-window kernel
    in the shape of asof_sorted's instead (tiles of FRAME_TILE rows, a
    window of at most FRAME_WIN rows staged in LDS), for A/B; the two give
    the same output."""
    preceding = _frame_extent(preceding, "preceding", 2 ** 63, "2^63")
    following = _frame_extent(following, "following", 2 ** 63, "2^63")
    if sorted_times.dtype != torch.int64:
        raise TypeError(
            f"range frames need int64 times, got {sorted_times.dtype}")
    if keys_sorted.dtype != torch.int64:
        raise TypeError("keys must be int64")
    if sorted_times.numel() != keys_sorted.numel():
        raise ValueError("one time per key required")
    _group_check_rows(keys_sorted.numel())
    if not keys_sorted.is_cuda and not sorted_times.is_cuda:
        from . import _cpu
        return _cpu.frame_bounds(keys_sorted, sorted_times, preceding,
                                 following)
    row = os.environ.get("MR_FRAME_ROW", _FRAME_ROW_DEFAULT) == "1"
    lo, hi = ext().frame_bounds(keys_sorted, sorted_times, preceding,
                                following, row)
    return lo, hi


def frame_bounds_rows(offsets: torch.Tensor, preceding: int,
                      following: int = 0, nrows: Optional[int] = None):
    """Row frames (SQL's ROWS BETWEEN preceding PRECEDING AND following
    FOLLOWING) from the offsets of group_by_key_sorted: for row i of the key
    that owns rows [s, e), lo = max(s, i - preceding) and
    hi = min(e, i + following + 1).  preceding and following are Python
    ints in [0, 2^31).  -> (lo, hi), i64[n] each, on the device of offsets.

    Plain torch on the offsets (a repeat_interleave, an arange and two
    clamps): every row's answer is arithmetic on its own index and its
    key's two offsets, with nothing to search, so it is not worth a kernel.
    nrows = the row count offsets[-1] when the caller knows it; without it
    the count is read back (one host sync)."""
    preceding = _frame_extent(preceding, "preceding", FRAME_MAX_ROW_EXTENT,
                              "2^31")
    following = _frame_extent(following, "following", FRAME_MAX_ROW_EXTENT,
                              "2^31")
    if offsets.dtype != torch.int64:
        raise TypeError("offsets must be int64")
    _group_check_offsets(offsets)
    if nrows is None:
        nrows = int(offsets[-1])
    _group_check_rows(nrows)
    seg = torch.repeat_interleave(
        torch.arange(offsets.numel() - 1, device=offsets.device),
        offsets[1:] - offsets[:-1], output_size=nrows)
    i = torch.arange(nrows, device=offsets.device)
    lo = torch.maximum(i - preceding, offsets[:-1].index_select(0, seg))
    hi = torch.minimum(i + (following + 1), offsets[1:].index_select(0, seg))
    return lo, hi


def frame_reduce(vals: torch.Tensor, lo: torch.Tensor, hi: torch.Tensor,
                 op: str = "sum") -> torch.Tensor:
    """out[i] = the sum, minimum or maximum of vals over the rows
    lo[i] <= j < hi[i], for frames with lo[i] <= i < hi[i] as frame_bounds
    and frame_bounds_rows make them.  vals is i64 or f64, lo and hi i64, one
    per value; the result has the dtype and length of vals and the inputs
    are never written.  It needs no keys: a frame never crosses one.  No
    host sync.

    i64 sums wrap modulo 2^64.  f64 sums are IEEE over the rows of the frame
    only, in the kernel's own association: the pieces combined for a frame
    are disjoint and lie inside it (never a difference of running sums), so
    the error is bounded by the frame's own sum |v| and a NaN or an inf
    affects exactly the frames that contain it.  min / max compare by
    group_order_keys (-0.0 equals +0.0, NaN is the largest value) and return
    the stored bits of the earliest row of the frame among those with the
    winning order key.

    A frame that breaks the contract is clamped, lo to [0, i] and hi to
    [i + 1, n], on both tiers: it gives a defined answer and never
    addresses outside the column.

    Device path (ops/hip/frame.hip): prefix and suffix aggregates inside
    tiles of FRAME_RTILE rows and an aligned binary tree over the tile
    aggregates; a frame inside one tile is a query of a tree built over the
    tile in LDS, a longer one is suffix + whole tiles from the tile tree +
    prefix.  Three launches ordered by their boundaries alone, fewer than
    2^31 rows.  The CPU tier aggregates every frame directly (f64 sums by
    math.fsum), so f64 sums may differ from the device in the last bits."""
    if op not in _SEG_SCAN_OPS:
        raise ValueError(f"op must be 'sum', 'min' or 'max', got {op!r}")
    v, f64 = _group_vals_i64(vals)
    if lo.dtype != torch.int64 or hi.dtype != torch.int64:
        raise TypeError("lo and hi must be int64")
    if lo.numel() != vals.numel() or hi.numel() != vals.numel():
        raise ValueError("one lo and one hi per value required")
    _group_check_rows(vals.numel())
    if not vals.is_cuda and not lo.is_cuda and not hi.is_cuda:
        from . import _cpu
        return _cpu.frame_reduce(vals, lo, hi, op)
    return ext().frame_reduce(v, lo, hi, _SEG_SCAN_OPS[op],
                              f64).view(vals.dtype)


# ---------------------------------------------------------------------------
# resident-graph propagation (K4/K5 for iterative reducers over keyed data:
# every key reduces a value gathered from other keys over its edge list)
# ---------------------------------------------------------------------------

# caps of the graph kernels (ops/hip/graph.hip): edges per tile, most blocks
# (and rows of partials) of the PageRank update pass.  The CPU tier has no
# tiles; it reports the same values so tests size their cases alike.
GRAPH_TILE = 2048
GRAPH_PR_BLOCKS = 1024

_GRAPH_IDENTITY = {"sum": 0, "min": 2 ** 63 - 1, "max": -2 ** 63}


def graph_caps():
    """-> (GRAPH_TILE, GRAPH_PR_BLOCKS): the extension's own values on a GPU
    machine, the Python constants above on the CPU tier."""
    if torch.cuda.is_available():
        return tuple(int(c) for c in ext().graph_caps())
    return GRAPH_TILE, GRAPH_PR_BLOCKS


def _graph_propagate_composed(offsets, src, x, op, dst=None):
    """The contract of graph_propagate composed from the project's other
    ops: materialise the gathered column, reduce it by the destination of
    every edge, scatter the rows that have edges.  src must be in range.
    dst = the sorted destination column when the caller keeps it (the
    benchmark does); it is rebuilt from offsets otherwise."""
    n, m = x.numel(), src.numel()
    out = torch.full((n,), 0.0 if x.dtype == torch.float64
                     else _GRAPH_IDENTITY[op], dtype=x.dtype, device=x.device)
    if n == 0 or m == 0:
        return out
    if dst is None:
        dst = torch.repeat_interleave(
            torch.arange(n, device=x.device), offsets[1:] - offsets[:-1],
            output_size=m)
    vals = x.index_select(0, src)
    uk, uv, _, _ = reduce_by_key_sorted(dst, vals, op=op)
    out[uk] = uv
    return out


def graph_propagate(offsets: torch.Tensor, src: torch.Tensor,
                    x: torch.Tensor, op: str = "sum") -> torch.Tensor:
    """out[v] = the sum, minimum or maximum of x[src[e]] over the in-edges
    offsets[v] <= e < offsets[v + 1] of row v.  offsets is i64[n + 1], the
    CSR row starts by destination (non-decreasing, offsets[0] = 0,
    offsets[n] = m; the caller's contract, not checked); src is int32[m],
    dense source ids in [0, n); x is i64 or f64 [n].  The result has the
    dtype and length of x and the inputs are never written.  No host sync;
    fewer than 2^31 edges and rows.

    "sum": i64 wraps modulo 2^64, f64 is IEEE.  "min" / "max": i64 only
    (signed); f64 raises TypeError.  An empty row gives the identity: 0,
    INT64_MAX or INT64_MIN.  A src entry outside [0, n) contributes the
    identity and is never dereferenced; offsets that break the contract give
    an unspecified but defined answer and never address outside src, x or
    out.

    Device path (ops/hip/graph.hip): tiles of GRAPH_TILE edges whatever the
    rows look like, so a hub is spread over many blocks and empty rows cost
    nothing; rows inside a tile are finished there, rows across tiles by a
    one-block scan of the tile aggregates.  No atomics: the association of
    a row's f64 sum depends on (offsets, m) alone, so two calls return the
    same bits.  The CPU tier sums f64 rows by math.fsum, so it may differ
    from the device in the last bits.

    MR_GRAPH_COMPOSED=1 (read per call) runs the same contract composed
    from index_select, reduce_by_key_sorted and a scatter instead, for A/B
    and as an oracle on the device; its f64 sums go through atomics and are
    not reproducible, and it needs every src in range."""
    if op not in _SEG_SCAN_OPS:
        raise ValueError(f"op must be 'sum', 'min' or 'max', got {op!r}")
    v, f64 = _group_vals_i64(x, "x")
    if f64 and op != "sum":
        raise TypeError(f"graph {op} needs int64 values, got {x.dtype}")
    if offsets.dtype != torch.int64:
        raise TypeError("offsets must be int64")
    if src.dtype != torch.int32:
        raise TypeError(f"src must be int32, got {src.dtype}")
    if offsets.numel() != x.numel() + 1:
        raise ValueError(
            f"offsets must hold {x.numel() + 1} entries for {x.numel()} "
            f"rows, got {offsets.numel()}")
    _group_check_rows(x.numel())
    _group_check_rows(src.numel())
    if not offsets.is_cuda and not src.is_cuda and not x.is_cuda:
        from . import _cpu
        return _cpu.graph_propagate(offsets, src, x, op)
    if os.environ.get("MR_GRAPH_COMPOSED", "0") == "1":
        return _graph_propagate_composed(offsets, src, x, op)
    return ext().graph_propagate(offsets.contiguous(), src.contiguous(),
                                 v.contiguous(), _SEG_SCAN_OPS[op],
                                 f64).view(x.dtype)


def pagerank_update(sums: torch.Tensor, old: torch.Tensor,
                    inv_out: torch.Tensor, damping: float,
                    dangling: torch.Tensor):
    """One PageRank update over the n nodes, all f64:
    new = (1 - d) / n + d * (sums + dangling / n), contrib = new * inv_out
    (inv_out is 1 / outdeg, 0 for a node without out-edges).  -> (new,
    contrib, partials): partials is f64[blocks, 2] whose column 0 sums to
    |new - old|_1 and column 1 to the rank held by the nodes with inv_out
    == 0 (the next iteration's dangling mass); torch.sum over the block axis
    finishes them in a fixed order.  dangling is a 0-dim tensor on the
    device of sums, so iterations chain with no host sync."""
    for name, t in (("sums", sums), ("old", old), ("inv_out", inv_out),
                    ("dangling", dangling)):
        if t.dtype != torch.float64:
            raise TypeError(f"{name} must be float64, got {t.dtype}")
    if old.numel() != sums.numel() or inv_out.numel() != sums.numel():
        raise ValueError("one old rank and one inv_out per sum required")
    if dangling.numel() != 1:
        raise ValueError("dangling must hold one value")
    if not sums.is_cuda and not old.is_cuda and not inv_out.is_cuda:
        from . import _cpu
        return _cpu.pagerank_update(sums, old, inv_out, float(damping),
                                    dangling)
    new, contrib, partials = ext().pagerank_update(
        sums.contiguous(), old.contiguous(), inv_out.contiguous(),
        float(damping), dangling.reshape(1))
    return new, contrib, partials
