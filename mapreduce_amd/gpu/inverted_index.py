"""Inverted index: word -> sorted list of (doc id, term frequency).

The value-list-heavy workload of BASELINE.json (stresses the all-to-all
shuffle with large value lists).  Map emits (word, doc); the "reduce"
is a group-by — with the sort-once design the doc list of a key IS its
contiguous segment, so reduce is segment bookkeeping, not computation
(SURVEY.md K4 -> K1+K5).

Pipeline per rank (GPU):
  tokenize_spill_composite -> (wordhash ^ splitmix64(doc), pos) with the
    doc id binary-searched from the split offsets IN-KERNEL
  bucketize + per-bucket LDS count -> unique (word, doc) postings with
    term frequencies (aggregation BEFORE any sort: ~7x fewer elements)
  recover (doc, wordhash) from exemplar positions; sort by doc bits then
    stable by wordhash -> doc lists ordered within each word
  [world > 1] exchange by wordhash partition (mulhi), re-sort, re-merge
  segment by wordhash -> doc-list offsets per word + exemplar bytes
  [positions=True, single rank] the occurrence stream is kept as well:
    token_ordinals -> (doc, ordinal within doc) per occurrence; sorted by
    (doc, ord) then stable by wordhash it lies in posting order, so the
    positions of posting j are the slice pos_offsets[j] + [0, tf[j])
(CPU tier keeps the sort-first reference shape.)
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import List, NamedTuple, Optional, Tuple

import torch

from .. import ops
from . import dist as dx


class SearchResult(NamedTuple):
    hits: int    # documents matching the query (not capped by k)
    docs: list   # [(doc, score), ...] best first, at most k


@dataclass
class InvertedIndexResult:
    keys: torch.Tensor        # i64 u64-hash bits, sorted, one per word
    doc_offsets: torch.Tensor  # i64[nwords+1] into docs/tf
    docs: torch.Tensor        # i64: doc ids, sorted within each word
    tf: torch.Tensor          # i64: term frequency of (word, doc)
    pos: torch.Tensor         # exemplar (off<<16|len) into blob_src
    blob_src: torch.Tensor    # u8
    hash_kind: str = "wordhash64"  # GPU tier: wordhash64 (ops/hip
                                   # common.h); CPU test tier: fnv1a64
                                   # (ops/_cpu.py tokenize_words)
    ndocs: Optional[int] = None  # documents indexed (the N of tf-idf);
                                 # None when the job ran on several ranks
    # positional layer (InvertedIndexJob(..., positions=True)), else None:
    # posting j owns positions[pos_offsets[j]:pos_offsets[j + 1]], the
    # ascending 0-based token ordinals of the word within the document
    positions: Optional[torch.Tensor] = None    # i32[occurrences]
    pos_offsets: Optional[torch.Tensor] = None  # i64[postings + 1]

    def to_host(self):
        lens, blob = ops.extract_words(self.blob_src, self.pos)
        raw = bytes(blob.cpu().numpy().tobytes())
        offs = self.doc_offsets.cpu().tolist()
        docs = self.docs.cpu().tolist()
        tf = self.tf.cpu().tolist()
        out = {}
        off = 0
        for i, L in enumerate(lens.cpu().tolist()):
            w = raw[off:off + L]
            off += L
            out[w] = list(zip(docs[offs[i]:offs[i + 1]],
                              tf[offs[i]:offs[i + 1]]))
        return out

    def lex_perm(self) -> torch.Tensor:
        """Device permutation putting the words in lexicographic byte
        order (ops.lex_order over the exemplars), computed once and
        cached.  Hash order stays the arrays' native order."""
        perm = getattr(self, "_lex_perm", None)
        if perm is None:
            perm = ops.lex_order(self.blob_src, self.pos)
            self._lex_perm = perm
        return perm

    def _rows(self, idx: torch.Tensor):
        """[(word, postings)] for the word rows idx, in idx order; only
        those rows' exemplars and postings cross to the host."""
        if idx.numel() == 0:
            return []
        lens, blob = ops.extract_words(self.blob_src,
                                       self.pos.index_select(0, idx))
        raw = bytes(blob.cpu().numpy().tobytes())
        o0 = self.doc_offsets.index_select(0, idx)
        cnt = self.doc_offsets.index_select(0, idx + 1) - o0
        # flat posting indices of the selected rows, row after row
        ends = torch.cumsum(cnt, 0)
        row = torch.repeat_interleave(
            torch.arange(idx.numel(), device=idx.device), cnt)
        flat = (torch.arange(row.numel(), device=idx.device)
                - (ends - cnt).index_select(0, row)
                + o0.index_select(0, row))
        docs = self.docs.index_select(0, flat).cpu().tolist()
        tf = self.tf.index_select(0, flat).cpu().tolist()
        out = []
        off = a = 0
        for L, c in zip(lens.cpu().tolist(), cnt.cpu().tolist()):
            out.append((raw[off:off + L],
                        list(zip(docs[a:a + c], tf[a:a + c]))))
            off += L
            a += c
        return out

    def pair_iterator(self, order: str = "hash"):
        """The reference finalfn contract (server.lua:360-385): yields
        (word, postings-list) pairs; order="lex" walks the device
        lexicographic permutation (the reference's sorted-result
        guarantee) instead of sorting on the host."""
        if order == "lex":
            items = self._rows(self.lex_perm())
        else:
            items = self.to_host().items()
        for w, postings in items:
            yield w, postings

    def prefix(self, p, limit: Optional[int] = None):
        """[(word, postings)] for every word starting with p, in
        lexicographic order (the first `limit` of them): the range
        [lower_bound(p), lower_bound(succ(p))) of lex_perm()."""
        if isinstance(p, str):
            p = p.encode()
        perm = self.lex_perm()
        lo, hi = ops.lex_prefix_range(self.blob_src, self.pos, perm, p)
        if limit is not None:
            hi = min(hi, lo + max(0, int(limit)))
        return self._rows(perm[lo:hi])

    def _signed_keys(self) -> torch.Tensor:
        """keys hold u64 bit patterns; XOR the sign bit maps unsigned
        order onto int64 order so torch.searchsorted works (cached)."""
        sk = getattr(self, "_sk", None)
        if sk is None:
            sk = self.keys ^ (-1 << 63)
            self._sk = sk
        return sk

    def _term_hash(self, word) -> int:
        """The word's key as the i64 bit pattern stored in keys."""
        if isinstance(word, str):
            word = word.encode()
        if self.hash_kind == "wordhash64":
            from mapreduce_amd.utils.tuple import wordhash64
            k = wordhash64(word)
        else:  # fnv1a64 (CPU test tier, ops/_cpu.py tokenize_words)
            k = 0xCBF29CE484222325
            for b in word:
                k = ((k ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
        return k - (1 << 64) if k >= (1 << 63) else k

    def lookup(self, word) -> list:
        """Serve one word's postings [(doc, tf), ...] — O(log n) binary
        search on the hash-sorted index, no host materialization."""
        ki = self._term_hash(word)
        sk = self._signed_keys()
        q = torch.tensor([ki ^ (-1 << 63)], dtype=torch.int64,
                         device=sk.device)
        i = int(torch.searchsorted(sk, q).item())
        if i >= self.keys.numel() or int(self.keys[i].item()) != ki:
            return []
        o0 = int(self.doc_offsets[i].item())
        o1 = int(self.doc_offsets[i + 1].item())
        return list(zip(self.docs[o0:o1].cpu().tolist(),
                        self.tf[o0:o1].cpu().tolist()))

    def idf_weights(self, ndocs: Optional[int] = None) -> torch.Tensor:
        """i64[nwords] fixed-point idf, w = rint(65536 * ln(1 + N / df)),
        df = the word's document count.  Computed on the host in f64 from
        one readback of df and uploaded, so both tiers hold the same
        integers; cached per N."""
        n = self.ndocs if ndocs is None else ndocs
        if n is None:
            raise ValueError(
                "tfidf scoring needs the document count: this index has no "
                "ndocs (built on several ranks); pass ndocs=")
        n = int(n)
        cache = self.__dict__.setdefault("_idf", {})
        w = cache.get(n)
        if w is None:
            import numpy as np
            df = getattr(self, "_df_host", None)
            if df is None:
                df = np.diff(self.doc_offsets.cpu().numpy()).astype(
                    np.float64)
                self._df_host = df
            wh = np.rint(65536.0 * np.log(1.0 + n / df)).astype(np.int64)
            w = torch.from_numpy(wh).to(self.keys.device)
            cache[n] = w
        return w

    @staticmethod
    def _terms(query) -> list:
        """A query as a list of distinct byte-string terms: str/bytes are
        split on whitespace, sequences taken as they are; duplicates
        dropped, first occurrence kept."""
        if isinstance(query, (str, bytes)):
            query = query.split()
        out, seen = [], set()
        for t in query:
            if isinstance(t, str):
                t = t.encode()
            t = bytes(t)
            if t not in seen:
                seen.add(t)
                out.append(t)
        return out

    def search_batch(self, queries, mode: str = "and", k: int = 10,
                     scoring: str = "tf", ndocs: Optional[int] = None
                     ) -> List[SearchResult]:
        """Ranked search of many queries at once: one ops.postings_search
        call, two uploads (term hashes, offsets) and one readback whatever
        the number of queries.  See search()."""
        if scoring == "tf":
            weights = None
        elif scoring == "tfidf":
            weights = self.idf_weights(ndocs)
        else:
            raise ValueError(
                f"scoring must be 'tf' or 'tfidf', got {scoring!r}")
        hashes, offs = [], [0]
        for query in queries:
            hashes.extend(self._term_hash(t) for t in self._terms(query))
            offs.append(len(hashes))
        out = ops.postings_search(
            self.keys, self.doc_offsets, self.docs, self.tf, weights,
            torch.tensor(hashes, dtype=torch.int64),
            torch.tensor(offs, dtype=torch.int64), k, mode)
        d, s, n, h = out
        k = d.shape[1]
        host = torch.cat([d, s, n[:, None], h[:, None]], dim=1).cpu().tolist()
        return [SearchResult(row[2 * k + 1],
                             list(zip(row[:row[2 * k]],
                                      row[k:k + row[2 * k]])))
                for row in host]

    def search(self, terms, mode: str = "and", k: int = 10,
               scoring: str = "tf", ndocs: Optional[int] = None
               ) -> SearchResult:
        """Documents matching a multi-term query, best first.

        terms: a str/bytes split on whitespace, or a sequence of terms.
        mode "and": documents holding every term; "or": at least one.
        scoring "tf": score = sum of the matching terms' frequencies;
        "tfidf": each weighted by idf_weights(ndocs).  Equal scores order
        by ascending doc id.  -> SearchResult(hits, [(doc, score), ...])
        with at most k documents; hits counts all matches.  This rank's
        index only (words are hash-partitioned across ranks)."""
        return self.search_batch([terms], mode=mode, k=k, scoring=scoring,
                                 ndocs=ndocs)[0]

    @staticmethod
    def _phrase_terms(query) -> list:
        """A phrase as its ordered byte-string terms: split like _terms,
        but duplicates stay ("a a b" is three terms)."""
        if isinstance(query, (str, bytes)):
            query = query.split()
        return [bytes(t.encode() if isinstance(t, str) else t)
                for t in query]

    def _need_positions(self) -> None:
        if self.positions is None or self.pos_offsets is None:
            raise ValueError(
                "this index has no positional layer; build it with "
                "InvertedIndexJob(..., positions=True)")

    def phrase_batch(self, queries, k: int = 10) -> List[SearchResult]:
        """Exact-phrase search of many queries at once: one
        ops.postings_phrase call, two uploads (term hashes, offsets) and
        one readback whatever the number of queries.  See phrase()."""
        self._need_positions()
        hashes, offs = [], [0]
        for query in queries:
            hashes.extend(self._term_hash(t)
                          for t in self._phrase_terms(query))
            offs.append(len(hashes))
        d, s, n, h = ops.postings_phrase(
            self.keys, self.doc_offsets, self.docs, self.tf,
            self.pos_offsets, self.positions,
            torch.tensor(hashes, dtype=torch.int64),
            torch.tensor(offs, dtype=torch.int64), k)
        k = d.shape[1]
        host = torch.cat([d, s, n[:, None], h[:, None]], dim=1).cpu().tolist()
        return [SearchResult(row[2 * k + 1],
                             list(zip(row[:row[2 * k]],
                                      row[k:k + row[2 * k]])))
                for row in host]

    def phrase(self, terms, k: int = 10) -> SearchResult:
        """Documents holding the terms next to each other, in this order.

        terms: a str/bytes split on whitespace, or a sequence of terms;
        repeated terms count ("a a" needs two consecutive a).  Words are
        adjacent when their token ordinals are, whatever whitespace lies
        between them.  score = how often the phrase occurs in the document;
        equal scores order by ascending doc id.  -> SearchResult(hits,
        [(doc, score), ...]) with at most k documents.  Needs an index
        built with positions=True (ValueError otherwise)."""
        return self.phrase_batch([terms], k=k)[0]

    def lookup_positions(self, word) -> list:
        """One word's positional postings [(doc, [ord, ...]), ...]: the
        token ordinals of every occurrence, ascending, per document."""
        self._need_positions()
        ki = self._term_hash(word)
        sk = self._signed_keys()
        q = torch.tensor([ki ^ (-1 << 63)], dtype=torch.int64,
                         device=sk.device)
        i = int(torch.searchsorted(sk, q).item())
        if i >= self.keys.numel() or int(self.keys[i].item()) != ki:
            return []
        o0, o1 = self.doc_offsets[i:i + 2].cpu().tolist()
        po = self.pos_offsets[o0:o1 + 1].cpu().tolist()
        docs = self.docs[o0:o1].cpu().tolist()
        flat = self.positions[po[0]:po[-1]].cpu().tolist()
        return [(d, flat[a - po[0]:b - po[0]])
                for d, a, b in zip(docs, po[:-1], po[1:])]


_SM64_C0 = 0x9E3779B97F4A7C15 - (1 << 64)
_SM64_C1 = 0xBF58476D1CE4E5B9 - (1 << 64)
_SM64_C2 = 0x94D049BB133111EB - (1 << 64)


def _lsr(x: torch.Tensor, k: int) -> torch.Tensor:
    """Logical shift right on int64 bit patterns (torch >> is arithmetic)."""
    return (x >> k) & ((1 << (64 - k)) - 1)


def splitmix64_t(x: torch.Tensor) -> torch.Tensor:
    """SplitMix64 on int64 bit patterns (wrapping mul) — must match
    utils.tuple.splitmix64; unit-tested against it."""
    z = x + _SM64_C0
    z = (z ^ _lsr(z, 30)) * _SM64_C1
    z = (z ^ _lsr(z, 27)) * _SM64_C2
    return z ^ _lsr(z, 31)


class InvertedIndexJob:
    def __init__(self, device, group=None, doc_base: int = 0,
                 positions: bool = False):
        self.device = torch.device(device)
        self.group = group
        self.rank, self.world = dx.world_info(group)
        self.doc_base = doc_base  # global id of this rank's first doc
        # also keep every occurrence's token ordinal (phrase search);
        # single rank only
        self.positions = bool(positions)

    def _positional_layer(self, text, starts, k2, p, tf, doc_bits: int):
        """GPU: the occurrence stream (composite key, pos) without pads ->
        (positions i32[nocc], pos_offsets i64[np + 1]) in posting order.
        Occurrences are sorted by (doc, ord) over the bits that exist, then
        stably by wordhash — the order of the postings, whose tf are the
        slice lengths."""
        doc, ordn = ops.token_ordinals(text, p, starts)
        doc = doc + self.doc_base
        wh = k2 ^ splitmix64_t(doc)
        comp = (doc << 32) | ordn.to(torch.int64)
        comp, wh = ops.sort_by_key(comp, wh, bits=32 + doc_bits)
        wh, comp = ops.sort_by_key(wh, comp, bits=64)
        return self._finish_positions(
            (comp & 0xFFFFFFFF).to(torch.int32), tf)

    @staticmethod
    def _finish_positions(positions, tf):
        pos_offsets = torch.zeros(tf.numel() + 1, dtype=torch.int64,
                                  device=tf.device)
        torch.cumsum(tf, 0, out=pos_offsets[1:])
        total = int(pos_offsets[-1].item())
        assert total == positions.numel(), (
            f"positional layer: {positions.numel()} occurrences for "
            f"term frequencies summing to {total}")
        return positions, pos_offsets

    def _sort_by_doc_then_hash(self, h, d, p, max_doc: int = 1 << 30):
        # LSD composite: stable sorts, least-significant key first; doc
        # ids are small, so the doc pass sorts only the bits that exist
        d1, h1, p1 = (d, h, p)
        if h.is_cuda:
            doc_bits = max(8, int(max_doc).bit_length())
            d1, h1, p1 = ops.sort_by_key(d, h, p, bits=doc_bits)
            h2, d2, p2 = ops.sort_by_key(h1, d1, p1, bits=64)
        else:
            d1, h1, p1 = ops.sort_by_key(d, h, p, bits=64)
            h2, d2, p2 = ops.sort_by_key(h1, d1, p1, bits=64)
        return h2, d2, p2

    def _segment_pairs(self, h, d, p):
        """(hash, doc) grouped -> unique (hash, doc, tf, first pos)."""
        # composite key for boundary detection: (hash, doc) change points.
        # build u64 composite via xor-mix is unsafe; detect heads where
        # hash or doc changes — reuse head_flags on each and OR.
        if h.numel() == 0:
            z = h
            return h, d, torch.zeros_like(h), p
        if h.is_cuda:
            fh = ops.ext().head_flags(h)
            fd = ops.ext().head_flags(d)
            flags = (fh | fd)
            seg = torch.cumsum(flags, 0)
            nseg = int(seg[-1].item())
            uh, tf = ops.ext().seg_reduce_i64(
                h, torch.empty(0, dtype=torch.int64, device=h.device), seg,
                nseg)
            ud = ops.ext().seg_first_u64(d, seg, nseg)
            up = ops.ext().seg_first_u64(p, seg, nseg)
            return uh, ud, tf, up
        import numpy as np
        hn = h.numpy().view(np.uint64)
        dn = d.numpy()
        heads = np.ones(len(hn), dtype=bool)
        heads[1:] = (hn[1:] != hn[:-1]) | (dn[1:] != dn[:-1])
        idx = np.flatnonzero(heads)
        tf = np.diff(np.append(idx, len(hn)))
        from mapreduce_amd.ops._cpu import _from_u64
        return (_from_u64(hn[idx]), torch.from_numpy(dn[idx]),
                torch.from_numpy(tf.astype(np.int64)), p[torch.from_numpy(idx)])

    def run(self, text: torch.Tensor,
            splits: Optional[List[Tuple[int, int]]] = None
            ) -> InvertedIndexResult:
        dev = self.device
        if self.positions:
            import os
            if self.world > 1 or dx.force_collectives():
                raise NotImplementedError(
                    "positions=True builds a single-rank index: the "
                    "exchange carries (word, doc, tf), not occurrences")
            if dev.type == "cuda" and \
                    os.environ.get("MR_II_CACHE", "0") == "1":
                raise ValueError(
                    "MR_II_CACHE=1 absorbs occurrences into the LDS cache; "
                    "positions=True needs every occurrence")
            if text.numel() >= 2 ** 31:
                raise ValueError(
                    f"positions=True: text of {text.numel()} bytes; "
                    "token ordinals are 32-bit")
        positions = pos_offsets = None
        if splits is None:
            splits = [(0, int(text.numel()))]
        starts = torch.tensor([s for s, _ in splits] + [splits[-1][1]],
                              device=dev, dtype=torch.int64)
        max_doc = self.doc_base + len(splits) + 1
        doc_bits = max(8, int(max_doc).bit_length())
        if dev.type == "cuda":
            import os
            # ---- aggregate BEFORE sorting: the tokenizer emits composite
            # (word, doc) keys directly (doc looked up in-kernel from the
            # split offsets; wordhash ^ splitmix64(doc)), which the
            # bucketize + LDS-count machinery collapses to unique postings
            # (~7x fewer elements for the radix passes; sorting the raw
            # stream measured ~20 ms of a 26 ms job).  doc is recoverable
            # from the exemplar position, so wordhash = k2 ^
            # splitmix64(doc) reverses the composite.  HT_EMPTY chunk
            # padding stops at the bucketize (radix_bucketize skip mode;
            # 8.06 vs 8.52 ms/job with the pads carried through).
            # MR_II_CACHE=1: LDS-cached composite tokenizer — MEASURED
            # SLOWER (9.16 vs 9.00 ms): the grid-stride tile mapping
            # spreads each block over ~30 tiles of DIFFERENT documents,
            # so (word, doc) composites go cold at every tile switch
            # (~55% miss vs wordcount's 30%) and the insert cost
            # outweighs the drain savings.  Default OFF (spill-all);
            # kept for the record.
            use_cache = os.environ.get("MR_II_CACHE", "0") == "1"
            table = ops.make_table(max(1 << 16, text.numel() // 36), dev)
            if use_cache:
                cap = text.numel() // 2 + 16 + 2048 * 4 * 2048
                opts = dict(dtype=torch.int64, device=dev)
                h = torch.empty(cap, **opts)
                pp = torch.empty(cap, **opts)
                c = torch.zeros(1, **opts)
                nw = torch.zeros(1, **opts)
                ops.ext().tokenize_cache_spill_composite(
                    text, 0, table.tkeys, table.tvals, table.texm, cap,
                    nw, h, pp, c, starts, self.doc_base)
                n = int(c.item())
                if n > cap:
                    raise RuntimeError(
                        f"spill overflow: {n} reserved > {cap}")
                k2, p = h[:n], pp[:n]
            else:
                cap = text.numel() // 2 + 16 + 2048 * 4 * 512
                k2, p, c, nw = ops.ext().tokenize_spill_composite(
                    text, 0, cap, starts, self.doc_base)
                n = int(c.item())
                if n > cap:
                    raise RuntimeError(
                        f"spill overflow: {n} reserved > {cap}")
                k2, p = k2[:n], p[:n]
            if n:
                hk, pv, bucket_off = ops.ext().radix_bucketize(
                    k2, p, 56, True)
                # r2 joint re-sweep on the idx32 tree (the knobs
                # INTERACT): 1024 slots x 128 slices = 8.48 ms vs the
                # old 2048x64 = 8.91 (-4.8%).  Full grid: slices at
                # 1024 slots: 32=11.0, 48=9.49, 64=8.84, 96=8.53,
                # 128=8.48, 192=8.55, 256=8.65, 512=9.04; 512 slots x
                # 256 ties (8.49).  Smaller tables buy occupancy,
                # which more slices then convert into block-level
                # parallelism — the overflow ht_add fallback stays
                # cold because distinct/slice shrinks with slices.
                slices = int(os.environ.get("MR_II_SLICES", "128"))
                ops.ext().bucket_count(hk, pv, bucket_off, 256, slices,
                                       table.tkeys, table.tvals,
                                       table.texm, 0, 1024)
            uk2, tf, upos = table.extract()
            ud = torch.searchsorted(starts, upos >> 16, right=True) - 1
            ud = ud + self.doc_base
            uh = uk2 ^ splitmix64_t(ud)
            # output order: doc within word, words by hash
            d1, h1, tf1, p1 = ops.sort_by_key(ud, uh, tf, upos,
                                              bits=doc_bits)
            uh, ud, tf, up = ops.sort_by_key(h1, d1, tf1, p1, bits=64)
            if self.positions:
                real = k2 != -1  # HT_EMPTY chunk padding of the spill
                positions, pos_offsets = self._positional_layer(
                    text, starts, k2[real], p[real], tf, doc_bits)
        else:
            h, p, n = ops.tokenize_words(text)
            byte_off = p >> 16
            d = torch.searchsorted(starts, byte_off, right=True) - 1
            d = d + self.doc_base
            h, d, p = self._sort_by_doc_then_hash(h, d, p, max_doc)
            uh, ud, tf, up = self._segment_pairs(h, d, p)
            if self.positions:
                # the tokenizer emits in text order and both sorts are
                # stable: occurrences already lie in (word, doc, ord) order
                _, ordn = ops.token_ordinals(text, p, starts)
                positions, pos_offsets = self._finish_positions(ordn, tf)

        blob_src = text
        if self.world > 1 or dx.force_collectives():
            counts_d = ops.partition_counts(uh, self.world)
            lens, blob = ops.extract_words(text, up)
            bnd = torch.cumsum(counts_d, 0)
            if lens.numel():
                lcs = torch.cumsum(lens, 0)
                cum = torch.where(
                    bnd > 0, lcs.index_select(0, (bnd - 1).clamp(min=0)),
                    torch.zeros_like(bnd))
                blob_counts_d = torch.cat([cum[:1], cum[1:] - cum[:-1]])
            else:
                blob_counts_d = torch.zeros_like(counts_d)
            packed = torch.cat([counts_d, blob_counts_d])
            recv_packed = dx.exchange_counts(packed, self.group)
            host = torch.stack([packed, recv_packed]).cpu()
            sc = host[0, :self.world].tolist()
            sb = host[0, self.world:].tolist()
            rc = host[1, :self.world].tolist()
            rb = host[1, self.world:].tolist()
            quad = torch.stack([uh, ud, tf, lens], dim=1).reshape(-1)
            rquad = dx.exchange(quad, [4 * c for c in sc],
                                [4 * c for c in rc], self.group)
            rquad = rquad.view(-1, 4)
            rh = rquad[:, 0].contiguous()
            rd = rquad[:, 1].contiguous()
            rtf = rquad[:, 2].contiguous()
            rlens = rquad[:, 3].contiguous()
            if dev.type == "cuda":
                # C5 overlap (BASELINE): blob all-to-all on a side
                # stream, concurrent with the composite re-sort below
                # (7.4M-posting sorts are the big local cost here —
                # exactly where the overlap pays; same issue order on
                # every rank keeps the communicator deterministic)
                ev = torch.cuda.Event()
                ev.record()
                side = getattr(self, "_side_stream", None)
                if side is None:
                    side = torch.cuda.Stream(dev)
                    self._side_stream = side
                side.wait_event(ev)
                with torch.cuda.stream(side):
                    rblob = dx.exchange(blob, sb, rb, self.group)
            else:
                rblob = dx.exchange(blob, sb, rb, self.group)
            roff = torch.cumsum(rlens, 0) - rlens
            rp = (roff << 16) | rlens
            # composite re-sort (carrying pos + tf via an index payload) +
            # merge duplicate (hash, doc) pairs arriving from several ranks
            idx = torch.arange(rh.numel(), device=dev, dtype=torch.int64)
            hs, ds, perm = self._sort_by_doc_then_hash(
                rh, rd, idx, (self.doc_base + len(splits) + 1) * self.world)
            ps = rp.index_select(0, perm)
            tfs = rtf.index_select(0, perm)
            if dev.type == "cuda":
                cur = torch.cuda.current_stream(dev)
                cur.wait_stream(self._side_stream)
                rblob.record_stream(cur)
            if hs.is_cuda and hs.numel():
                fh = ops.ext().head_flags(hs)
                fd = ops.ext().head_flags(ds)
                seg = torch.cumsum(fh | fd, 0)
                nseg = int(seg[-1].item())
                uh, stf = ops.ext().seg_reduce_i64(hs, tfs, seg, nseg)
                ud = ops.ext().seg_first_u64(ds, seg, nseg)
                up = ops.ext().seg_first_u64(ps, seg, nseg)
                tf = stf
            else:
                import numpy as np
                hn = hs.numpy().view(np.uint64)
                dn = ds.numpy()
                heads = np.ones(len(hn), dtype=bool)
                if len(hn):
                    heads[1:] = (hn[1:] != hn[:-1]) | (dn[1:] != dn[:-1])
                idx2 = np.flatnonzero(heads)
                from mapreduce_amd.ops._cpu import _from_u64
                seg_id = np.cumsum(heads) - 1
                sums = np.zeros(len(idx2), dtype=np.int64)
                np.add.at(sums, seg_id, tfs.numpy())
                uh = _from_u64(hn[idx2])
                ud = ds[torch.from_numpy(idx2)]
                up = ps[torch.from_numpy(idx2)]
                tf = torch.from_numpy(sums)
            blob_src = rblob

        # per-word doc-list offsets + one exemplar per word
        seg, nwords = ops.segment_boundaries(uh)
        if nwords:
            if uh.is_cuda:
                wk, doc_counts = ops.ext().seg_reduce_i64(
                    uh, torch.empty(0, dtype=torch.int64, device=dev), seg,
                    nwords)
                wpos = ops.ext().seg_first_u64(up, seg, nwords)
            else:
                import numpy as np
                hn = uh.numpy().view(np.uint64)
                wkeys, idx3, cnts = np.unique(hn, return_index=True,
                                              return_counts=True)
                from mapreduce_amd.ops._cpu import _from_u64
                wk = _from_u64(wkeys)
                doc_counts = torch.from_numpy(cnts.astype(np.int64))
                wpos = up[torch.from_numpy(idx3)]
            offsets = torch.zeros(nwords + 1, dtype=torch.int64, device=dev)
            torch.cumsum(doc_counts, 0, out=offsets[1:])
        else:
            wk = uh
            wpos = up
            offsets = torch.zeros(1, dtype=torch.int64, device=dev)
        return InvertedIndexResult(
            keys=wk, doc_offsets=offsets, docs=ud, tf=tf, pos=wpos,
            blob_src=blob_src,
            hash_kind="wordhash64" if dev.type == "cuda" else "fnv1a64",
            ndocs=self.doc_base + len(splits) if self.world == 1 else None,
            positions=positions, pos_offsets=pos_offsets)
