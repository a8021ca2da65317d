"""Flagship fused word-count job — the BASELINE.json headline workload.

Per step (= one full MapReduce job over the rank's corpus):

  MAP+COMBINE   tokenize_v7 kernel over the coalesced splits: per-block
                LDS cache tables count the Zipf head in-kernel (the
                reference's mapfn emit + inline combiner job.lua:83-97);
                cache misses spill through the wave-chunked allocator,
                then one top-byte bucketize (radix_bucketize, which also
                drops the allocator's pads) + per-bucket LDS count
                (bucket_count) drains them — every per-word atomic is an
                LDS atomic.
  EXTRACT+SORT  table -> unique (hash, count, exemplar pos) sorted by hash,
                in one native op (ops.extract_sorted: table keys are
                unique, so MSD bins + rank counting; it also leaves the
                word lengths, their offsets and the blob size for the
                shuffle and for materialize()) — with mulhi partitioning,
                the sorted array is partition-contiguous.
  SHUFFLE       RCCL all-to-all of (hash, count, exemplar len/bytes) slices
                (C5/C6): one collective per array over the 7 xGMI links.
  REDUCE        sort the received runs + segmented reduce-by-key (K4->K1+K5),
                keeping the first exemplar per key.
  RESULT        per-rank sorted (hash, count, word) arrays; to_host()
                materializes (word -> count) for the finalfn boundary (C8).

The reducer here is the declared associative+commutative+idempotent sum
(examples/WordCount flags), which is exactly the reference's own fast-path
precondition (job.lua:264-274)."""

from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Tuple

import torch

from .. import ops
from . import dist as dx


# bucket_count slices per top-byte bucket (MR_BUCKET_SLICES overrides)
DEFAULT_BUCKET_SLICES = 16


@dataclass
class WordCountResult:
    keys: torch.Tensor      # i64 (u64 hash bits), sorted
    counts: torch.Tensor    # i64
    pos: torch.Tensor       # packed (off<<16|len) into blob_src
    blob_src: torch.Tensor  # u8 source for exemplar bytes
    nwords: int             # words processed by this rank this step
    hash_kind: str = "wordhash64"  # GPU tier: wordhash64; CPU test tier:
                                   # fnv1a64 (ops/_cpu.py tokenize_words)
    # what ops.extract_sorted already computed for (keys, counts, pos),
    # kept so materialize() need not recompute it: the contiguous
    # [keys | counts | lens] buffer, the exclusive scan of lens and its
    # end, and the blob_src they belong to (None: nothing cached)
    packed: Optional[torch.Tensor] = None
    offs: Optional[torch.Tensor] = None
    total_bytes: Optional[int] = None
    cache_src: Optional[torch.Tensor] = None

    def attach_ready_event(self, stream) -> None:
        """Producer on a SIDE stream (the job pipeline) marks when the
        result tensors are ready: consumers host-sync the event before
        reading.  A lazy host-synced event is used instead of
        enqueuing a wait on the caller's (default) stream: a
        null-stream wait op can fence other blocking streams, and the
        lazy form costs nothing on paths that never read the tensors
        (the bench hot loop).  Same-box pipe-vs-seq A/Bs vary +-2%
        box to box either way; the race fix itself is what matters
        (was a 1-in-3 suite flake)."""
        import torch
        ev = torch.cuda.Event()
        ev.record(stream)
        self._ready = ev

    def _wait_ready(self) -> None:
        ev = getattr(self, "_ready", None)
        if ev is not None:
            ev.synchronize()
            self._ready = None

    def key_of(self, word) -> int:
        """The int64 bit pattern this result keys `word` under (serving
        lookups must hash with the tier that built the result)."""
        if isinstance(word, str):
            word = word.encode()
        if self.hash_kind == "wordhash64":
            from mapreduce_amd.utils.tuple import wordhash64
            k = wordhash64(word)
        elif self.hash_kind == "fnv1a64":
            k = 0xCBF29CE484222325
            for b in word:
                k = ((k ^ b) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
        else:
            raise ValueError(
                f"results keyed with {self.hash_kind!r} do not support "
                "hash lookups")
        return k - (1 << 64) if k >= (1 << 63) else k

    def count_of(self, word) -> int:
        """Point lookup: one binary search on the hash-sorted keys."""
        self._wait_ready()
        ki = self.key_of(word)
        sk = self.keys ^ (-1 << 63)  # unsigned order -> int64 order
        q = torch.tensor([ki ^ (-1 << 63)], dtype=torch.int64,
                         device=sk.device)
        i = int(torch.searchsorted(sk, q).item())
        if i >= self.keys.numel() or int(self.keys[i].item()) != ki:
            return 0
        return int(self.counts[i].item())

    def lex_perm(self) -> torch.Tensor:
        """Device permutation putting the words in lexicographic byte
        order (ops.lex_order over the exemplars), computed once and
        cached.  Hash order stays the arrays' native order."""
        self._wait_ready()
        perm = getattr(self, "_lex_perm", None)
        if perm is None:
            perm = ops.lex_order(self.blob_src, self.pos)
            self._lex_perm = perm
        return perm

    def _ordered(self, order: str):
        """(keys, counts, pos) in the requested order."""
        if order != "lex":
            return self.keys, self.counts, self.pos
        perm = self.lex_perm()
        return (self.keys.index_select(0, perm),
                self.counts.index_select(0, perm),
                self.pos.index_select(0, perm))

    def _pairs(self, counts: torch.Tensor,
               pos: torch.Tensor) -> List[Tuple[bytes, int]]:
        lens, blob = ops.extract_words(self.blob_src, pos)
        raw = bytes(blob.cpu().numpy().tobytes())
        out = []
        off = 0
        for L, c in zip(lens.cpu().tolist(), counts.cpu().tolist()):
            out.append((raw[off:off + L], c))
            off += L
        return out

    def _prefix_range(self, p) -> Tuple[int, int]:
        if isinstance(p, str):
            p = p.encode()
        return ops.lex_prefix_range(self.blob_src, self.pos,
                                    self.lex_perm(), p)

    def count_prefix(self, p) -> int:
        """Number of distinct words starting with p: two device binary
        searches on the lexicographic permutation, no exemplar traffic."""
        lo, hi = self._prefix_range(p)
        return hi - lo

    def prefix(self, p, limit: Optional[int] = None
               ) -> List[Tuple[bytes, int]]:
        """All (word, count) with word starting with p, in lexicographic
        order (the first `limit` of them) — the range
        [lower_bound(p), lower_bound(succ(p))) of the permutation; only
        the selected exemplars cross to the host, as in topk."""
        lo, hi = self._prefix_range(p)
        if limit is not None:
            hi = min(hi, lo + max(0, int(limit)))
        if hi <= lo:
            return []
        idx = self.lex_perm()[lo:hi]
        return self._pairs(self.counts.index_select(0, idx),
                           self.pos.index_select(0, idx))

    def materialize(self, blocking: bool = True, order: str = "hash"):
        """Deliver the job's results to host memory (the analogue of the
        reference writing result.P<p> files + the server reading them,
        C7/C8): raw key/count arrays + the packed exemplar word bytes.
        One packed i64 D2H + one u8 D2H into cached pinned buffers.
        order="lex" returns the same four arrays permuted into
        lexicographic word order (lex_perm) on the device first.

        blocking=False enqueues the copies on the current stream and
        returns immediately — the next job's kernels overlap the D2H, and
        any later stream synchronize guarantees the host buffers are
        complete (how bench.py uses it).  Returns (keys_cpu, counts_cpu,
        lens_cpu, blob_cpu)."""
        self._wait_ready()  # no-op for the producer's own in-stream call
        n = self.keys.numel()
        if (order == "hash" and self.packed is not None
                and self.cache_src is self.blob_src
                and self.packed.numel() == 3 * n):
            # extract_sorted left the packed buffer, the offsets and the
            # blob size: one gather, no scan, no sync, no cat
            packed = self.packed
            blob = ops.gather_words(self.blob_src, self.pos, self.offs,
                                    self.total_bytes)
        else:
            keys, counts, pos = self._ordered(order)
            lens, blob = ops.extract_words(self.blob_src, pos)
            packed = torch.cat([keys, counts, lens])
        if packed.is_cuda:
            host = torch.empty(packed.shape, dtype=packed.dtype,
                               pin_memory=True)
            host.copy_(packed, non_blocking=True)
            hblob = torch.empty(blob.shape, dtype=blob.dtype,
                                pin_memory=True)
            hblob.copy_(blob, non_blocking=True)
            if blocking:
                torch.cuda.current_stream(packed.device).synchronize()
        else:
            host, hblob = packed, blob
        return (host[:n], host[n:2 * n], host[2 * n:], hblob)

    def to_host(self, order: str = "hash") -> List[Tuple[bytes, int]]:
        """Materialize (word, count) pairs (C8).

        order="hash" (default): the engine's native u64-hash order —
        deterministic and grouped, the order the device arrays are in.
        order="lex": lexicographic by word bytes, matching the reference's
        sorted-result guarantee (job.lua:194, server.lua:360-385) —
        counts and exemplars are permuted on the device (lex_perm) before
        extraction, so the host never sorts."""
        self._wait_ready()
        _, counts, pos = self._ordered(order)
        return self._pairs(counts, pos)

    def pair_iterator(self, order: str = "hash"):
        """The reference finalfn contract (server.lua:360-385): yields
        (key, values) with values a list — here the reduced [count] —
        so a host-tier finalfn consumes a GPU-tier result unchanged.
        order as in to_host ("lex" = the reference's sorted guarantee)."""
        for w, c in self.to_host(order=order):
            yield w, [c]

    def topk(self, k: int) -> List[Tuple[bytes, int]]:
        """The k most frequent words, descending — device-side torch.topk
        over counts, then only those k exemplars cross to the host (a
        serving shortcut the reference would pay a full result read for)."""
        self._wait_ready()
        n = self.counts.numel()
        k = min(k, n)
        if k == 0:
            return []
        cnt, idx = torch.topk(self.counts, k)
        return self._pairs(cnt, self.pos.index_select(0, idx))


class WordCountJob:
    """mode:
      "streaming" (GPU default) — tokenize_cache_spill -> top-byte radix
        bucketize -> per-bucket LDS count (all per-word atomics in LDS);
      "fused" — tokenize straight into the global hash table (slower on
        Zipf text: per-word probes are L2-latency-bound; kept for A/B and
        as the low-memory path)."""

    def __init__(self, device, vocab_estimate: int = 1 << 18, group=None,
                 mode: str = "auto", timing: bool = False):
        self.device = torch.device(device)
        self.group = group
        self.rank, self.world = dx.world_info(group)
        self.vocab_estimate = vocab_estimate
        if mode == "auto":
            mode = "streaming" if self.device.type == "cuda" else "fused"
        self.mode = mode
        self.table = ops.make_table(vocab_estimate, self.device)
        self._nwords = torch.zeros(1, dtype=torch.int64, device=self.device)
        # per-phase tracing (the job-document timestamps of job.lua:117-152
        # in HIP-event form; stats format parity with server.lua:557-602);
        # on CPU devices wall-clock marks keep the same stats shape
        self.timing = timing
        self._hip_events = timing and self.device.type == "cuda"
        self.last_phase_ms: dict = {}
        self._events: list = []
        # rounds the last shuffle used (>1 = skew guard chunked it)
        self.last_shuffle_rounds = 1

    def _mark(self, name: str) -> None:
        if not self.timing:
            return
        if self._hip_events:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
        else:
            import time
            ev = time.perf_counter()
        self._events.append((name, ev))

    def _collect_timing(self) -> None:
        if not self.timing or len(self._events) < 2:
            return
        if self._hip_events:
            self._events[-1][1].synchronize()
        out = {}
        for (n0, e0), (n1, e1) in zip(self._events, self._events[1:]):
            out[n1] = (e0.elapsed_time(e1) if self._hip_events
                       else (e1 - e0) * 1000.0)
        self.last_phase_ms = out
        self._events = []

    def reset(self, vocab_estimate: int = 0):
        self.table = ops.make_table(vocab_estimate or self.vocab_estimate,
                                    self.device)
        self._nwords.zero_()

    # ---------------- claimable phase API (used by gpu.runner) -----------
    # begin_map() -> map_split(s, e) per claimed job -> finish_map() ->
    # shuffle_reduce() — run() composes these; the cluster runner drives
    # them under control-plane job claims.

    def begin_map(self, text: torch.Tensor,
                  expected_launches: int = 1) -> None:
        """expected_launches: how many map_split launches this job will
        issue.  The wave-chunked spill allocator pads chunk tails PER
        LAUNCH (grid is capped at 2048 blocks x 4 waves, each wave may
        strand one partial chunk), so the slack must scale with the
        launch count — measured: 16 chunked launches over Europarl
        reserve ~256M slots vs the 1-launch cap's 143M (spill
        overflow).  The runner coalesces contiguous splits into one
        launch; chunked-staging callers pass their chunk count."""
        self.reset()
        self._text = text
        self._events = []
        self._mark("start")
        if self.mode == "streaming":
            opts = dict(dtype=torch.int64, device=self.device)
            # + slack for the wave-chunked spill allocator's padded chunk
            # tails (<= 2048 blocks x 4 waves x one 2048-entry chunk each)
            cap = (text.numel() // 2 + 16
                   + max(1, expected_launches) * 2048 * 4 * 2048)
            self._spill_h = torch.empty(cap, **opts)
            self._spill_p = torch.empty(cap, **opts)
            self._spill_c = torch.zeros(1, **opts)
            self._spill_cap = cap

    def map_split(self, s: int, e: int) -> None:
        """One map job: tokenize+combine bytes [s, e) of the corpus.
        Streaming mode appends cache misses to the shared spill arrays
        (atomic counter append composes across launches)."""
        if self.mode == "streaming":
            ops.ext().tokenize_cache_spill(
                self._text[s:e], s, self.table.tkeys, self.table.tvals,
                self.table.texm, self._spill_cap, self._nwords,
                self._spill_h, self._spill_p, self._spill_c)
        else:
            self.table.tokenize_count(self._text[s:e], s, self._nwords)

    def finish_map(self) -> int:
        """Drain the spill through bucketize + per-bucket LDS count.
        Returns the word count (the one host sync of the map phase)."""
        self._mark("map_tokenize")
        n = self._finish_map_inner()
        self._mark("map_combine")
        return n

    def _finish_map_inner(self) -> int:
        if self.mode == "streaming":
            import os
            slices = int(os.environ.get("MR_BUCKET_SLICES",
                                        DEFAULT_BUCKET_SLICES))
            # ONE packed D2H for both scalars (each .item() is a full
            # stream sync)
            both = torch.cat([self._spill_c, self._nwords]).cpu()
            nspill, n = int(both[0]), int(both[1])
            if nspill > self._spill_cap:
                # chunk reservations past the cap were dropped in-kernel;
                # unwritten tail slots would read as garbage keys — fail
                # loudly instead (sizing bug: grow the allocator slack)
                raise RuntimeError(
                    f"spill overflow: {nspill} reserved > cap "
                    f"{self._spill_cap}")
            if nspill:
                h = self._spill_h[:nspill]
                p = self._spill_p[:nspill]
                # the bucketize drops the allocator's HT_EMPTY chunk-tail
                # pads (~2.85M of 16.8M reserved slots on the bench
                # shape; they would all land in bucket 255) and returns
                # bucket_off from its native scan; hk/pv keep length
                # nspill, defined up to bucket_off[256]
                hk, pv, bucket_off = ops.ext().radix_bucketize(
                    h, p, 56, True)
                # 16 slices/bucket x 1024 LDS slots, re-swept without
                # the pad tail (profiles/drain_skip_r03.md): 8=1.349,
                # 16=1.307, 24=1.333, 32=1.334, 48=1.365, 64=1.388
                # ms/step; 2048 slots: 8=1.335, rising to 64=1.512.  The
                # old 64-slice optimum only kept bucket-255's pads off
                # the critical path; fewer slices cut the scattered
                # global flush atomics 3.97M -> 1.75M per job.  1024
                # slots = 20 KB = 8 blocks/CU (the kernel is occupancy/
                # latency bound, profiles/pmc_final_kernels.txt);
                # overflow degrades to per-element ht_add, never wrong.
                ops.ext().bucket_count(hk, pv, bucket_off, 256, slices,
                                       self.table.tkeys, self.table.tvals,
                                       self.table.texm, 0, 1024)
            self._spill_h = self._spill_p = None
            return n
        return int(self._nwords.item())

    @staticmethod
    def _coalesced(text: torch.Tensor, splits) -> bool:
        if not splits:
            return False
        prev_end = splits[0][0]
        for (s, e) in splits:
            if s != prev_end:
                return False
            prev_end = e
        return True

    def run(self, text: torch.Tensor,
            splits: Optional[List[Tuple[int, int]]] = None) -> WordCountResult:
        """One full job over this rank's corpus bytes."""
        if splits is None:
            splits = [(0, int(text.numel()))]
        # ---- MAP + COMBINE.  Map jobs (splits) sharing one contiguous
        # corpus buffer are coalesced into a single fused kernel launch:
        # a launch needs >>256 workgroups to fill the chip, and 197 small
        # launches serialize (measured 98% of step time before fusing).
        # Split boundaries are whitespace-aligned, so tokenization over the
        # coalesced range is byte-identical to per-split runs.
        # phase marks live inside the phase methods so the cluster
        # runner's claim-driven execution traces identically
        self.begin_map(text)
        if self._coalesced(text, splits):
            self.map_split(splits[0][0], splits[-1][1])
        else:
            for (s, e) in splits:
                self.map_split(s, e)
        nwords = self.finish_map()
        return self.shuffle_reduce(nwords)

    def _shuffle_budget_bytes(self) -> int:
        """Per-rank receive budget for one shuffle round.  MUST be
        deterministic and identical across ranks (all ranks derive the
        round count from it — disagreement would deadlock the
        collectives), so the auto value uses TOTAL device memory, never
        free memory.  `MR_SHUFFLE_BUDGET_BYTES` overrides (0 disables
        chunking); default on GPU is total HBM / 4 (72 GB on MI355X —
        receive + sort scratch + accumulator fit with headroom), and on
        the CPU test tier chunking runs only when the env forces it."""
        import os
        env = os.environ.get("MR_SHUFFLE_BUDGET_BYTES")
        if env is not None:
            return max(0, int(env))
        if self.device.type == "cuda":
            props = torch.cuda.get_device_properties(self.device)
            return int(props.total_memory) // 4
        return 0

    def _plan_shuffle_rounds(self, full: torch.Tensor) -> int:
        """Round count for the chunked shuffle (1 = single-shot).
        `full` is the host copy of exchange_counts_full's [i, seg, j]
        matrix (seg 0 = element counts, seg 1 = blob bytes), identical
        on every rank, so every rank computes the same answer.  The
        bound is the LARGEST rank's receive (the skewed partition's
        owner defines the round count for everyone — SURVEY.md §7
        "shuffle skew + memory budget")."""
        budget = self._shuffle_budget_bytes()
        if budget <= 0:
            return 1
        # 3 interleaved i64 arrays (key, count, len) + exemplar bytes
        need = (full[:, 0, :].sum(0) * 24 + full[:, 1, :].sum(0))
        worst = int(need.max().item())
        if worst <= budget:
            return 1
        # cap: even a pathological budget terminates; each round still
        # moves >= 1 element per (src, dst) pair
        return min((worst + budget - 1) // budget, 4096)

    def _chunked_shuffle_reduce(self, sk, sv, lens, blob, lcs,
                                full: torch.Tensor, rounds: int):
        """Bounded-memory shuffle: the all-to-all runs in `rounds`
        passes, each moving a 1/rounds slice of every partition segment,
        and each received slice is folded into a running reduced
        accumulator (sort + segmented reduce + blob compaction).  Exact
        for the declared associative+commutative reducer — the same
        property the reference's combiner fast path relies on
        (job.lua:264-274) — because count merging is order-free.  HBM
        high-water mark: one round's receive + the unique-key
        accumulator, instead of the full skewed partition (SURVEY.md §7;
        the reference never hits this because GridFS is unbounded)."""
        dev = self.device
        world, rank = self.world, self.rank
        send_c = full[rank, 0].tolist()
        # element boundaries: partition p, round r starts at
        # poff[p] + c_p * r // rounds  (host ints — no device sync)
        poff = [0]
        for c in send_c:
            poff.append(poff[-1] + c)
        ebnd = [[poff[p] + send_c[p] * r // rounds
                 for r in range(rounds + 1)] for p in range(world)]
        # byte offset of each element boundary: ecs[e] (start of element
        # e's exemplar bytes), with e == n mapping to total blob bytes
        total_b = int(blob.numel())
        ecs = torch.cat([lcs - lens,
                         torch.tensor([total_b], dtype=torch.int64,
                                      device=dev)])
        bidx = torch.tensor([e for row in ebnd for e in row],
                            dtype=torch.int64, device=dev)
        boff = ecs.index_select(0, bidx).cpu().view(world, rounds + 1)
        bbnd = boff.tolist()
        # per-round blob send sizes -> ONE packed counts exchange
        # (element counts per round need no exchange: every rank derives
        # them from `full`'s per-partition counts with the same formula)
        rb = torch.tensor(
            [bbnd[p][r + 1] - bbnd[p][r]
             for r in range(rounds) for p in range(world)],
            dtype=torch.int64, device=dev)
        recv_rb = (dx.exchange_counts(rb, self.group)
                   .cpu().view(rounds, world).tolist())
        cin = full[:, 0, rank].tolist()  # elements each source sends me
        tri2d = torch.stack([sk, sv, lens], dim=1)

        acc_k = torch.empty(0, dtype=torch.int64, device=dev)
        acc_v = torch.empty(0, dtype=torch.int64, device=dev)
        acc_p = torch.empty(0, dtype=torch.int64, device=dev)
        acc_blob = torch.empty(0, dtype=torch.uint8, device=dev)
        for r in range(rounds):
            sc = [ebnd[p][r + 1] - ebnd[p][r] for p in range(world)]
            rc = [cin[i] * (r + 1) // rounds - cin[i] * r // rounds
                  for i in range(world)]
            sb = [bbnd[p][r + 1] - bbnd[p][r] for p in range(world)]
            stri = torch.cat([tri2d[ebnd[p][r]:ebnd[p][r + 1]]
                              for p in range(world)]).reshape(-1)
            sblob = torch.cat([blob[bbnd[p][r]:bbnd[p][r + 1]]
                               for p in range(world)])
            rtri = dx.exchange(stri, [3 * c for c in sc],
                               [3 * c for c in rc], self.group).view(-1, 3)
            rblob = dx.exchange(sblob, sb, recv_rb[r], self.group)
            rlens = rtri[:, 2].contiguous()
            roff = torch.cumsum(rlens, 0) - rlens
            rpos = ((roff + int(acc_blob.numel())) << 16) | rlens
            # fold into the accumulator: counts add, first exemplar kept
            mk = torch.cat([acc_k, rtri[:, 0].contiguous()])
            mv = torch.cat([acc_v, rtri[:, 1].contiguous()])
            mp = torch.cat([acc_p, rpos])
            acc_blob = torch.cat([acc_blob, rblob])
            k2, v2, p2 = ops.sort_by_key(mk, mv, mp)
            acc_k, acc_v, acc_p, _ = ops.reduce_by_key_sorted(k2, v2, p2)
            # compact: keep only surviving exemplars' bytes so the blob
            # stays O(unique keys), not O(rounds x receive)
            clens, acc_blob = ops.extract_words(acc_blob, acc_p)
            clens = clens.to(dev)
            coff = torch.cumsum(clens, 0) - clens
            acc_p = (coff << 16) | clens
        return acc_k, acc_v, acc_p, acc_blob

    def shuffle_reduce(self, nwords: int) -> WordCountResult:
        """Phase 2: extract + sort uniques, all-to-all exchange, segmented
        reduce — collective across ranks (every rank must enter)."""
        text = self._text
        dev = self.device
        self.last_shuffle_rounds = 1

        # ---- EXTRACT + SORT: one native op from the table to the sorted,
        # packed result; it also leaves the word lengths, their offsets
        # and the blob size (MR_EXTRACT_SORTED=0: the composed general
        # ops, same tuple)
        sk, sv, sp, lens, offs, total_b, packed = ops.extract_sorted(
            self.table)
        cache = None

        if self.world > 1 or dx.force_collectives():
            # ---- SHUFFLE (C5/C6): slice sorted arrays by partition
            counts_d = ops.partition_counts(sk, self.world)
            blob = ops.gather_words(text, sp, offs, total_b)
            # per-partition blob byte counts: cumsum(lens) at boundaries
            bnd = torch.cumsum(counts_d, 0)
            if lens.numel():
                lcs = torch.cumsum(lens, 0)
                cum = torch.where(
                    bnd > 0, lcs.index_select(0, (bnd - 1).clamp(min=0)),
                    torch.zeros_like(bnd))
                blob_counts_d = torch.cat([cum[:1], cum[1:] - cum[:-1]])
            else:
                lcs = torch.zeros(0, dtype=torch.int64, device=dev)
                blob_counts_d = torch.zeros_like(counts_d)
            # ONE packed size exchange + ONE host sync for both arrays
            # (xGMI collectives and D2H syncs are per-call latency-bound;
            # fewer+larger wins — guide).  The FULL count matrix comes
            # back, so every rank can compute every rank's receive size
            # and agree on the chunked-round count with no extra
            # collective.
            packed = torch.cat([counts_d, blob_counts_d])
            full = dx.exchange_counts_full(packed, self.group).cpu()
            send_c = full[self.rank, 0].tolist()
            send_b = full[self.rank, 1].tolist()
            recv_c = full[:, 0, self.rank].tolist()
            recv_b = full[:, 1, self.rank].tolist()
            rounds = self._plan_shuffle_rounds(full)
            self.last_shuffle_rounds = rounds
            if rounds > 1:
                fk, fv, fp, blob_src = self._chunked_shuffle_reduce(
                    sk, sv, lens, blob, lcs, full, rounds)
            else:
                # ONE i64 all-to-all for (key, count, len): rows interleave
                # the three arrays, so each partition's segment stays
                # contiguous and split sizes just triple
                tri = torch.stack([sk, sv, lens], dim=1).reshape(-1)
                rtri = dx.exchange(tri, [3 * c for c in send_c],
                                   [3 * c for c in recv_c], self.group)
                rtri = rtri.view(-1, 3)
                rk = rtri[:, 0].contiguous()
                rv = rtri[:, 1].contiguous()
                rlens = rtri[:, 2].contiguous()
                if dev.type == "cuda":
                    # C5 overlap (BASELINE): the exemplar-blob all-to-all
                    # rides a SIDE stream while the current stream sorts
                    # the received (key,count) runs — the collective uses
                    # the xGMI links/SDMA, the sort uses the CUs, so they
                    # compose.  Rank order stays deterministic: every
                    # rank issues tri-exchange then blob-exchange on the
                    # same communicator.
                    ev = torch.cuda.Event()
                    ev.record()  # blob + sizes ready; sorts not yet queued
                    side = getattr(self, "_side_stream", None)
                    if side is None:
                        side = torch.cuda.Stream(dev)
                        self._side_stream = side
                    side.wait_event(ev)
                    with torch.cuda.stream(side):
                        rblob = dx.exchange(blob, send_b, recv_b,
                                            self.group)
                    roff = torch.cumsum(rlens, 0) - rlens
                    rpos = (roff << 16) | rlens
                    # ---- REDUCE overlaps the blob exchange
                    k2, v2, p2 = ops.sort_by_key(rk, rv, rpos)
                    fk, fv, fp, _ = ops.reduce_by_key_sorted(k2, v2, p2)
                    cur = torch.cuda.current_stream(dev)
                    cur.wait_stream(side)
                    rblob.record_stream(cur)
                else:
                    rblob = dx.exchange(blob, send_b, recv_b, self.group)
                    roff = torch.cumsum(rlens, 0) - rlens
                    rpos = (roff << 16) | rlens
                    # ---- REDUCE: sort received runs, segment
                    k2, v2, p2 = ops.sort_by_key(rk, rv, rpos)
                    fk, fv, fp, _ = ops.reduce_by_key_sorted(k2, v2, p2)
                blob_src = rblob
        else:
            fk, fv, fp = sk, sv, sp
            blob_src = text
            cache = dict(packed=packed, offs=offs, total_bytes=total_b,
                         cache_src=text)

        self._mark("shuffle_reduce")
        self._collect_timing()
        return WordCountResult(
            keys=fk, counts=fv, pos=fp, blob_src=blob_src, nwords=nwords,
            hash_kind="wordhash64" if dev.type == "cuda" else "fnv1a64",
            **(cache or {}))
