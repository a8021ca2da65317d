// MapReduce hot-path kernels for MI355X (gfx950), CDNA4-native.
//
// These replace the reference's CPU-Lua hot loops:
//   K2/K3  tokenize_v7_kernel     — THE production tokenizer: branchless
//          ws-mask scan, chunked register hashing (wordhash64), per-block
//          LDS cache for the Zipf head, wave-chunked spill allocator for
//          the tail (template flags add spill-all and fused (word,doc)
//          composite modes for the inverted index).  It is v6's window:
//          each lane hashes and probes its words one after the other, in
//          v6's order.  What differs: the block's next tile is prefetched
//          into registers during the word loop and written to the ONE LDS
//          tile buffer after it (two barriers per tile: one right after
//          the tile's bytes are read into registers, one after the
//          prefetch is written), and a word's first 8 bytes are extracted
//          with 32-bit selects + v_alignbyte.  tokenize_v6_kernel differs
//          only in that it stages the tile in the open (barrier, load,
//          wait, LDS write, barrier) and extracts every chunk with 64-bit
//          selects and a funnel shift; it is kept as v7's A/B partner
//          (MR_TOKENIZE_V6=1) with the same five instantiations.
//          tokenize_kernel (plain (hash, pos) emit, has a CPU twin, used
//          by the inverted index's small paths) and tokenize_count_kernel
//          (fused tokenize + table count, the low-memory mode) are the
//          two other tokenizers
//   K5     bucket_count_kernel    — per-bucket LDS count of the
//          top-byte-partitioned spill tail; hash_insert/extract are the
//          generic table ops (extract has a chunked-compaction v2 for
//          large tables); the sorted form is radix_sort.hip + the
//          seg_reduce kernels below
//   K2     partition_hist         — all-to-all send counts (C5 setup)
//   K7/K8  gather_bytes           — exemplar word extraction for the
//          hash -> string dictionary at the finalfn boundary
//
// All memory-bound: vectorized accesses, grid-stride loops.  The recurring
// measured lesson (see profiles/): a shared atomic counter serializes
// cross-XCD at ~9 ns/op — every append path here reserves CHUNKED ranges
// per wave and pads unused tail slots with HT_EMPTY, which downstream
// consumers skip.

#include "common.h"

// ---------------------------------------------------------------------------
// K2/K3: tokenizer — emit (hash64, pos) per word of a byte buffer
// ---------------------------------------------------------------------------
// pos packs (start << 16 | len) so the exemplar word bytes can be gathered
// later; output order is nondeterministic (atomic append) — every consumer
// sorts or hash-aggregates, so order never matters.  NOTE: one counter
// atomic per word — fine at test scale, NOT a hot-path kernel (the
// production paths use the wave-chunked allocator; see header).

#define TOK_BYTES 16

__global__ void tokenize_kernel(const u8* __restrict__ text, long n,
                                u64* __restrict__ out_hash,
                                u64* __restrict__ out_pos,
                                unsigned long long* __restrict__ counter,
                                long cap) {
  long t0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) * (long)TOK_BYTES;
  long stride = (long)gridDim.x * blockDim.x * TOK_BYTES;
  for (long base = t0; base < n; base += stride) {
    long end = base + TOK_BYTES < n ? base + TOK_BYTES : n;
    u8 prev = (base == 0) ? ' ' : text[base - 1];
    for (long i = base; i < end; ++i) {
      u8 c = text[i];
      if (!is_ws(c) && is_ws(prev)) {
        u64 h = FNV64_OFFSET;
        long j = i;
        while (j < n) {
          u8 cc = text[j];
          if (is_ws(cc)) break;
          h ^= cc;
          h *= FNV64_PRIME;
          ++j;
        }
        unsigned long long idx = atomicAdd(counter, 1ull);
        if ((long)idx < cap) {
          out_hash[idx] = h;
          long len = j - i;
          if (len > 0xFFFF) len = 0xFFFF;
          out_pos[idx] = ((u64)i << 16) | (u64)len;
        }
      }
      prev = c;
    }
  }
}

// hash-table primitives (shared by the fused and unfused insert paths)
DEV u64 remap_key(u64 k) {
  // keep HT_EMPTY available as the slot sentinel for arbitrary inputs
  return k == HT_EMPTY ? HT_EMPTY - 1 : k;
}

DEV u32 first_slot(u64 k, u64 cap_mask) {
  // keys are already FNV-mixed; fold high bits so table size bits differ
  return (u32)((k ^ (k >> 32)) & cap_mask);
}

// ---------------------------------------------------------------------------
// K2+K5 fused: tokenize-and-count straight into the hash table.
// One pass over the text, no intermediate (hash, pos) arrays, no host sync
// per split (the word counter is read once per phase) — the map emit and
// the inline combiner of job.lua:83-97 collapsed into a single kernel.
// pos_base offsets word positions so many splits share one corpus buffer.
// ---------------------------------------------------------------------------

__device__ void ht_add(u64 k, u64 p, i64 cnt, u64* tkeys, i64* tvals,
                       u64* texm, u64 cap_mask);

// Layout per block iteration: stage a TOK_TILE-byte text tile (+halo) into
// LDS with coalesced dwordx4 loads, scan bytes from LDS (fast dynamic
// indexing — registers would spill, guide rule 20), and count words into a
// per-block LDS cache table.  The cache absorbs the Zipf head: a hot word
// like "the" (~7% of tokens) costs LDS atomics inside each block and ONE
// HBM table update per block at flush — without it, the global same-address
// atomic chain serialized the whole kernel (measured: 98% of step time).
#define TOK_TILE 4096       // bytes per block per grid-stride iteration
#define TOK_HALO 64         // lookahead so most words finish inside LDS
#define TOK_CACHE 1024      // LDS cache slots (power of 2)
#define TOK_PROBE 2         // max LDS probes before spilling (cold words
                            // must fail FAST: a filled cache turns every
                            // miss into a dependent LDS probe chain —
                            // measured 3.8 ms/step at 16 probes)

__global__ __launch_bounds__(256) void tokenize_count_kernel(
    const u8* __restrict__ text, long n, u64 pos_base,
    u64* __restrict__ tkeys, i64* __restrict__ tvals, u64* __restrict__ texm,
    u64 cap_mask, unsigned long long* __restrict__ nwords) {
  __shared__ u8 tile[TOK_TILE + TOK_HALO];
  __shared__ u64 ckeys[TOK_CACHE];
  __shared__ u64 cpos[TOK_CACHE];
  __shared__ u32 ccnt[TOK_CACHE];
  for (int s = threadIdx.x; s < TOK_CACHE; s += blockDim.x) {
    ckeys[s] = HT_EMPTY;
    ccnt[s] = 0;
  }
  unsigned long long my_words = 0;
  long tile0 = (long)blockIdx.x * TOK_TILE;
  long tstride = (long)gridDim.x * TOK_TILE;
  for (long base = tile0; base < n; base += tstride) {
    __syncthreads();
    // ---- stage tile + halo (dwordx4-coalesced where aligned)
    long avail = n - base;
    long want = avail < TOK_TILE + TOK_HALO ? avail : TOK_TILE + TOK_HALO;
    for (int o = threadIdx.x * 16; o < want; o += blockDim.x * 16) {
      if (o + 16 <= want && (((uintptr_t)&text[base + o]) & 15) == 0) {
        *(uint4*)&tile[o] = *(const uint4*)&text[base + o];
      } else {
        for (int b = 0; b < 16 && o + b < want; ++b)
          tile[o + b] = text[base + o + b];
      }
    }
    __syncthreads();
    // ---- scan this thread's TOK_BYTES window
    long my0 = (long)threadIdx.x * TOK_BYTES;
    long myend = my0 + TOK_BYTES;
    if (myend > avail) myend = avail;
    if (my0 < myend) {
      u8 prev = (base + my0 == 0) ? ' ' : (my0 ? tile[my0 - 1]
                                               : text[base - 1]);
      for (long i = my0; i < myend; ++i) {
        u8 c = tile[i];
        if (!is_ws(c) && is_ws(prev)) {
          u64 h = FNV64_OFFSET;
          long j = i;
          long lim = want;
          while (j < lim) {
            u8 cc = tile[j];
            if (is_ws(cc)) break;
            h ^= cc;
            h *= FNV64_PRIME;
            ++j;
          }
          if (j == lim && base + j < n) {
            // rare: word continues past the halo — finish from HBM
            long g = base + j;
            while (g < n) {
              u8 cc = text[g];
              if (is_ws(cc)) break;
              h ^= cc;
              h *= FNV64_PRIME;
              ++g;
            }
            j = g - base;
          }
          long len = j - i;
          if (len > 0xFFFF) len = 0xFFFF;
          u64 k = remap_key(h);
          u64 p = ((pos_base + (u64)(base + i)) << 16) | (u64)len;
          ++my_words;
          // ---- LDS cache insert (linear probe, bounded)
          u32 slot = (u32)((k ^ (k >> 32)) & (TOK_CACHE - 1));
          bool done = false;
          for (int pr = 0; pr < TOK_PROBE; ++pr) {
            u64 cur = ckeys[slot];
            if (cur == k) {
              atomicAdd(&ccnt[slot], 1u);
              done = true;
              break;
            }
            if (cur == HT_EMPTY) {
              u64 prev_k = atomicCAS((unsigned long long*)&ckeys[slot],
                                     (unsigned long long)HT_EMPTY,
                                     (unsigned long long)k);
              if (prev_k == HT_EMPTY) cpos[slot] = p;
              if (prev_k == HT_EMPTY || prev_k == k) {
                atomicAdd(&ccnt[slot], 1u);
                done = true;
                break;
              }
            }
            slot = (slot + 1) & (TOK_CACHE - 1);
          }
          if (!done)  // cache full here: straight to the HBM table
            ht_add(k, p, 1, tkeys, tvals, texm, cap_mask);
        }
        prev = c;
      }
    }
  }
  // ---- flush the block cache to the global table
  __syncthreads();
  for (int s = threadIdx.x; s < TOK_CACHE; s += blockDim.x) {
    if (ckeys[s] != HT_EMPTY && ccnt[s])
      ht_add(ckeys[s], cpos[s], (i64)ccnt[s], tkeys, tvals, texm, cap_mask);
  }
  // one atomic per wave for the word-count metric (guide G12)
  unsigned long long ws = my_words;
  for (int off = 32; off > 0; off >>= 1) ws += __shfl_down(ws, off, WAVE);
  if (lane_id() == 0 && ws) atomicAdd(nwords, ws);
}

// ---------------------------------------------------------------------------
// K2+K5 v6: single-phase window tokenizer, the A/B partner of v7 below
// (MR_TOKENIZE_V6=1).  A block stages a 4 KB tile (+64 B halo) into LDS.
// Per thread: classify its 16 LDS bytes (+16 lookahead) into a whitespace
// bitmask (SWAR, branchless), iterate word starts with ffs (~words, not
// ~bytes, iterations), hash from REGISTERS via funnel shifts (zero LDS
// re-reads), count the word in the block's LDS cache, spill the misses
// through the wave-chunked allocator.  Two barriers per tile — a word-list
// restructure with a third measured 2x slower: extra barriers and LDS cost
// more than lane balance buys (NOTES.md, recorded negative results).
// Template flags add spill-all (no cache) and the fused (word, doc)
// composite keys of the inverted index.
// ---------------------------------------------------------------------------

// (pos << 16 | len) of the word at the lowest set bit of `smw` (the
// not-yet-consumed starts of a 16-byte window): len is the distance to the
// next whitespace bit of m32, or `long_len` when the word runs past the
// 32-byte register window (only a window's last start can).
__device__ __forceinline__ u64 v6_spill_pos(u64 wpos0, u32 smw, u32 m32,
                                            u32 long_len) {
  int s = __ffs(smw) - 1;
  u32 t = m32 >> s;
  u32 len = t ? (u32)(__ffs(t) - 1) : long_len;
  return ((wpos0 + (u64)s) << 16) | (u64)len;
}

// threads per block of every v6 / v7 launch: one window pass of
// TOK_THREADS x 16 bytes is the tile.  The launchers static_assert their
// block size against it.
constexpr int TOK_THREADS = 256;

template <int CACHE_N, bool GPOS,
          bool SPILL_ALL = false,  // emit every word (no cache)
          bool COMPOSITE = false,  // keys = wordhash ^ splitmix64(doc)
                                   // (doc from split_off binary search) —
                                   // the inverted-index path, fusing the
                                   // doc lookup + mix into the tokenizer
          int SCHUNK = 512>  // chunked-allocator reservation size: pads
                             // scale with it (waves x SCHUNK/2 wasted
                             // tail entries) vs atomic amortization
__global__ __launch_bounds__(TOK_THREADS) void tokenize_v6_kernel(
    const u8* __restrict__ text, long n, u64 pos_base,
    u64* __restrict__ tkeys, i64* __restrict__ tvals, u64* __restrict__ texm,
    u64 cap_mask, u64* __restrict__ out_hash, u64* __restrict__ out_pos,
    unsigned long long* __restrict__ spill_counter, long spill_cap,
    unsigned long long* __restrict__ nwords, u64* __restrict__ cpos_g,
    const i64* __restrict__ split_off = nullptr, int nsplit_off = 0,
    long doc_base = 0) {
  constexpr int TILE_N = TOK_THREADS * TOK_BYTES;  // one window pass per tile
  __shared__ __align__(16) u8 tile[TILE_N + TOK_HALO];
  __shared__ u64 ckeys[CACHE_N];
  // exemplar positions: LDS normally; with GPOS a global side-buffer
  // (written once per distinct word per block — off the critical path)
  // frees 16 KB LDS for occupancy
  __shared__ u64 cpos_l[GPOS ? 1 : CACHE_N];
  __shared__ u32 ccnt[CACHE_N];
  u64* cpos = GPOS ? &cpos_g[(u64)blockIdx.x * CACHE_N] : cpos_l;
  for (int s = threadIdx.x; s < CACHE_N; s += blockDim.x) {
    ckeys[s] = HT_EMPTY;
    ccnt[s] = 0;
  }
  const int tid = threadIdx.x;
  unsigned long long my_words = 0;
  // wave-chunked spill allocator: ONE same-address global atomic per
  // 512-entry chunk per wave instead of one per window — the shared
  // counter's cross-XCD atomic serialization measured 2.7 ms of a
  // 3.2 ms kernel (ablation: no-spill 0.48 ms vs full 3.19 ms with
  // near-identical static code).  Chunk tails are padded with HT_EMPTY
  // keys; downstream consumers skip them.
  constexpr int SPILL_CHUNK = SCHUNK;
  long wchunk = -1;
  int wleft = 0;
  long tile0 = (long)blockIdx.x * TILE_N;
  long tstride = (long)gridDim.x * TILE_N;
  for (long base = tile0; base < n; base += tstride) {
    __syncthreads();
    long avail = n - base;
    long want = avail < TILE_N + TOK_HALO ? avail : TILE_N + TOK_HALO;
    for (int o = tid * 16; o < want; o += blockDim.x * 16) {
      if (o + 16 <= want && (((uintptr_t)&text[base + o]) & 15) == 0) {
        *(uint4*)&tile[o] = *(const uint4*)&text[base + o];
      } else {
        for (int b = 0; b < 16 && o + b < want; ++b)
          tile[o + b] = text[base + o + b];
      }
    }
    __syncthreads();
    // One window pass covers the tile.  It is still written as a loop (of
    // one pass, body not indented): without the loop the compiler schedules
    // this kernel differently, 3 to 5 instructions longer, and v6 is kept
    // as it was measured.
    for (int wnd = 0; wnd < 1; ++wnd) {
    long my0 = (long)tid * TOK_BYTES;
    // whole wave stays in the loop (the spill wave-scan below needs every
    // lane present); out-of-range lanes just contribute ns = 0
    bool wactive = my0 < avail;
    // 32 bytes in registers: my window + 16B lookahead (halo-staged)
    const uint4 va = wactive ? *(const uint4*)&tile[my0] : uint4{0, 0, 0, 0};
    const uint4 vb = wactive ? *(const uint4*)&tile[my0 + 16] : uint4{0, 0, 0, 0};
    const u64 q0 = (u64)va.x | ((u64)va.y << 32);
    const u64 q1 = (u64)va.z | ((u64)va.w << 32);
    const u64 q2 = (u64)vb.x | ((u64)vb.y << 32);
    const u64 q3 = (u64)vb.z | ((u64)vb.w << 32);
    // SWAR classify: 4 x ws_mask8 (~17 u64 ops each) replaces 32 per-byte
    // is_ws calls (ablation: stage+classify was 44% of the kernel at 4 MB)
    u32 m32 = ws_mask8(q0) | (ws_mask8(q1) << 8) |
              (ws_mask8(q2) << 16) | (ws_mask8(q3) << 24);
    // bytes at/after `want` count as whitespace (stale stage data)
    long lim32 = want - my0;
    if (lim32 < 32)
      m32 |= (lim32 <= 0) ? 0xFFFFFFFFu : ~((1u << lim32) - 1);
    u32 prevb = (base + my0 == 0)
                    ? 1u
                    : (wactive ? (u32)is_ws(my0 ? tile[my0 - 1]
                                                : text[base - 1]) : 1u);
    u32 sm = wactive ? (~m32 & ((m32 << 1) | prevb) & 0xFFFFu) : 0u;
    long limw = avail - my0;  // starts must be real data bytes
    if (limw < 16) sm &= (limw <= 0) ? 0u : ((1u << limw) - 1);
    my_words += __popc(sm);
    // fully-unrolled word loop (a 16-byte window holds <= 8 words):
    // compile-time slot indices keep the miss buffers in REGISTERS —
    // runtime-indexed arrays here lower to divergent v_movrel waterfalls
    // (measured 2.7 ms of a 3.2 ms kernel, ablation modes 3 vs 4), and
    // per-word ballot aggregation is worse still (12.8 ms: divergent
    // ballots + atomics)
    // Only the keys are buffered: a spilled record's position is rebuilt
    // where it is stored (v6_spill_pos) from the start mask, m32 and the
    // one long-word length — 16 fewer VGPRs (106 -> 90 on the word-count
    // default, which admits 5 waves/SIMD instead of 4).
    u64 sh_[8];
    const u32 sm0 = sm;
    u32 long_len = 0;  // len of the (at most one, last) word past the window
    const u64 wpos0 = pos_base + (u64)(base + my0);
    u32 miss_mask = 0;
    #pragma unroll
    for (int wi = 0; wi < 8; ++wi) {
      if (!sm) break;
      int s = __ffs(sm) - 1;
      sm &= sm - 1;
      u32 t = m32 >> s;
      u64 h = FNV64_OFFSET;
      u32 len;
      if (t) {
        len = (u32)(__ffs(t) - 1);  // bit s is clear, so len >= 1
        // chunked hash from registers: bytes s..s+len-1 of q0..q3 as
        // 8-byte windows (branchless selects, zero LDS re-reads; the
        // last window masks to the remaining bytes)
        for (u32 c = 0; c < len; c += 8) {
          int j0 = s + (int)c;
          int qi = j0 >> 3;
          u64 lo = (qi & 2) ? ((qi & 1) ? q3 : q2) : ((qi & 1) ? q1 : q0);
          u64 hi = (qi >= 3) ? 0 : ((qi & 2) ? q3 : ((qi & 1) ? q2 : q1));
          int sh2 = 8 * (j0 & 7);
          u64 w = sh2 ? ((lo >> sh2) | (hi << (64 - sh2))) : lo;
          u32 rem = len - c;
          if (rem < 8) w &= (((u64)1 << (8 * rem)) - 1);
          h = whash_chunk(h, w);
        }
        h = whash_fin(h, len);
      } else {
        // word longer than the 32-byte window: scan from global,
        // accumulating the same 8-byte chunks
        long g = base + my0 + s;
        u64 chunk = 0;
        int cb = 0;
        long wlen = 0;
        while (g < n && !is_ws(text[g])) {
          chunk |= (u64)text[g] << (8 * cb);
          if (++cb == 8) {
            h = whash_chunk(h, chunk);
            chunk = 0;
            cb = 0;
          }
          ++g;
          ++wlen;
        }
        if (cb) h = whash_chunk(h, chunk);
        h = whash_fin(h, (u64)wlen);
        len = (u32)(wlen > 0xFFFF ? 0xFFFF : wlen);
        long_len = len;
      }
      if (COMPOSITE) {
        // fuse the (word, doc) composite: doc from the split-offset
        // table (L2-resident; ~10-step binary search per word)
        i64 byte = (i64)(pos_base + (u64)(base + my0 + s));
        int doc = ub_minus1(split_off, nsplit_off, byte);
        h ^= splitmix64_dev((u64)(doc + doc_base));
      }
      u64 k = remap_key(h);
      u64 p = ((pos_base + (u64)(base + my0 + s)) << 16) | (u64)len;
      if (SPILL_ALL) {
        miss_mask |= 1u << wi;
        sh_[wi] = k;
        continue;
      }
      // LDS cache insert
      u32 slot = (u32)((k ^ (k >> 32)) & (CACHE_N - 1));
      bool done = false;
      for (int pr = 0; pr < TOK_PROBE; ++pr) {
        u64 cur2 = ckeys[slot];
        if (cur2 == k) {
          atomicAdd(&ccnt[slot], 1u);
          done = true;
          break;
        }
        if (cur2 == HT_EMPTY) {
          u64 prevk = atomicCAS((unsigned long long*)&ckeys[slot],
                                (unsigned long long)HT_EMPTY,
                                (unsigned long long)k);
          if (prevk == HT_EMPTY) cpos[slot] = p;
          if (prevk == HT_EMPTY || prevk == k) {
            atomicAdd(&ccnt[slot], 1u);
            done = true;
            break;
          }
        }
        slot = (slot + 1) & (CACHE_N - 1);
      }
      if (!done) {
        miss_mask |= 1u << wi;  // wi is compile-time: register slot
        sh_[wi] = k;
      }
    }
    // window-level spill reservation: every lane of the wave is present
    // here (wactive design above)
    u32 my_ns = (u32)__popc(miss_mask);
    // (four ballots + mbcnt instead of these six dependent shuffles
    // measured no gain: profiles/tokenizer_occupancy_r04.md)
    u32 incl = my_ns;
    #pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
      u32 x = __shfl_up(incl, off, WAVE);
      if ((threadIdx.x & (WAVE - 1)) >= off) incl += x;
    }
    u32 wave_total = __shfl(incl, WAVE - 1, WAVE);
    int lane = threadIdx.x & (WAVE - 1);
    if (wave_total && (int)wave_total > wleft) {
      // retire the old chunk's tail (pad with HT_EMPTY) + grab a new
      // one (at least a window's worth: a pathological window can
      // produce up to 64x8 misses, more than a small SPILL_CHUNK)
      for (int i = lane; i < wleft; i += WAVE)
        if (wchunk + i < spill_cap) out_hash[wchunk + i] = HT_EMPTY;
      int grab = (int)wave_total > SPILL_CHUNK ? (int)wave_total
                                               : SPILL_CHUNK;
      unsigned long long nb = 0;
      if (lane == 0)
        nb = atomicAdd(spill_counter, (unsigned long long)grab);
      wchunk = (long)__shfl(nb, 0, WAVE);
      wleft = grab;
    }
    long o = wchunk + (long)(incl - my_ns);
    if (wave_total) {
      wchunk += wave_total;
      wleft -= (int)wave_total;
    }
    u32 smw = sm0;
    #pragma unroll
    for (int wi = 0; wi < 8; ++wi) {
      if (miss_mask & (1u << wi)) {
        u64 p = v6_spill_pos(wpos0, smw, m32, long_len);
        if (o < spill_cap) {
          out_hash[o] = sh_[wi];
          out_pos[o] = p;
        }
        ++o;
      }
      smw &= smw - 1;
    }
    }  // wnd
  }
  {  // retire this wave's final spill-chunk tail
    int lane = threadIdx.x & (WAVE - 1);
    for (int i = lane; i < wleft; i += WAVE)
      if (wchunk + i < spill_cap) out_hash[wchunk + i] = HT_EMPTY;
  }
  __syncthreads();
  for (int s = tid; s < CACHE_N; s += blockDim.x)
    if (ckeys[s] != HT_EMPTY && ccnt[s])
      ht_add(ckeys[s], cpos[s], (i64)ccnt[s], tkeys, tvals, texm, cap_mask);
  unsigned long long ws = my_words;
  for (int off = 32; off > 0; off >>= 1) ws += __shfl_down(ws, off, WAVE);
  if (lane_id() == 0 && ws) atomicAdd(nwords, ws);
}

// ---------------------------------------------------------------------------
// K2+K5 v7: v6's window (same masks, hashes, cache probes, spill allocator;
// the same words are cached and spilled) with two changes, both chosen from
// counters that showed the kernel VALU-bound at 4 waves per SIMD rather than
// parked (profiles/tokenizer_phases_r07.md):
//
//   * The next tile is prefetched into registers.  One window pass covers
//     the whole tile (TILE_N = 256 x 16) and a thread's 32 bytes + previous
//     byte are in registers right after the staging barrier, so the tile
//     buffer is free again at once.  The next tile's global loads (one
//     16-byte load per thread, the 64-byte halo as one dword on threads
//     0-15, thread 0's previous byte: no thread makes a second trip) are
//     issued before the word loop and written to LDS after it; the spill
//     stores come after that write, so the wait on the prefetch never waits
//     on stores of its own iteration.  The barrier after the LDS reads is
//     met by waves that just left the staging barrier together; the one
//     where waves arrive skewed is still one per tile, and LDS stays at one
//     tile buffer.  Unaligned text and the last, partial tile are staged by
//     the plain loop in a cold branch.
//   * A word's first 8 bytes (all of most words) come from three of the
//     window's first six dwords, picked by start >> 2 and joined by two
//     v_alignbyte, instead of 64-bit selects over q0..q3 and a 64-bit funnel
//     shift: 10 % fewer VALU instructions per job.  Later chunks of longer
//     words keep v6's form.
//
// The window code below is a copy of v6's on purpose.  Moving it into shared
// __forceinline__ helpers was tried piece by piece (masks, later-chunk hash,
// long-word scan, cache probe, spill phase, final flush): every piece changed
// the generated code of v6, and all but the mask construction that of v7
// (from one commuted operand to 200 instructions), and wait placement in
// this loop is fragile.  So a change to the window is made in both kernels;
// the v6 == v7 bit-identity test keeps them in step.
// ---------------------------------------------------------------------------
#define V7_WAIT_VM0 0x0F70  // s_waitcnt vmcnt(0) alone (gfx9 encoding)

template <int TILE_N>
__device__ __forceinline__ void v7_stage_plain(u8* tile,
                                               const u8* __restrict__ text,
                                               long base, long want,
                                               bool aligned) {
  for (int o = threadIdx.x * 16; o < want; o += TOK_THREADS * 16) {
    if (aligned && o + 16 <= want) {
      *(uint4*)&tile[o] = *(const uint4*)&text[base + o];
    } else {
      for (int b = 0; b < 16 && o + b < want; ++b)
        tile[o + b] = text[base + o + b];
    }
  }
}

template <int CACHE_N, bool GPOS, bool SPILL_ALL = false,
          bool COMPOSITE = false, int SCHUNK = 512>
// 5 waves per SIMD asked for where the LDS admits 5 blocks: 96 VGPRs, as v6
__global__ __launch_bounds__(TOK_THREADS, GPOS || SPILL_ALL ? 5 : 3)
void tokenize_v7_kernel(
    const u8* __restrict__ text, long n, u64 pos_base,
    u64* __restrict__ tkeys, i64* __restrict__ tvals, u64* __restrict__ texm,
    u64 cap_mask, u64* __restrict__ out_hash, u64* __restrict__ out_pos,
    unsigned long long* __restrict__ spill_counter, long spill_cap,
    unsigned long long* __restrict__ nwords, u64* __restrict__ cpos_g,
    const i64* __restrict__ split_off = nullptr, int nsplit_off = 0,
    long doc_base = 0) {
  constexpr int TILE_N = TOK_THREADS * TOK_BYTES;  // one window pass per tile
  __shared__ __align__(16) u8 tile[TILE_N + TOK_HALO];
  __shared__ u64 ckeys[CACHE_N];
  __shared__ u64 cpos_l[GPOS ? 1 : CACHE_N];
  __shared__ u32 ccnt[CACHE_N];
  u64* cpos = GPOS ? &cpos_g[(u64)blockIdx.x * CACHE_N] : cpos_l;
  for (int s = threadIdx.x; s < CACHE_N; s += blockDim.x) {
    ckeys[s] = HT_EMPTY;
    ccnt[s] = 0;
  }
  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  unsigned long long my_words = 0;
  constexpr int SPILL_CHUNK = SCHUNK;
  long wchunk = -1;
  int wleft = 0;
  const long tile0 = (long)blockIdx.x * TILE_N;
  const long tstride = (long)gridDim.x * TILE_N;
  // uniform per launch: base and o are multiples of 16
  const bool aligned = (((uintptr_t)text) & 15) == 0;
  if (tile0 < n) {
    long avail0 = n - tile0;
    v7_stage_plain<TILE_N>(tile, text, tile0,
                           avail0 < TILE_N + TOK_HALO ? avail0
                                                      : TILE_N + TOK_HALO,
                           aligned);
  }
  const long my0 = (long)tid * TOK_BYTES;
  // the byte before the tile (thread 0's previous byte) travels with the
  // prefetch in a register: a load of it inside the window would make wave
  // 0 wait for the whole prefetch (loads return in order)
  u32 pb_cur = (tid == 0 && tile0 > 0 && tile0 < n) ? text[tile0 - 1] : 0x20;
  // nothing is in flight when the loop is entered: the compiler's wait
  // placement then sees a register written by a pending load only on paths
  // where it is one, and keeps the top of the loop free of vmcnt waits.
  // This only steers the compiler and a later one may place its waits
  // differently.  To check that it still helps, read the ISA of the
  // default instantiation (hipcc -S --offload-arch=gfx950 -O3): inside
  // the tile loop there must be no s_waitcnt vmcnt between the
  // global_load_dwordx4 / global_load_dword of the prefetch and the second
  // s_barrier, and none after it before the word loop's first
  // global_load_ubyte (the long-word scan).  Without this line there were
  // three vmcnt(0) there and the prefetch was waited for at once.
  __builtin_amdgcn_s_waitcnt(V7_WAIT_VM0);
  for (long base = tile0; base < n; base += tstride) {
    const long avail = n - base;
    const long want = avail < TILE_N + TOK_HALO ? avail : TILE_N + TOK_HALO;
    // next tile of this block: prefetched when it is a full tile + halo of
    // 16-byte-aligned text, staged by the plain loop otherwise
    const long nbase = base + tstride;
    const bool pf_fast = aligned && nbase + TILE_N + TOK_HALO <= n;
    uint4 pf = uint4{0, 0, 0, 0};
    u32 ph = 0;
    u32 pb_next = 0x20;
    if (tid == 0 && nbase < n) pb_next = text[nbase - 1];
    if (pf_fast) {
      pf = *(const uint4*)&text[nbase + my0];
      if (tid < TOK_HALO / 4) ph = *(const u32*)&text[nbase + TILE_N + tid * 4];
    }
    __syncthreads();
    // whole wave stays in the loop (the spill wave-scan below needs every
    // lane present); out-of-range lanes just contribute ns = 0
    const bool wactive = my0 < avail;
    const uint4 va = wactive ? *(const uint4*)&tile[my0] : uint4{0, 0, 0, 0};
    const uint4 vb = wactive ? *(const uint4*)&tile[my0 + 16] : uint4{0, 0, 0, 0};
    u32 prevb = (base + my0 == 0)
                    ? 1u
                    : (wactive ? (u32)is_ws(my0 ? tile[my0 - 1]
                                                : (u8)pb_cur) : 1u);
    __syncthreads();  // every thread holds its bytes: the tile buffer
                      // may be overwritten
    const u64 q0 = (u64)va.x | ((u64)va.y << 32);
    const u64 q1 = (u64)va.z | ((u64)va.w << 32);
    const u64 q2 = (u64)vb.x | ((u64)vb.y << 32);
    const u64 q3 = (u64)vb.z | ((u64)vb.w << 32);
    u32 m32 = ws_mask8(q0) | (ws_mask8(q1) << 8) |
              (ws_mask8(q2) << 16) | (ws_mask8(q3) << 24);
    // bytes at/after `want` count as whitespace (stale stage data)
    long lim32 = want - my0;
    if (lim32 < 32)
      m32 |= (lim32 <= 0) ? 0xFFFFFFFFu : ~((1u << lim32) - 1);
    u32 sm = wactive ? (~m32 & ((m32 << 1) | prevb) & 0xFFFFu) : 0u;
    long limw = avail - my0;  // starts must be real data bytes
    if (limw < 16) sm &= (limw <= 0) ? 0u : ((1u << limw) - 1);
    my_words += __popc(sm);
    // compile-time slot indices keep sh_[] in registers (see v6); only the
    // keys are buffered, positions are rebuilt at the store (v6_spill_pos)
    u64 sh_[8];
    const u32 sm0 = sm;
    u32 long_len = 0;
    const u64 wpos0 = pos_base + (u64)(base + my0);
    u32 miss_mask = 0;
    // ---- v6's word loop
    #pragma unroll
    for (int wi = 0; wi < 8; ++wi) {
      if (!sm) break;
      int s = __ffs(sm) - 1;
      sm &= sm - 1;
      u32 t = m32 >> s;
      u64 h = FNV64_OFFSET;
      u32 len;
      if (t) {
        len = (u32)(__ffs(t) - 1);  // bit s is clear, so len >= 1
        {
          // bytes s..s+7 (s < 16): three of the window's first six dwords
          // picked by s >> 2, joined by two byte-aligns
          const int di = s >> 2;
          const u32 bsh = (u32)s & 3u;
          u32 a0 = (di & 2) ? ((di & 1) ? va.w : va.z) : ((di & 1) ? va.y : va.x);
          u32 a1 = (di & 2) ? ((di & 1) ? vb.x : va.w) : ((di & 1) ? va.z : va.y);
          u32 a2 = (di & 2) ? ((di & 1) ? vb.y : vb.x) : ((di & 1) ? va.w : va.z);
          u64 w = (u64)__builtin_amdgcn_alignbyte(a1, a0, bsh) |
                  ((u64)__builtin_amdgcn_alignbyte(a2, a1, bsh) << 32);
          u32 nb = len < 8 ? len : 8;
          w &= ~(u64)0 >> (64 - 8 * nb);
          h = whash_chunk(h, w);
        }
        for (u32 c = 8; c < len; c += 8) {
          int j0 = s + (int)c;
          int qi = j0 >> 3;
          u64 lo = (qi & 2) ? ((qi & 1) ? q3 : q2) : ((qi & 1) ? q1 : q0);
          u64 hi = (qi >= 3) ? 0 : ((qi & 2) ? q3 : ((qi & 1) ? q2 : q1));
          int sh2 = 8 * (j0 & 7);
          u64 w = sh2 ? ((lo >> sh2) | (hi << (64 - sh2))) : lo;
          u32 rem = len - c;
          if (rem < 8) w &= (((u64)1 << (8 * rem)) - 1);
          h = whash_chunk(h, w);
        }
        h = whash_fin(h, len);
      } else {
        // word longer than the 32-byte window: scan from global
        long g = base + my0 + s;
        u64 chunk = 0;
        int cb = 0;
        long wlen = 0;
        while (g < n && !is_ws(text[g])) {
          chunk |= (u64)text[g] << (8 * cb);
          if (++cb == 8) {
            h = whash_chunk(h, chunk);
            chunk = 0;
            cb = 0;
          }
          ++g;
          ++wlen;
        }
        if (cb) h = whash_chunk(h, chunk);
        h = whash_fin(h, (u64)wlen);
        len = (u32)(wlen > 0xFFFF ? 0xFFFF : wlen);
        long_len = len;
      }
      if (COMPOSITE) {
        i64 byte = (i64)(pos_base + (u64)(base + my0 + s));
        int doc = ub_minus1(split_off, nsplit_off, byte);
        h ^= splitmix64_dev((u64)(doc + doc_base));
      }
      u64 k = remap_key(h);
      sh_[wi] = k;
      if (SPILL_ALL) {
        miss_mask |= 1u << wi;
        continue;
      }
      // v6's probe, one word at a time
      u64 p = ((pos_base + (u64)(base + my0 + s)) << 16) | (u64)len;
      u32 slot = (u32)((k ^ (k >> 32)) & (CACHE_N - 1));
      bool done = false;
      for (int pr = 0; pr < TOK_PROBE; ++pr) {
        u64 cur2 = ckeys[slot];
        if (cur2 == k) {
          atomicAdd(&ccnt[slot], 1u);
          done = true;
          break;
        }
        if (cur2 == HT_EMPTY) {
          u64 prevk = atomicCAS((unsigned long long*)&ckeys[slot],
                                (unsigned long long)HT_EMPTY,
                                (unsigned long long)k);
          if (prevk == HT_EMPTY) cpos[slot] = p;
          if (prevk == HT_EMPTY || prevk == k) {
            atomicAdd(&ccnt[slot], 1u);
            done = true;
            break;
          }
        }
        slot = (slot + 1) & (CACHE_N - 1);
      }
      if (!done) miss_mask |= 1u << wi;
    }
    // ---- the prefetched tile goes to LDS before this window's spill
    // stores are issued (the wait above them is then for loads only)
    if (nbase < n) {
      if (pf_fast) {
        *(uint4*)&tile[my0] = pf;
        if (tid < TOK_HALO / 4) *(u32*)&tile[TILE_N + tid * 4] = ph;
      } else {
        long navail = n - nbase;
        v7_stage_plain<TILE_N>(tile, text, nbase,
                               navail < TILE_N + TOK_HALO ? navail
                                                          : TILE_N + TOK_HALO,
                               aligned);
      }
    }
    pb_cur = pb_next;  // here, not at its load: the copy waits for it
    // ---- spill phase (v6's): wave scan, chunk reservation, stores
    {
      u32 my_ns = (u32)__popc(miss_mask);
      u32 incl = my_ns;
      #pragma unroll
      for (int off = 1; off < WAVE; off <<= 1) {
        u32 x = __shfl_up(incl, off, WAVE);
        if (lane >= off) incl += x;
      }
      u32 wave_total = __shfl(incl, WAVE - 1, WAVE);
      if (wave_total && (int)wave_total > wleft) {
        for (int i = lane; i < wleft; i += WAVE)
          if (wchunk + i < spill_cap) out_hash[wchunk + i] = HT_EMPTY;
        int grab = (int)wave_total > SPILL_CHUNK ? (int)wave_total
                                                 : SPILL_CHUNK;
        unsigned long long nb = 0;
        if (lane == 0)
          nb = atomicAdd(spill_counter, (unsigned long long)grab);
        wchunk = (long)__shfl(nb, 0, WAVE);
        wleft = grab;
      }
      long o = wchunk + (long)(incl - my_ns);
      if (wave_total) {
        wchunk += wave_total;
        wleft -= (int)wave_total;
      }
      u32 smw = sm0;
      #pragma unroll
      for (int wi = 0; wi < 8; ++wi) {
        if (miss_mask & (1u << wi)) {
          u64 p = v6_spill_pos(wpos0, smw, m32, long_len);
          if (o < spill_cap) {
            out_hash[o] = sh_[wi];
            out_pos[o] = p;
          }
          ++o;
        }
        smw &= smw - 1;
      }
    }
  }
  // retire this wave's final spill-chunk tail
  for (int i = lane; i < wleft; i += WAVE)
    if (wchunk + i < spill_cap) out_hash[wchunk + i] = HT_EMPTY;
  __syncthreads();
  for (int s = tid; s < CACHE_N; s += blockDim.x)
    if (ckeys[s] != HT_EMPTY && ccnt[s])
      ht_add(ckeys[s], cpos[s], (i64)ccnt[s], tkeys, tvals, texm, cap_mask);
  unsigned long long ws = my_words;
  for (int off = 32; off > 0; off >>= 1) ws += __shfl_down(ws, off, WAVE);
  if (lane == 0 && ws) atomicAdd(nwords, ws);
}

// ---------------------------------------------------------------------------
// K5 bucketized count: input (hash, pos) grouped by top-8-bit bucket (one
// radix partition pass).  grid = NBUCKETS x SLICES blocks; each block
// LDS-counts its slice of one bucket — a bucket's distinct keys (~vocab/256)
// fit the 2048-slot LDS table, so every per-word atomic is an LDS atomic;
// the global table sees only per-block flushes of distinct keys.
// ---------------------------------------------------------------------------

#define BKT_SLOTS 2048  // default LDS table slots (power of 2)

// SLOTS trades LDS table capacity against occupancy: 2048 slots = 40 KB
// = 4 blocks/CU; 1024 = 20 KB = 8 blocks/CU (PMC: waves wait ~16k cycles
// per ~660 VALU instrs — latency-bound, occupancy is the lever).  A slice
// holds ~390 distinct keys on the Europarl shape; overflow degrades to
// per-element ht_add, never wrong.
// ILP: independent probe chains in flight per thread.  The kernel is
// latency-bound at FULL occupancy (vgpr=12, 8 blocks/CU = 32 waves) —
// the LDS probe/atomic dependency chain is the limiter, and the huge
// register headroom admits interleaving several elements' chains
// (per probe round: ILP independent LDS loads, then ILP resolves).
// Same-key duplicates within one thread's group are safe: a losing
// CAS sees prevk == its own key and takes the atomicAdd path.
template <int SLOTS, int ILP = 1>
__global__ __launch_bounds__(256) void bucket_count_kernel(
    const u64* __restrict__ hashes, const u64* __restrict__ pos,
    const i64* __restrict__ bucket_off,  // [nbuckets+1] exclusive offsets,
                                         // OR per-bucket lengths when
                                         // region_stride > 0 (fixed-stride
                                         // regions: bucket b lives at
                                         // [b*stride, b*stride+len[b]))
    int nbuckets, int slices, u64* __restrict__ tkeys,
    i64* __restrict__ tvals, u64* __restrict__ texm, u64 cap_mask,
    long region_stride) {
  __shared__ u64 ckeys[SLOTS];
  __shared__ u64 cpos[SLOTS];
  __shared__ u32 ccnt[SLOTS];
  int bucket = blockIdx.x / slices;
  int slice = blockIdx.x % slices;
  if (bucket >= nbuckets) return;
  long b0, b1;
  if (region_stride > 0) {
    b0 = (long)bucket * region_stride;
    long len = bucket_off[bucket];
    b1 = b0 + (len < region_stride ? len : region_stride);
  } else {
    b0 = bucket_off[bucket];
    b1 = bucket_off[bucket + 1];
  }
  long bn = b1 - b0;
  long per = (bn + slices - 1) / slices;
  long s0 = b0 + (long)slice * per;
  long s1 = s0 + per < b1 ? s0 + per : b1;
  if (s0 >= s1) return;
  for (int s = threadIdx.x; s < SLOTS; s += blockDim.x) {
    ckeys[s] = HT_EMPTY;
    ccnt[s] = 0;
  }
  __syncthreads();
  // NOTE (r2 negative results, profiles/bucket_count_ab_r02.md): this
  // loop is NOT read-BW bound — lazy pos loads (load only on first
  // insert, -120 MB/step) measured 354 us vs 334 baseline, and a
  // manual next-key prefetch also 354 us.  The unconditional pos load
  // supplies useful memory-level parallelism; the limiter is the LDS
  // probe/atomic chain (ILP interleaves it).
  for (long i0 = s0 + threadIdx.x; i0 < s1;
       i0 += (long)ILP * blockDim.x) {
    u64 k[ILP];
    u64 p[ILP];
    u32 slot[ILP];
    u32 pend = 0;
    #pragma unroll
    for (int j = 0; j < ILP; ++j) {
      long i = i0 + (long)j * blockDim.x;
      k[j] = (i < s1) ? hashes[i] : HT_EMPTY;
      if (k[j] != HT_EMPTY) {  // HT_EMPTY = spill-chunk padding / tail
        p[j] = pos[i];
        slot[j] = (u32)((k[j] ^ (k[j] >> 17)) & (SLOTS - 1));
        pend |= 1u << j;
      }
    }
    for (int pr = 0; pr < 64 && pend; ++pr) {
      u64 cur[ILP];
      #pragma unroll
      for (int j = 0; j < ILP; ++j)
        if (pend & (1u << j)) cur[j] = ckeys[slot[j]];
      #pragma unroll
      for (int j = 0; j < ILP; ++j) {
        if (!(pend & (1u << j))) continue;
        if (cur[j] == k[j]) {
          atomicAdd(&ccnt[slot[j]], 1u);
          pend &= ~(1u << j);
        } else if (cur[j] == HT_EMPTY) {
          u64 prevk = atomicCAS((unsigned long long*)&ckeys[slot[j]],
                                (unsigned long long)HT_EMPTY,
                                (unsigned long long)k[j]);
          if (prevk == HT_EMPTY) cpos[slot[j]] = p[j];
          if (prevk == HT_EMPTY || prevk == k[j]) {
            atomicAdd(&ccnt[slot[j]], 1u);
            pend &= ~(1u << j);
          } else {
            slot[j] = (slot[j] + 1) & (SLOTS - 1);
          }
        } else {
          slot[j] = (slot[j] + 1) & (SLOTS - 1);
        }
      }
    }
    #pragma unroll
    for (int j = 0; j < ILP; ++j)  // pathological bucket: global table
      if (pend & (1u << j))
        ht_add(k[j], p[j], 1, tkeys, tvals, texm, cap_mask);
  }
  __syncthreads();
  for (int s = threadIdx.x; s < SLOTS; s += blockDim.x)
    if (ckeys[s] != HT_EMPTY && ccnt[s])
      ht_add(ckeys[s], cpos[s], (i64)ccnt[s], tkeys, tvals, texm, cap_mask);
}

// ---------------------------------------------------------------------------
// K5 (aggregation form): open-addressing hash table, linear probing.
// Combiner for declared associative+commutative reducers (job.lua:104-106 —
// the reference's own fast-path flags select this path).
// ---------------------------------------------------------------------------
// Table: tkeys (HT_EMPTY = free), tvals (i64 sum), texm (first-inserter
// exemplar pos; 0 if untracked).  cap is a power of two.

__device__ void ht_add(u64 k, u64 p, i64 cnt, u64* tkeys, i64* tvals,
                       u64* texm, u64 cap_mask) {
  u32 slot = first_slot(k, cap_mask);
  while (true) {
    u64 cur = tkeys[slot];
    if (cur == k) {
      atomicAdd((unsigned long long*)&tvals[slot], (unsigned long long)cnt);
      return;
    }
    if (cur == HT_EMPTY) {
      u64 prev = atomicCAS((unsigned long long*)&tkeys[slot],
                           (unsigned long long)HT_EMPTY,
                           (unsigned long long)k);
      if (prev == HT_EMPTY) {
        if (texm) texm[slot] = p;  // first inserter records the exemplar;
                                   // consumed only after kernel completion
        atomicAdd((unsigned long long*)&tvals[slot], (unsigned long long)cnt);
        return;
      }
      if (prev == k) {
        atomicAdd((unsigned long long*)&tvals[slot], (unsigned long long)cnt);
        return;
      }
    }
    slot = (u32)((slot + 1) & cap_mask);
  }
}

__global__ void hash_insert_count_kernel(const u64* __restrict__ keys,
                                         const u64* __restrict__ pos,
                                         long n, u64* __restrict__ tkeys,
                                         i64* __restrict__ tvals,
                                         u64* __restrict__ texm,
                                         u64 cap_mask) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  for (; i < n; i += stride)
    ht_add(remap_key(keys[i]), pos ? pos[i] : 0, 1, tkeys, tvals, texm,
           cap_mask);
}

// generic (key, i64 value) insert — gradient counts, inverted-index sizes...
__global__ void hash_insert_sum_i64_kernel(const u64* __restrict__ keys,
                                           const i64* __restrict__ vals,
                                           long n, u64* __restrict__ tkeys,
                                           i64* __restrict__ tvals,
                                           u64 cap_mask) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    u64 k = remap_key(keys[i]);
    i64 v = vals[i];
    u32 slot = first_slot(k, cap_mask);
    while (true) {
      u64 cur = tkeys[slot];
      if (cur == k) {
        atomicAdd((unsigned long long*)&tvals[slot], (unsigned long long)v);
        break;
      }
      if (cur == HT_EMPTY) {
        u64 prev = atomicCAS((unsigned long long*)&tkeys[slot],
                             (unsigned long long)HT_EMPTY,
                             (unsigned long long)k);
        if (prev == HT_EMPTY || prev == k) {
          atomicAdd((unsigned long long*)&tvals[slot], (unsigned long long)v);
          break;
        }
      }
      slot = (u32)((slot + 1) & cap_mask);
    }
  }
}

__global__ void hash_extract_kernel(const u64* __restrict__ tkeys,
                                    const i64* __restrict__ tvals,
                                    const u64* __restrict__ texm, long cap,
                                    u64* __restrict__ okeys,
                                    i64* __restrict__ ovals,
                                    u64* __restrict__ opos,
                                    unsigned long long* __restrict__ counter) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  for (; i < cap; i += stride) {
    u64 k = tkeys[i];
    if (k != HT_EMPTY) {
      unsigned long long idx = atomicAdd(counter, 1ull);
      okeys[idx] = k;
      ovals[idx] = tvals[i];
      if (opos && texm) opos[idx] = texm[i];
    }
  }
}

// v2 extract: wave-chunked compaction.  v1's one-atomic-per-wave on the
// shared counter serializes cross-XCD (measured 6.3 ms scanning a 2^25
// table); v2 reserves 256-entry chunks per wave and pads unused tail
// slots with HT_EMPTY keys — consumers mask/trim them.  Used for large
// tables; v1 remains the no-padding path for small ones.
__global__ __launch_bounds__(256) void hash_extract_v2_kernel(
    const u64* __restrict__ tkeys, const i64* __restrict__ tvals,
    const u64* __restrict__ texm, long cap, u64* __restrict__ okeys,
    i64* __restrict__ ovals, u64* __restrict__ opos,
    unsigned long long* __restrict__ counter, long ocap) {
  constexpr int CHUNK = 256;
  const int lane = threadIdx.x & (WAVE - 1);
  const u64 lt = ((u64)1 << lane) - 1;
  long w0 = ((long)blockIdx.x * blockDim.x + threadIdx.x) / WAVE;
  long nw = ((long)gridDim.x * blockDim.x) / WAVE;
  long wchunk = -1;
  int wleft = 0;
  for (long base = w0 * WAVE; base < cap; base += nw * WAVE) {
    long i = base + lane;
    bool valid = i < cap;
    u64 k = valid ? tkeys[i] : HT_EMPTY;
    bool ne = valid && k != HT_EMPTY;
    u64 mm = __ballot(ne);
    int tot = __popcll(mm);
    if (tot > wleft) {
      for (int j = lane; j < wleft; j += WAVE)
        if (wchunk + j < ocap) okeys[wchunk + j] = HT_EMPTY;
      unsigned long long nb = 0;
      if (lane == 0)
        nb = atomicAdd(counter, (unsigned long long)CHUNK);
      wchunk = (long)__shfl(nb, 0, WAVE);
      wleft = CHUNK;
    }
    if (ne) {
      long o = wchunk + __popcll(mm & lt);
      if (o < ocap) {
        okeys[o] = k;
        ovals[o] = tvals[i];
        if (opos && texm) opos[o] = texm[i];
      }
    }
    wchunk += tot;
    wleft -= tot;
  }
  for (int j = lane; j < wleft; j += WAVE)
    if (wchunk + j < ocap) okeys[wchunk + j] = HT_EMPTY;
}

// ---------------------------------------------------------------------------
// K5 (sorted form): segmented reduce-by-key over a key-sorted run.
// head_flags + (host cumsum) + scatter stage; K4's k-way merge becomes
// "sort once, then segment" (SURVEY.md K4).
// ---------------------------------------------------------------------------

__global__ void head_flags_kernel(const u64* __restrict__ keys, long n,
                                  i64* __restrict__ flags) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  for (; i < n; i += stride)
    flags[i] = (i == 0) || (keys[i] != keys[i - 1]);
}

// seg[i] = (inclusive cumsum of flags)[i] - 1; scatter keys at heads, add vals
__global__ void seg_scatter_i64_kernel(const u64* __restrict__ keys,
                                       const i64* __restrict__ vals,
                                       const i64* __restrict__ seg, long n,
                                       u64* __restrict__ okeys,
                                       i64* __restrict__ ovals) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    i64 s = seg[i] - 1;
    if (i == 0 || seg[i] != seg[i - 1]) okeys[s] = keys[i];
    atomicAdd((unsigned long long*)&ovals[s],
              (unsigned long long)(vals ? vals[i] : 1));
  }
}

// min/max variants of the segmented scatter-reduce — the other canonical
// associative+commutative+idempotent reducers the fast-path property
// flags admit (job.lua:104-106; min/max are idempotent, so they are safe
// even under the combiner's re-application).  Signed i64 comparison;
// ovals must be pre-initialized to INT64_MAX (min) / INT64_MIN (max) by
// the host wrapper.
template <bool IS_MIN>
__global__ void seg_scatter_i64_minmax_kernel(
    const u64* __restrict__ keys, const i64* __restrict__ vals,
    const i64* __restrict__ seg, long n, u64* __restrict__ okeys,
    i64* __restrict__ ovals) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    i64 s = seg[i] - 1;
    if (i == 0 || seg[i] != seg[i - 1]) okeys[s] = keys[i];
    if (IS_MIN)
      atomicMin((long long*)&ovals[s], (long long)vals[i]);
    else
      atomicMax((long long*)&ovals[s], (long long)vals[i]);
  }
}

// f64 twin (HIP provides native double atomicMin/Max); ovals
// pre-initialized to +inf / -inf by the host wrapper
template <bool IS_MIN>
__global__ void seg_scatter_f64_minmax_kernel(
    const u64* __restrict__ keys, const double* __restrict__ vals,
    const i64* __restrict__ seg, long n, u64* __restrict__ okeys,
    double* __restrict__ ovals) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    i64 s = seg[i] - 1;
    if (i == 0 || seg[i] != seg[i - 1]) okeys[s] = keys[i];
    if (IS_MIN)
      atomicMin(&ovals[s], vals[i]);
    else
      atomicMax(&ovals[s], vals[i]);
  }
}

// pick one auxiliary value (e.g. exemplar pos) per segment: first element
__global__ void seg_first_u64_kernel(const u64* __restrict__ aux,
                                     const i64* __restrict__ seg, long n,
                                     u64* __restrict__ oaux) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  for (; i < n; i += stride)
    if (i == 0 || seg[i] != seg[i - 1]) oaux[seg[i] - 1] = aux[i];
}

__global__ void seg_scatter_f64_kernel(const u64* __restrict__ keys,
                                       const double* __restrict__ vals,
                                       const i64* __restrict__ seg, long n,
                                       u64* __restrict__ okeys,
                                       double* __restrict__ ovals) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    i64 s = seg[i] - 1;
    if (i == 0 || seg[i] != seg[i - 1]) okeys[s] = keys[i];
    atomicAdd(&ovals[s], vals[i]);
  }
}

// ---------------------------------------------------------------------------
// K2: partition histogram — send counts for the RCCL all-to-all (C5)
// ---------------------------------------------------------------------------

#define MAX_PARTS 1024

__global__ void partition_hist_kernel(const u64* __restrict__ keys, long n,
                                      u32 nparts, i64* __restrict__ hist) {
  __shared__ i64 lh[MAX_PARTS];
  for (u32 p = threadIdx.x; p < nparts; p += blockDim.x) lh[p] = 0;
  __syncthreads();
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  for (; i < n; i += stride)
    atomicAdd((unsigned long long*)&lh[partition_of(keys[i], nparts)], 1ull);
  __syncthreads();
  for (u32 p = threadIdx.x; p < nparts; p += blockDim.x)
    if (lh[p]) atomicAdd((unsigned long long*)&hist[p],
                         (unsigned long long)lh[p]);
}

// ---------------------------------------------------------------------------
// K7/K8: gather exemplar word bytes into a packed blob (dictionary build)
// ---------------------------------------------------------------------------

__global__ void gather_bytes_kernel(const u8* __restrict__ text,
                                    const u64* __restrict__ pos,
                                    const i64* __restrict__ out_off, long n,
                                    u8* __restrict__ out) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  for (; i < n; i += stride) {
    u64 p = pos[i];
    long start = (long)(p >> 16);
    long len = (long)(p & 0xFFFF);
    long o = out_off[i];
    for (long j = 0; j < len; ++j) out[o + j] = text[start + j];
  }
}

// lengths from packed pos
__global__ void pos_len_kernel(const u64* __restrict__ pos, long n,
                               i64* __restrict__ lens) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  for (; i < n; i += stride) lens[i] = (i64)(pos[i] & 0xFFFF);
}
