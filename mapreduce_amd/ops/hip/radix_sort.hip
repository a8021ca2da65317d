// LSD radix sort for u64 keys (+ u64 payload), CDNA4-native.
//
// 8-bit digits, LDS digit histograms, stable tile-local ranking via
// wave64 ballots (8 single-bit ballots build the same-digit lane mask; the
// lowest lane of each digit group publishes the group count to LDS, a
// 256-thread prefix orders waves deterministically).  Per pass:
//   1. radix_hist_kernel     — per-tile 256-bin LDS histogram, written
//                              digit-major: hist[d * ntiles + t]
//   2. (host) exclusive scan of the flat [256 * ntiles] array — digit-major
//      order makes the scan produce exactly base[d][t]
//   3. radix_scatter_kernel  — stable scatter to base[d][t] + local rank
//
// SKIP mode (spill-drain bucketize only): records whose key is HT_EMPTY —
// the spill allocator's chunk-tail pads — are neither counted nor written,
// so they stop at the first kernel that reads them.  The predicate is
// rs_live<SKIP>() in BOTH kernels; SKIP=false compiles to the plain pass
// (real sort keys may legitimately be all-ones).
//
// Replaces the reference's table.sort + heap merge (job.lua:194,
// utils.lua:206-271): sort once, then segment (K4 -> K1+K5).

#include "common.h"

#define RS_BLOCK 256
#define RS_WAVES (RS_BLOCK / WAVE)
#define RS_ITEMS 8
#define RS_TILE (RS_BLOCK * RS_ITEMS)
#define RS_BINS 256

// ITEMS (elements/thread) sets the tile: 8 -> 2048 (38 KB LDS in the
// v2 scatter, 4 blocks/CU); 4 -> 1024 (22 KB, 7 blocks/CU) — occupancy
// vs digit-run length (write coalescing) tradeoff, selected per size by
// MR_RS_ITEMS.
template <bool SKIP>
DEV bool rs_live(u64 k) { return !SKIP || k != HT_EMPTY; }

// WIDE: a full, 16-byte-aligned tile is read two keys per load with all of
// a thread's loads issued before its first LDS atomic (which keys a thread
// counts does not matter to a histogram).
// HT: histogram entry type.  i64 feeds the torch cumsum of the full sort;
// u32 (a tile holds <= 2048 records) feeds the native bucketize scan.
template <int ITEMS, bool SKIP = false, typename HT = i64, bool WIDE = false>
__global__ __launch_bounds__(RS_BLOCK) void radix_hist_kernel(
    const u64* __restrict__ keys, long n, int shift, long ntiles,
    HT* __restrict__ hist) {
  __shared__ u32 lh[RS_BINS];
  for (int b = threadIdx.x; b < RS_BINS; b += blockDim.x) lh[b] = 0;
  __syncthreads();
  long tile = blockIdx.x;
  long base = tile * (RS_BLOCK * ITEMS);
  if (WIDE && base + RS_BLOCK * ITEMS <= n &&
      ((unsigned long long)keys & 15) == 0) {
    // full tile, 16-byte aligned: two keys per load, every load of the
    // thread issued before the first LDS atomic
    const ulonglong2* p = reinterpret_cast<const ulonglong2*>(keys + base);
    ulonglong2 q[ITEMS / 2];
    #pragma unroll
    for (int j = 0; j < ITEMS / 2; ++j) q[j] = p[j * RS_BLOCK + threadIdx.x];
    #pragma unroll
    for (int j = 0; j < ITEMS / 2; ++j) {
      if (rs_live<SKIP>(q[j].x))
        atomicAdd(&lh[(u32)((q[j].x >> shift) & 0xFF)], 1u);
      if (rs_live<SKIP>(q[j].y))
        atomicAdd(&lh[(u32)((q[j].y >> shift) & 0xFF)], 1u);
    }
  } else {
    for (int r = 0; r < ITEMS; ++r) {
      long i = base + r * RS_BLOCK + threadIdx.x;
      if (i < n) {
        u64 k = keys[i];
        if (rs_live<SKIP>(k)) atomicAdd(&lh[(u32)((k >> shift) & 0xFF)], 1u);
      }
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < RS_BINS; b += blockDim.x)
    hist[(long)b * ntiles + tile] = (HT)lh[b];
}

// v2: LDS-staged scatter.  v1 writes each element straight to its global
// position — 16 B granules scattered across 256 digit destinations, so
// nearly every write wastes most of its cache line.  v2 first reorders the
// whole tile in LDS by (digit, stable rank), then streams it out in stage
// order: consecutive lanes write consecutive positions of each digit run
// (avg run = TILE/256 elements), restoring write coalescing.
// digit_start_in_tile comes from a 256-entry LDS prefix over this tile's
// histogram (recomputed; must equal radix_hist_kernel's counts).
// VT: payload type.  u64 = the general (key, value) sort; u32 = the
// permutation-index sort (radix_sort_idx32) — 4 B payloads cut per-pass
// payload traffic in half AND halve the stage_v LDS (38 -> 30 KB/block,
// one extra resident block), for callers that gather their real payload
// once through the final permutation instead of dragging it through
// every pass (TeraSort, sort_by_key).
// SKIP: drop HT_EMPTY records (see header); the tile then stages only
// digit_start[RS_BINS] <= tile_n records and streams out exactly those.
// BT: base_dx entry type (i64 from the torch scan, u32 from the native one).
template <int ITEMS, typename VT = u64, bool SKIP = false, typename BT = i64>
__global__ __launch_bounds__(RS_BLOCK) void radix_scatter_v2_kernel(
    const u64* __restrict__ keys, const VT* __restrict__ vals, long n,
    int shift, long ntiles, const BT* __restrict__ base_dx,
    u64* __restrict__ okeys, VT* __restrict__ ovals) {
  __shared__ u32 wavecnt[RS_WAVES][RS_BINS];
  __shared__ u32 cnt_base[RS_BINS];     // running per-digit counts
  __shared__ u32 digit_start[RS_BINS + 1];
  __shared__ u64 stage_k[(RS_BLOCK * ITEMS)];
  __shared__ VT stage_v[(RS_BLOCK * ITEMS)];
  for (int b = threadIdx.x; b < RS_BINS; b += blockDim.x) cnt_base[b] = 0;
  long tile = blockIdx.x;
  long tbase = tile * (RS_BLOCK * ITEMS);
  long tile_n = n - tbase < (RS_BLOCK * ITEMS) ? n - tbase : (RS_BLOCK * ITEMS);
  int wave = threadIdx.x / WAVE;
  int lane = threadIdx.x % WAVE;
  u64 lt_mask = ((u64)1 << lane) - 1;
  bool has_vals = ovals != nullptr;

  // ---- per-tile digit histogram + exclusive prefix -> digit_start
  __syncthreads();
  for (int r = 0; r < ITEMS; ++r) {
    long i = tbase + (long)r * RS_BLOCK + threadIdx.x;
    if (i < n) {
      u64 k = keys[i];
      if (rs_live<SKIP>(k))
        atomicAdd(&cnt_base[(u32)((k >> shift) & 0xFF)], 1u);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    u32 run = 0;
    for (int d = 0; d < RS_BINS; ++d) {  // serial 256-step scan: ~cheap
      digit_start[d] = run;
      run += cnt_base[d];
    }
    digit_start[RS_BINS] = run;
  }
  __syncthreads();
  for (int b = threadIdx.x; b < RS_BINS; b += blockDim.x) cnt_base[b] = 0;
  __syncthreads();

  // ---- stable rank + stage into LDS at (digit_start + tile_rank)
  for (int r = 0; r < ITEMS; ++r) {
    for (int b = threadIdx.x; b < RS_BINS; b += blockDim.x)
      for (int w = 0; w < RS_WAVES; ++w) wavecnt[w][b] = 0;
    __syncthreads();
    long i = tbase + (long)r * RS_BLOCK + threadIdx.x;
    bool valid = i < n;
    u64 k = valid ? keys[i] : 0;
    valid = valid && rs_live<SKIP>(k);
    u32 d = valid ? (u32)((k >> shift) & 0xFF) : 0;
    u64 m = __ballot(valid);
    #pragma unroll
    for (int b = 0; b < 8; ++b) {
      u64 bb = __ballot(valid && ((d >> b) & 1));
      m &= ((d >> b) & 1) ? bb : ~bb;
    }
    u32 lane_rank = 0;
    if (valid) {
      lane_rank = (u32)__popcll(m & lt_mask);
      int leader = __ffsll((unsigned long long)m) - 1;
      if (lane == leader) wavecnt[wave][d] = (u32)__popcll(m);
    }
    __syncthreads();
    if (threadIdx.x < RS_BINS) {
      u32 run = cnt_base[threadIdx.x];
      #pragma unroll
      for (int w = 0; w < RS_WAVES; ++w) {
        u32 c = wavecnt[w][threadIdx.x];
        wavecnt[w][threadIdx.x] = run;
        run += c;
      }
      cnt_base[threadIdx.x] = run;
    }
    __syncthreads();
    if (valid) {
      u32 s = digit_start[d] + wavecnt[wave][d] + lane_rank;
      stage_k[s] = k;
      if (has_vals) stage_v[s] = vals[i];
    }
    __syncthreads();
  }

  // ---- stream out in stage order: coalesced within each digit run.
  // SKIP staged only the live records: slots past digit_start[RS_BINS]
  // were never written and must not be read.
  long nstage = SKIP ? (long)digit_start[RS_BINS] : tile_n;
  for (long s = threadIdx.x; s < nstage; s += blockDim.x) {
    u64 k = stage_k[s];
    u32 d = (u32)((k >> shift) & 0xFF);
    u32 local = (u32)s - digit_start[d];
    long pos = (long)base_dx[(long)d * ntiles + tile] + local;
    okeys[pos] = k;
    if (has_vals) ovals[pos] = stage_v[s];
  }
}

DEV u32 wave_incl_scan_u32(u32 v, int lane) {
  #pragma unroll
  for (int off = 1; off < WAVE; off <<= 1) {
    u32 o = __shfl_up(v, off, WAVE);
    if (lane >= off) v += o;
  }
  return v;
}

// v3: the v2 scatter with the ranking's waits taken out — same arguments,
// same (bit-identical, stable) output, default since MR_RADIX_V2=1 became
// the A/B switch.  Per tile:
//   1. blocked mapping, loaded once: wave w, round r, lane l owns tile index
//      (w*ITEMS + r)*64 + l, so (wave, round, lane) order IS index order.
//      All ITEMS keys go to registers up front with every load in flight,
//      so no load latency is left inside the ranking.  The payload comes
//      with them, or (LATE) is fetched at staging time by the lanes that
//      stage a record; which is faster depends on the caller (ops_ext.hip).
//   2. wave-private ranking, no block barrier: wcnt[wave][d] carries the
//      digit-d count of this wave's EARLIER rounds; a lane's in-wave rank is
//      that plus popc(same-digit lanes below it); the group's leader then
//      adds the group size.  Rounds depend on each other only through one
//      wave's own LDS row, ordered by a wavefront-scope fence.
//   3. one cross-wave pass: thread b turns wcnt[0..3][b] into exclusive
//      wave bases and the digit total (= the tile histogram; no separate
//      histogram phase, no second key read), a 256-thread wave scan + four
//      wave sums gives digit_start, which is folded straight into
//      wcnt[w][b] = digit_start[b] + wavebase[w][b] and
//      gbase[b] = base[b][tile] - digit_start[b] (base loaded at entry).
//   4. stage at wcnt[wave][d] + rank, barrier, stream out to gbase[d] + s.
// LDS: wcnt + gbase + the two stages — v2's footprint minus cnt_base and
// digit_start (the four wave sums borrow stage_k[0..3], which is not
// written before the barrier that follows their last read).
template <int ITEMS, typename VT = u64, bool SKIP = false, typename BT = i64,
          bool LATE = false>
__global__ __launch_bounds__(RS_BLOCK) void radix_scatter_v3_kernel(
    const u64* __restrict__ keys, const VT* __restrict__ vals, long n,
    int shift, long ntiles, const BT* __restrict__ base_dx,
    u64* __restrict__ okeys, VT* __restrict__ ovals) {
  static_assert(RS_BLOCK == RS_BINS, "thread b owns digit b");
  __shared__ u32 wcnt[RS_WAVES][RS_BINS];
  __shared__ BT gbase[RS_BINS];
  __shared__ u64 stage_k[(RS_BLOCK * ITEMS)];
  __shared__ VT stage_v[(RS_BLOCK * ITEMS)];
  long tile = blockIdx.x;
  long tbase = tile * (RS_BLOCK * ITEMS);
  long tile_n = n - tbase < (RS_BLOCK * ITEMS) ? n - tbase : (RS_BLOCK * ITEMS);
  int wave = threadIdx.x / WAVE;
  int lane = threadIdx.x % WAVE;
  u64 lt_mask = ((u64)1 << lane) - 1;
  bool has_vals = ovals != nullptr;

  // ---- everything this thread reads from global memory, issued at once.
  // Loads past the end re-read the last record instead of being
  // predicated: a "load or keep the register" select makes the compiler
  // branch around each load and wait for the earlier ones first.
  BT my_base = base_dx[(long)threadIdx.x * ntiles + tile];
  long i0 = tbase + (long)(wave * ITEMS) * WAVE + lane;
  u64 k[ITEMS];
  VT v[ITEMS];
  bool valid[ITEMS];
  #pragma unroll
  for (int r = 0; r < ITEMS; ++r) {
    long i = i0 + (long)r * WAVE;
    k[r] = keys[i < n ? i : n - 1];
  }
  if (has_vals && !LATE) {
    // a pad's payload is fetched and dropped rather than making every
    // payload load wait for its key
    #pragma unroll
    for (int r = 0; r < ITEMS; ++r) {
      long i = i0 + (long)r * WAVE;
      v[r] = vals[i < n ? i : n - 1];
    }
  } else {
    #pragma unroll
    for (int r = 0; r < ITEMS; ++r) v[r] = 0;
  }
  #pragma unroll
  for (int r = 0; r < ITEMS; ++r)
    valid[r] = i0 + (long)r * WAVE < n && rs_live<SKIP>(k[r]);

  // ---- wave-private stable ranks (this wave's wcnt row only)
  #pragma unroll
  for (int b = lane; b < RS_BINS; b += WAVE) wcnt[wave][b] = 0;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  u32 rank[ITEMS];
  #pragma unroll
  for (int r = 0; r < ITEMS; ++r) {
    u32 d = valid[r] ? (u32)((k[r] >> shift) & 0xFF) : 0;
    u64 m = __ballot(valid[r]);
    #pragma unroll
    for (int b = 0; b < 8; ++b) {
      u64 bb = __ballot(valid[r] && ((d >> b) & 1));
      m &= ((d >> b) & 1) ? bb : ~bb;
    }
    u32 prev = valid[r] ? wcnt[wave][d] : 0;
    rank[r] = prev + (u32)__popcll(m & lt_mask);
    // every lane's read of this round precedes the leaders' updates ...
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (valid[r] && lane == __ffsll((unsigned long long)m) - 1)
      wcnt[wave][d] = prev + (u32)__popcll(m);
    // ... which precede every lane's read of the next round
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();

  // ---- one cross-wave pass: thread b owns digit b
  u32 wb[RS_WAVES];
  u32 total = 0;
  #pragma unroll
  for (int w = 0; w < RS_WAVES; ++w) {
    wb[w] = total;
    total += wcnt[w][threadIdx.x];
  }
  u32 incl = wave_incl_scan_u32(total, lane);
  if (lane == WAVE - 1) stage_k[wave] = incl;  // wave sums, see header
  __syncthreads();
  u32 pre = 0, all = 0;
  #pragma unroll
  for (int w = 0; w < RS_WAVES; ++w) {
    u32 ws = (u32)stage_k[w];
    if (w < wave) pre += ws;
    all += ws;
  }
  u32 dstart = pre + incl - total;  // digit_start[b]
  #pragma unroll
  for (int w = 0; w < RS_WAVES; ++w) wcnt[w][threadIdx.x] = dstart + wb[w];
  gbase[threadIdx.x] = my_base - (BT)dstart;  // u32: wraps, undone at use
  __syncthreads();

  // ---- stage in (digit, stable rank) order: all slot reads, then all
  // writes, so the LDS latencies overlap instead of queueing per record
  #pragma unroll
  for (int r = 0; r < ITEMS; ++r) {
    u32 d = (u32)((k[r] >> shift) & 0xFF);
    rank[r] += valid[r] ? wcnt[wave][d] : 0;  // now the stage slot
  }
  #pragma unroll
  for (int r = 0; r < ITEMS; ++r) {
    if (valid[r]) {
      stage_k[rank[r]] = k[r];
      if (has_vals)
        stage_v[rank[r]] = LATE ? vals[i0 + (long)r * WAVE] : v[r];
    }
  }
  __syncthreads();

  // ---- stream out in stage order: coalesced within each digit run.
  // SKIP staged only the live records (`all` of them): slots past that
  // were never written and are not read.  Same batching: keys and
  // payloads, then bases, then the stores.
  u32 nstage = SKIP ? all : (u32)tile_n;
  long pos[ITEMS];
  #pragma unroll
  for (int j = 0; j < ITEMS; ++j) {
    u32 s = j * RS_BLOCK + threadIdx.x;
    k[j] = s < nstage ? stage_k[s] : 0;
    if (has_vals) v[j] = s < nstage ? stage_v[s] : (VT)0;
  }
  #pragma unroll
  for (int j = 0; j < ITEMS; ++j) {
    u32 s = j * RS_BLOCK + threadIdx.x;
    u32 d = (u32)((k[j] >> shift) & 0xFF);
    pos[j] = (long)(BT)(gbase[d] + (BT)s);
  }
  #pragma unroll
  for (int j = 0; j < ITEMS; ++j) {
    u32 s = j * RS_BLOCK + threadIdx.x;
    if (s < nstage) {
      okeys[pos[j]] = k[j];
      if (has_vals) ovals[pos[j]] = v[j];
    }
  }
}

__global__ __launch_bounds__(RS_BLOCK) void radix_scatter_kernel(
    const u64* __restrict__ keys, const u64* __restrict__ vals, long n,
    int shift, long ntiles, const i64* __restrict__ base_dx,
    u64* __restrict__ okeys, u64* __restrict__ ovals) {
  // wavecnt[w][d]: this round's digit-d count of wave w, then (after the
  // prefix phase) the exclusive tile-rank base for wave w's digit-d items.
  __shared__ u32 wavecnt[RS_WAVES][RS_BINS];
  __shared__ u32 cnt_base[RS_BINS];  // digit counts of earlier rounds
  for (int b = threadIdx.x; b < RS_BINS; b += blockDim.x) cnt_base[b] = 0;
  long tile = blockIdx.x;
  long tbase = tile * RS_TILE;
  int wave = threadIdx.x / WAVE;
  int lane = threadIdx.x % WAVE;
  u64 lt_mask = ((u64)1 << lane) - 1;

  for (int r = 0; r < RS_ITEMS; ++r) {
    for (int b = threadIdx.x; b < RS_BINS; b += blockDim.x)
      for (int w = 0; w < RS_WAVES; ++w) wavecnt[w][b] = 0;
    __syncthreads();

    long i = tbase + (long)r * RS_BLOCK + threadIdx.x;
    bool valid = i < n;
    u64 k = valid ? keys[i] : 0;
    u32 d = valid ? (u32)((k >> shift) & 0xFF) : 0;

    // same-digit lane mask among valid lanes (8 single-bit ballots)
    u64 m = __ballot(valid);
    #pragma unroll
    for (int b = 0; b < 8; ++b) {
      u64 bb = __ballot(valid && ((d >> b) & 1));
      m &= ((d >> b) & 1) ? bb : ~bb;
    }
    u32 lane_rank = 0;
    if (valid) {
      lane_rank = (u32)__popcll(m & lt_mask);
      int leader = __ffsll((unsigned long long)m) - 1;
      if (lane == leader) wavecnt[wave][d] = (u32)__popcll(m);
    }
    __syncthreads();

    // deterministic wave order: thread b prefixes digit b over waves
    if (threadIdx.x < RS_BINS) {
      u32 run = cnt_base[threadIdx.x];
      #pragma unroll
      for (int w = 0; w < RS_WAVES; ++w) {
        u32 c = wavecnt[w][threadIdx.x];
        wavecnt[w][threadIdx.x] = run;
        run += c;
      }
      cnt_base[threadIdx.x] = run;
    }
    __syncthreads();

    if (valid) {
      u32 tile_rank = wavecnt[wave][d] + lane_rank;
      long pos = base_dx[(long)d * ntiles + tile] + tile_rank;
      okeys[pos] = k;
      if (ovals) ovals[pos] = vals[i];
    }
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// Native scan between the bucketize histogram and scatter (two launches,
// RS_BINS blocks each) — replaces zeros + cumsum + subtract + row-sum +
// zeros(257) + cumsum over a [256 x ntiles] i64 array with two passes over
// a u32 one.
//   1. rs_row_totals_kernel: totals[d] = sum_t hist[d][t]
//   2. rs_row_scan_kernel:   bucket_off[d] = sum_{e<d} totals[e] (each block
//      re-reduces the 256 totals), then hist[d][t] <- bucket_off[d] +
//      exclusive row prefix, IN PLACE: the flat digit-major exclusive scan
//      base[d][t] the scatter consumes.  Positions are u32 (host checks
//      n < 2^32).
// ---------------------------------------------------------------------------
#define RS_SCAN_UNROLL 4

__global__ __launch_bounds__(RS_BLOCK) void rs_row_totals_kernel(
    const u32* __restrict__ hist, long ntiles, i64* __restrict__ totals) {
  __shared__ i64 wsum[RS_WAVES];
  const u32* row = hist + (long)blockIdx.x * ntiles;
  i64 acc = 0;
  for (long t0 = threadIdx.x; t0 < ntiles; t0 += RS_SCAN_UNROLL * RS_BLOCK) {
    u32 v[RS_SCAN_UNROLL];
    #pragma unroll
    for (int j = 0; j < RS_SCAN_UNROLL; ++j) {
      long t = t0 + (long)j * RS_BLOCK;
      v[j] = t < ntiles ? row[t] : 0;
    }
    #pragma unroll
    for (int j = 0; j < RS_SCAN_UNROLL; ++j) acc += v[j];
  }
  acc = wave_sum_i64(acc);
  if (threadIdx.x % WAVE == 0) wsum[threadIdx.x / WAVE] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    i64 s = 0;
    for (int w = 0; w < RS_WAVES; ++w) s += wsum[w];
    totals[blockIdx.x] = s;
  }
}

__global__ __launch_bounds__(RS_BLOCK) void rs_row_scan_kernel(
    u32* __restrict__ hist, long ntiles, const i64* __restrict__ totals,
    i64* __restrict__ bucket_off) {
  __shared__ i64 wsum[RS_WAVES];
  __shared__ u32 wpre[RS_SCAN_UNROLL * RS_WAVES];
  __shared__ i64 row_base;
  int d = blockIdx.x;
  int wave = threadIdx.x / WAVE;
  int lane = threadIdx.x % WAVE;
  // exclusive offset of digit d (+ the grand total from the last block)
  i64 tv = totals[threadIdx.x];  // RS_BLOCK == RS_BINS
  i64 part = wave_sum_i64(threadIdx.x < d ? tv : 0);
  if (lane == 0) wsum[wave] = part;
  __syncthreads();
  if (threadIdx.x == 0) {
    i64 s = 0;
    for (int w = 0; w < RS_WAVES; ++w) s += wsum[w];
    row_base = s;
    bucket_off[d] = s;
    if (d == RS_BINS - 1) bucket_off[RS_BINS] = s + totals[d];
  }
  __syncthreads();
  u32 carry = (u32)row_base;
  u32* row = hist + (long)d * ntiles;
  // RS_SCAN_UNROLL sub-chunks of RS_BLOCK entries per round: their loads
  // are issued together and one barrier pair serves all of them (the row
  // walk is latency-bound, not byte-bound)
  for (long t0 = 0; t0 < ntiles; t0 += RS_SCAN_UNROLL * RS_BLOCK) {
    u32 v[RS_SCAN_UNROLL], inc[RS_SCAN_UNROLL];
    #pragma unroll
    for (int j = 0; j < RS_SCAN_UNROLL; ++j) {
      long t = t0 + (long)j * RS_BLOCK + threadIdx.x;
      v[j] = t < ntiles ? row[t] : 0;
    }
    #pragma unroll
    for (int j = 0; j < RS_SCAN_UNROLL; ++j) {
      inc[j] = wave_incl_scan_u32(v[j], lane);
      if (lane == WAVE - 1) wpre[j * RS_WAVES + wave] = inc[j];
    }
    __syncthreads();
    u32 run = carry;
    #pragma unroll
    for (int j = 0; j < RS_SCAN_UNROLL; ++j) {
      #pragma unroll
      for (int w = 0; w < RS_WAVES; ++w) {
        if (w == wave) {
          long t = t0 + (long)j * RS_BLOCK + threadIdx.x;
          if (t < ntiles) row[t] = run + inc[j] - v[j];
        }
        run += wpre[j * RS_WAVES + w];
      }
    }
    carry = run;
    __syncthreads();
  }
}

// ---------------------------------------------------------------------------
// Payload gather through a u32 permutation: ONE streaming pass replaces
// dragging an 8-byte payload through all 8 radix passes (the
// radix_sort_idx32 pattern).  Reads are gathered (random within the
// pre-sort order), writes are fully coalesced.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gather_i64_u32_kernel(
    const i64* __restrict__ vals, const u32* __restrict__ idx, long n,
    i64* __restrict__ out) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  for (; i < n; i += stride) out[i] = vals[idx[i]];
}
