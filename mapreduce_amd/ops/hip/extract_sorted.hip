// Hash table -> sorted, packed result in one native op (the post-drain tail
// of the word-count job).
//
// Keys in a hash table are unique, so ordering them needs neither a stable
// general-purpose sort nor a permutation to drag the payloads through: sort
// MSD-first into bins of a few tens of keys, then give every key of a bin
// its rank = the number of smaller keys in that bin.  The rank is a pure
// function of the key set, so the output never depends on the order in
// which atomics arrive.
//
//   1. xs_hist       bins[top bits of key] += 1 per occupied slot (atomics
//                    spread over the bin array, no return value)
//   2. xs_bin_scan   one block: bin offsets, n, overflow flag -> meta
//   3. xs_scatter    occupied slot -> (key, slot) at bin_off + per-bin
//                    cursor (the bin's own counter, counted back down);
//                    order inside a bin is arbitrary here
//   4. xs_rank       one wave per bin: keys to LDS, rank by counting,
//                    write key / count / pos / len at bin_off + rank
//   5. xs_tile_sums  per-tile sums of lens
//   6. xs_offs_scan  offs = exclusive scan of lens, total_bytes -> meta
//
// n is known only on the device: kernels read it from meta[0], and the
// packed buffer [keys | counts | lens] is laid out at stride n inside an
// allocation of 3 * cap.  A bin longer than XS_RANK_M raises meta[2]; its
// keys are not written and the caller falls back to the general path.
#pragma once

#include "common.h"

#define XS_BLOCK 256
#define XS_WAVES (XS_BLOCK / WAVE)
#define XS_RANK_M 512            // keys one wave ranks in LDS
#define XS_SCAN_ITEMS 8
#define XS_SCAN_TILE (XS_BLOCK * XS_SCAN_ITEMS)  // lens per offsets block
#define XS_BINSCAN_BLOCK 1024
#define XS_SLOTS_PER_BIN 64      // bins = cap / 64: <= 64 keys a bin on
                                 // average even in a full table

// shift == 64 means one bin (tables of up to XS_SLOTS_PER_BIN slots)
DEV u32 xs_bin(u64 k, int shift) {
  return shift >= 64 ? 0u : (u32)(k >> shift);
}

__global__ __launch_bounds__(XS_BLOCK) void xs_hist_kernel(
    const u64* __restrict__ tkeys, long cap, int shift,
    u32* __restrict__ bins) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  for (; i < cap; i += stride) {
    u64 k = tkeys[i];
    if (k != HT_EMPTY) atomicAdd(&bins[xs_bin(k, shift)], 1u);
  }
}

// block-wide inclusive scan of one u32 per thread (Hillis-Steele in LDS);
// every thread of the block must call it
template <int N>
DEV u32 xs_block_incl_scan_u32(u32 v, u32* sh) {
  int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int off = 1; off < N; off <<= 1) {
    u32 o = t >= off ? sh[t - off] : 0u;
    __syncthreads();
    sh[t] += o;
    __syncthreads();
  }
  return sh[t];
}

template <int N>
DEV i64 xs_block_incl_scan_i64(i64 v, i64* sh) {
  int t = threadIdx.x;
  sh[t] = v;
  __syncthreads();
  for (int off = 1; off < N; off <<= 1) {
    i64 o = t >= off ? sh[t - off] : 0;
    __syncthreads();
    sh[t] += o;
    __syncthreads();
  }
  return sh[t];
}

// one block: bin_off[0..nbins] = exclusive scan of bins, meta = [n, 0,
// any bin > XS_RANK_M].  Each thread owns a contiguous run of bins.
__global__ __launch_bounds__(XS_BINSCAN_BLOCK) void xs_bin_scan_kernel(
    const u32* __restrict__ bins, int nbins, u32* __restrict__ bin_off,
    i64* __restrict__ meta) {
  __shared__ u32 sh[XS_BINSCAN_BLOCK];
  __shared__ u32 over;
  int t = threadIdx.x;
  if (t == 0) over = 0;
  int per = (nbins + XS_BINSCAN_BLOCK - 1) / XS_BINSCAN_BLOCK;
  int b0 = t * per;
  int b1 = b0 + per < nbins ? b0 + per : nbins;
  u32 sum = 0, mx = 0;
  for (int b = b0; b < b1; ++b) {
    u32 c = bins[b];
    sum += c;
    mx = c > mx ? c : mx;
  }
  u32 incl = xs_block_incl_scan_u32<XS_BINSCAN_BLOCK>(sum, sh);
  if (mx > XS_RANK_M) over = 1;  // benign same-value race
  u32 run = incl - sum;
  for (int b = b0; b < b1; ++b) {
    bin_off[b] = run;
    run += bins[b];
  }
  __syncthreads();
  if (t == XS_BINSCAN_BLOCK - 1) {
    bin_off[nbins] = incl;
    meta[0] = (i64)incl;
    meta[1] = 0;
    meta[2] = (i64)over;
  }
}

__global__ __launch_bounds__(XS_BLOCK) void xs_scatter_kernel(
    const u64* __restrict__ tkeys, long cap, int shift,
    u32* __restrict__ bins, const u32* __restrict__ bin_off,
    u64* __restrict__ bkeys, u32* __restrict__ bslot) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  for (; i < cap; i += stride) {
    u64 k = tkeys[i];
    if (k != HT_EMPTY) {
      u32 b = xs_bin(k, shift);
      // the bin's count is its cursor: old value in [1, size]
      u32 c = atomicSub(&bins[b], 1u);
      u32 dst = bin_off[b] + c - 1;  // < n <= cap
      bkeys[dst] = k;
      bslot[dst] = (u32)i;
    }
  }
}

// one wave per bin.  texm == nullptr when the table tracks no exemplars:
// then only keys and counts are written.
__global__ __launch_bounds__(XS_BLOCK) void xs_rank_kernel(
    const u64* __restrict__ bkeys, const u32* __restrict__ bslot,
    const u32* __restrict__ bin_off, int nbins,
    const i64* __restrict__ tvals, const u64* __restrict__ texm,
    const i64* __restrict__ meta, i64* __restrict__ packed,
    u64* __restrict__ opos) {
  __shared__ u64 lk[XS_WAVES][XS_RANK_M];
  int w = threadIdx.x / WAVE;
  int lane = threadIdx.x % WAVE;
  long bin = (long)blockIdx.x * XS_WAVES + w;
  u32 s = 0, m = 0;
  if (bin < nbins) {
    s = bin_off[bin];
    m = bin_off[bin + 1] - s;
  }
  if (m > XS_RANK_M) m = 0;  // overflow: skipped, meta[2] is already set
  for (u32 j = lane; j < m; j += WAVE) lk[w][j] = bkeys[s + j];
  __syncthreads();
  long n = meta[0];
  for (u32 j = lane; j < m; j += WAVE) {
    u64 k = lk[w][j];
    u32 r = 0;
    for (u32 t = 0; t < m; ++t) r += lk[w][t] < k ? 1u : 0u;
    long dst = (long)s + r;
    u32 slot = bslot[s + j];
    packed[dst] = (i64)k;
    packed[n + dst] = tvals[slot];
    if (texm) {
      u64 p = texm[slot];
      opos[dst] = p;
      packed[2 * n + dst] = (i64)(p & 0xFFFF);
    }
  }
}

// tile_sums[t] = sum of lens[t * TILE, min((t + 1) * TILE, n))
__global__ __launch_bounds__(XS_BLOCK) void xs_tile_sums_kernel(
    const i64* __restrict__ packed, const i64* __restrict__ meta,
    i64* __restrict__ tile_sums) {
  __shared__ i64 wsum[XS_WAVES];
  long n = meta[0];
  long start = (long)blockIdx.x * XS_SCAN_TILE;
  if (start >= n) return;  // uniform over the block
  const i64* lens = packed + 2 * n;
  i64 acc = 0;
  #pragma unroll
  for (int j = 0; j < XS_SCAN_ITEMS; ++j) {
    long i = start + (long)j * XS_BLOCK + threadIdx.x;
    acc += i < n ? lens[i] : 0;
  }
  acc = wave_sum_i64(acc);
  if (threadIdx.x % WAVE == 0) wsum[threadIdx.x / WAVE] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    i64 sum = 0;
    for (int w = 0; w < XS_WAVES; ++w) sum += wsum[w];
    tile_sums[blockIdx.x] = sum;
  }
}

// offs = exclusive scan of lens; every block re-reduces the tile sums
// before it (at most cap / TILE of them), then scans its own tile.  The
// block that holds the last element writes total_bytes.
__global__ __launch_bounds__(XS_BLOCK) void xs_offs_scan_kernel(
    const i64* __restrict__ packed, i64* __restrict__ meta,
    const i64* __restrict__ tile_sums, i64* __restrict__ offs) {
  __shared__ i64 sh[XS_BLOCK];
  __shared__ i64 wsum[XS_WAVES];
  long n = meta[0];
  long start = (long)blockIdx.x * XS_SCAN_TILE;
  if (start >= n) return;  // uniform over the block
  const i64* lens = packed + 2 * n;
  i64 part = 0;
  for (long t = threadIdx.x; t < (long)blockIdx.x; t += XS_BLOCK)
    part += tile_sums[t];
  part = wave_sum_i64(part);
  if (threadIdx.x % WAVE == 0) wsum[threadIdx.x / WAVE] = part;
  // thread t owns the XS_SCAN_ITEMS consecutive elements from i0
  long i0 = start + (long)threadIdx.x * XS_SCAN_ITEMS;
  i64 v[XS_SCAN_ITEMS];
  i64 tsum = 0;
  #pragma unroll
  for (int j = 0; j < XS_SCAN_ITEMS; ++j) {
    v[j] = i0 + j < n ? lens[i0 + j] : 0;
    tsum += v[j];
  }
  i64 incl = xs_block_incl_scan_i64<XS_BLOCK>(tsum, sh);  // syncs wsum too
  i64 base = 0;
  for (int w = 0; w < XS_WAVES; ++w) base += wsum[w];
  i64 run = base + incl - tsum;
  #pragma unroll
  for (int j = 0; j < XS_SCAN_ITEMS; ++j) {
    if (i0 + j < n) offs[i0 + j] = run;
    run += v[j];
  }
  if (threadIdx.x == XS_BLOCK - 1 && start + XS_SCAN_TILE >= n)
    meta[1] = base + incl;
}
