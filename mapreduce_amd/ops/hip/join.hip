// Equi-join of two key columns sorted ascending in u64 bit order: the join
// step of the reduce-side join (inner / left / semi / anti).
//
// Pass 1, bounds: lo[i] = the first right index with rk >= lk[i], cnt[i]
// = the length of the run of rk == lk[i] that starts there.  join_run does
// one row: a binary search for lo, then a galloping probe from lo and a
// binary search inside the last doubling, so a run of c rows costs
// ~2 log2 c loads, not log2 nr.  Two kernels give the same outputs:
//   join_bounds_kernel         thread per left row over the whole right
//                              column;
//   join_bounds_window_kernel  a block owns tiles of JOIN_BTILE left rows.
//       Wave 0 finds where the tile's first key starts in rk, wave 1 where
//       its last key ends: every row of the tile lands inside that window.
//       A window of at most JOIN_WIN keys is staged in LDS and searched
//       there; a longer one (a hot key) is searched in global memory, but
//       over the window alone.
// Semi and anti stop here.
//
// Host: off = exclusive cumsum(cnt'), cnt' = cnt (inner) or max(cnt, 1)
// (left); off[nl] = total sizes the output.
//
// Pass 2, join_expand_kernel: balanced by OUTPUT row.  A block owns tiles
// of JOIN_TILE consecutive output rows (capped grid, stride over tiles).
// Output row j belongs to the left row i with off[i] <= j < off[i + 1];
// ri = lo[i] + (j - off[i]), or -1 where cnt[i] == 0 (the pad row of an
// unmatched left row; only how="left" gives such a row an output slot).
// Per tile:
//   1. wave 0 finds i0 = the last left row with off <= the tile's first
//      output row, wave 1 finds i1 likewise for the tile's last row (two
//      searches in off, every lane of the wave on the same address);
//   2. the slice off[i0 .. i1] is staged in LDS.  n = i1 - i0 + 1 rows fit
//      when n <= JOIN_LDS_ROWS; otherwise LDS holds every k-th offset,
//      k = ceil(n / JOIN_LDS_ROWS), and the search below finishes its last
//      log2 k steps in global memory (the fallback; k == 1 never touches
//      global memory to search);
//   3. each thread resolves rows tile_start + r * JOIN_BLOCK + tid by
//      searching the staged slice, then stores li and ri: consecutive
//      lanes store consecutive i64, so both stores are coalesced.
// A left row whose run spans many tiles gives each of them i0 == i1: a
// one-entry slice, the cheapest tile there is.  A hot key is thus spread
// over total / JOIN_TILE blocks, not serialised on one lane.
//
// Control flow: every __syncthreads() is in block-uniform flow.  The tile
// loop runs on blockIdx.x, gridDim.x and ntiles alone; i0 and i1 reach
// every thread through LDS between two barriers, so the slice length, the
// stride k and the staging trip count are block-uniform; the per-row
// searches hold no barrier.  The wave == 0 / wave == 1 branches of step 1
// are wave-uniform and hold no barrier either.  The windowed bounds kernel
// has the same shape: its window reaches every thread through LDS between
// two barriers, so `fits` and the staging trip count are block-uniform.
//
// Bounds: lk loads in [0, nl), rk loads in [0, nr) (every probe index is
// below the search's current upper bound, itself <= nr; a window lies in
// [0, nr) and its LDS copy holds wn <= JOIN_WIN keys).  off, lo and cnt
// loads are at i0 <= i <= i1, both in [0, nl) by construction of the two
// searches, whatever off holds; li and ri stores at j < total.  All indices
// and offsets are 64-bit.
#pragma once

#include "common.h"

#define JOIN_BLOCK 256
#define JOIN_TILE 2048      // output rows per tile (8 per thread)
#define JOIN_LDS_ROWS 1024  // off entries staged per tile (8 KB)
#define JOIN_BTILE 1024     // left rows per tile of the windowed bounds pass
#define JOIN_WIN 2048       // right keys of a window staged in LDS (16 KB)

// one left key k in the ascending column a[0, n): first = the first index
// with a >= k, cnt = the number of entries equal to k
DEV void join_run(const u64* __restrict__ a, long n, u64 k, long& first,
                  long& cnt) {
  long lo = 0, hi = n;
  for (int step = 0; step < 64 && lo < hi; ++step) {
    long mid = lo + ((hi - lo) >> 1);
    if (a[mid] < k) lo = mid + 1;
    else hi = mid;
  }
  first = lo;
  // first index in [first, n) with a > k: probe first, first + 1,
  // first + 3, first + 7, ... until one is past the run, then bisect
  hi = n;
  long w = 1;
  for (int step = 0; step < 62; ++step) {
    long p = first + w - 1;
    if (p >= hi) break;
    if (a[p] <= k) lo = p + 1;
    else {
      hi = p;
      break;
    }
    w <<= 1;
  }
  for (int step = 0; step < 64 && lo < hi; ++step) {
    long mid = lo + ((hi - lo) >> 1);
    if (a[mid] <= k) lo = mid + 1;
    else hi = mid;
  }
  cnt = lo - first;
}

__global__ __launch_bounds__(JOIN_BLOCK) void join_bounds_kernel(
    const u64* __restrict__ lk, long nl, const u64* __restrict__ rk, long nr,
    i64* __restrict__ lo_out, i64* __restrict__ cnt_out) {
  const long stride = (long)gridDim.x * JOIN_BLOCK;
  for (long i = (long)blockIdx.x * JOIN_BLOCK + threadIdx.x; i < nl;
       i += stride) {
    long first, cnt;
    join_run(rk, nr, lk[i], first, cnt);
    lo_out[i] = first;
    cnt_out[i] = cnt;
  }
}

__global__ __launch_bounds__(JOIN_BLOCK) void join_bounds_window_kernel(
    const u64* __restrict__ lk, long nl, const u64* __restrict__ rk, long nr,
    long ntiles, i64* __restrict__ lo_out, i64* __restrict__ cnt_out) {
  __shared__ u64 s_rk[JOIN_WIN];
  __shared__ long s_w[2];

  const int tid = threadIdx.x;
  const int wave = tid / WAVE;

  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long t0 = tile * JOIN_BTILE;
    const long t1 = t0 + JOIN_BTILE < nl ? t0 + JOIN_BTILE : nl;

    // the window [first rk >= the tile's first key, first rk > its last)
    if (wave == 0) {
      const u64 k = lk[t0];
      long lo = 0, hi = nr;
      for (int step = 0; step < 64 && lo < hi; ++step) {
        long mid = lo + ((hi - lo) >> 1);
        if (rk[mid] < k) lo = mid + 1;
        else hi = mid;
      }
      if (tid == 0) s_w[0] = lo;
    } else if (wave == 1) {
      const u64 k = lk[t1 - 1];
      long lo = 0, hi = nr;
      for (int step = 0; step < 64 && lo < hi; ++step) {
        long mid = lo + ((hi - lo) >> 1);
        if (rk[mid] <= k) lo = mid + 1;
        else hi = mid;
      }
      if (tid == WAVE) s_w[1] = lo;
    }
    __syncthreads();
    const long wlo = s_w[0];
    const long wn = s_w[1] > wlo ? s_w[1] - wlo : 0;
    const bool fits = wn <= JOIN_WIN;  // block-uniform
    if (fits)
      for (int s = tid; s < (int)wn; s += JOIN_BLOCK) s_rk[s] = rk[wlo + s];
    __syncthreads();

    for (long i = t0 + tid; i < t1; i += JOIN_BLOCK) {
      long first, cnt;
      if (fits) join_run(s_rk, wn, lk[i], first, cnt);
      else join_run(rk + wlo, wn, lk[i], first, cnt);
      lo_out[i] = wlo + first;
      cnt_out[i] = cnt;
    }
    __syncthreads();  // s_rk and s_w are rewritten by the next tile
  }
}

// last index i in [0, n) with a[i] <= v, given a[0] <= v (n >= 1)
DEV long join_last_le(const i64* __restrict__ a, long n, long v) {
  long lo = 1, hi = n;  // first index in [1, n) with a[i] > v
  for (int step = 0; step < 64 && lo < hi; ++step) {
    long mid = lo + ((hi - lo) >> 1);
    if (a[mid] <= v) lo = mid + 1;
    else hi = mid;
  }
  return lo - 1;
}

__global__ __launch_bounds__(JOIN_BLOCK) void join_expand_kernel(
    const i64* __restrict__ off, long nl, const i64* __restrict__ lo,
    const i64* __restrict__ cnt, long total, long ntiles,
    i64* __restrict__ li, i64* __restrict__ ri) {
  __shared__ i64 s_off[JOIN_LDS_ROWS];
  __shared__ long s_i[2];

  const int tid = threadIdx.x;
  const int wave = tid / WAVE;

  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long ts = tile * JOIN_TILE;
    const long te = ts + JOIN_TILE < total ? ts + JOIN_TILE : total;

    // 1. the left rows covering [ts, te): off[0] == 0 <= ts
    if (wave == 0) {
      long i = join_last_le(off, nl, ts);
      if (tid == 0) s_i[0] = i;
    } else if (wave == 1) {
      long i = join_last_le(off, nl, te - 1);
      if (tid == WAVE) s_i[1] = i;
    }
    __syncthreads();
    const long i0 = s_i[0];
    const long i1 = s_i[1] > i0 ? s_i[1] : i0;

    // 2. stage off[i0 + s * k], s < m <= JOIN_LDS_ROWS
    const long n = i1 - i0 + 1;
    const long k = (n + JOIN_LDS_ROWS - 1) / JOIN_LDS_ROWS;
    const int m = (int)((n + k - 1) / k);
    for (int s = tid; s < m; s += JOIN_BLOCK) s_off[s] = off[i0 + s * k];
    __syncthreads();

    // 3. resolve and store
    for (long j = ts + tid; j < te; j += JOIN_BLOCK) {
      int a = 1, b = m;  // first s in [1, m) with s_off[s] > j
      for (int step = 0; step < 32 && a < b; ++step) {
        int mid = a + ((b - a) >> 1);
        if (s_off[mid] <= j) a = mid + 1;
        else b = mid;
      }
      const int s = a - 1;
      long i = i0 + s * k;
      i64 o = s_off[s];
      if (k > 1) {
        // the slice did not fit: finish among the k rows behind sample s
        long hi = i + k - 1 < i1 ? i + k - 1 : i1;
        i += join_last_le(off + i, hi - i + 1, j);
        o = off[i];
      }
      li[j] = i;
      ri[j] = cnt[i] > 0 ? lo[i] + (j - o) : -1;
    }
    __syncthreads();  // s_off and s_i are rewritten by the next tile
  }
}
