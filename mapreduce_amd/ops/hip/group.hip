// Per-key order statistics over rows sorted by key: the values of every key
// brought into order on the device, then picked from the ordered runs
// (quantiles, top-k, distinct counts).  K4/K5 for reducers that need the
// whole value list of a key.
//
// Order keys.  Values are i64 or f64 and travel as 64-bit patterns; their
// order is that of a u64 order key (group_okey):
//   i64: bits ^ (1 << 63);
//   f64: the sign-flip transform, after -0.0 took the bits of +0.0 and
//        every NaN took the one key above +inf (all ones).
// Values with the same order key are equal for every kernel here; the
// stored bits are never altered, only moved.
//
// group_tile_sort_kernel: a block owns one tile of GROUP_TILE consecutive
// rows.  It stages each row's order key (u64), a u32 of (tile-local segment
// number << 16 | row within the tile) and the first row of every local
// segment in LDS, then sorts by (local segment, order key, row).  The row is
// part of the sort key, so equal values keep their input order and the
// result is unique.  Two sorts:
//   rank counting, when no segment to finish is longer than GROUP_RANK_MAX:
//     a row's place inside its segment is the number of the segment's rows
//     ordered before it, len LDS reads per row and no barrier; the row's
//     value goes to out[t0 + start + rank];
//   a bitonic network over the whole tile otherwise (66 stages of one
//     barrier each; pairs (i, i | j) of a stage are disjoint and consecutive
//     lanes take consecutive pairs), then out[t0 + i] = vals[t0 + row of
//     the i-th element].
// Every segment that lies wholly inside the tile is finished; a segment that
// crosses a tile boundary is not (the host re-sorts those rows and
// overwrites their slots; the rank pass does not write them at all).  A
// tile that lies wholly inside one such segment is skipped.  The PERM
// instantiation also stores the input row of every value it stores, at the
// same index and under the same guards.
//   LDS: 8 B + 4 B + 2 B per row = 28 KB at GROUP_TILE 2048, five blocks
//   per CU.
//
// group_pick_kernel: one thread per (segment, rank specification); the index
// inside a segment of length len is (num * (len - 1) + add) / den in u64
// arithmetic (num <= den <= 10^6 and len < 2^31: no overflow).
//
// group_distinct_flags_kernel: 1 where a row starts a segment or its order
// key differs from the previous row's.
//
// Control flow: the tile kernel's barriers are all in block-uniform flow.
// The early exit depends on seg[] at fixed addresses read by every thread;
// the choice between the two sorts is read from LDS behind a barrier; the
// stage loops run on compile-time bounds.
//
// Bounds: seg and vals loads at t0 + i < n (and t0 - 1 >= 0, t1 < n for the
// two neighbours); LDS indices are i, i | j < GROUP_TILE, and a local
// segment number is at most its row, so s_start is indexed at <= GROUP_TILE;
// the rank pass clamps a segment's bounds to [0, cnt) around the row, so its
// store lands inside the tile whatever seg holds; the network's output row
// is taken from the low 16 bits of an entry this block wrote itself and is
// checked against the tile's row count before it indexes vals.  The pick
// kernel checks every offset pair against [0, n] before it loads.
#pragma once

#include "common.h"

#define GROUP_BLOCK 256
#define GROUP_TILE 2048     // rows per tile (8 per thread), a power of two
#define GROUP_QMAX 8        // rank specifications per group_pick launch
#define GROUP_RANK_MAX 256  // longest segment the rank-counting pass takes
#define GROUP_PAD_SEG 0xFFFFu

DEV u64 group_okey(u64 bits, bool f64) {
  const u64 sign = 1ull << 63;
  if (!f64) return bits ^ sign;
  if ((bits << 1) == 0) bits = 0;  // -0.0 orders as +0.0
  if ((bits & ~sign) > 0x7FF0000000000000ull) return ~0ull;  // NaN
  return bits ^ ((bits & sign) ? ~0ull : sign);
}

__global__ __launch_bounds__(GROUP_BLOCK) void group_order_keys_kernel(
    const u64* __restrict__ vals, long n, int f64, u64* __restrict__ out) {
  const long stride = (long)gridDim.x * GROUP_BLOCK;
  for (long i = (long)blockIdx.x * GROUP_BLOCK + threadIdx.x; i < n;
       i += stride)
    out[i] = group_okey(vals[i], f64 != 0);
}

// (segment, order key, row) ascending; meta = segment << 16 | row
DEV bool group_less(u64 ka, u32 ma, u64 kb, u32 mb) {
  const u32 sa = ma >> 16, sb = mb >> 16;
  if (sa != sb) return sa < sb;
  if (ka != kb) return ka < kb;
  return ma < mb;
}

// PERM: also perm[output row] = the input row its value came from
template <bool PERM>
__global__ __launch_bounds__(GROUP_BLOCK) void group_tile_sort_kernel(
    const i64* __restrict__ seg, const u64* __restrict__ vals, long n,
    int f64, u64* __restrict__ out, i64* __restrict__ perm) {
  __shared__ u64 s_key[GROUP_TILE];
  __shared__ u32 s_meta[GROUP_TILE];
  __shared__ unsigned short s_start[GROUP_TILE + 1];
  __shared__ int s_long;

  const int tid = threadIdx.x;
  const long t0 = (long)blockIdx.x * GROUP_TILE;
  if (t0 >= n) return;  // block-uniform
  const long t1 = t0 + GROUP_TILE < n ? t0 + GROUP_TILE : n;
  const int cnt = (int)(t1 - t0);
  const i64 seg0 = seg[t0];
  const i64 seg1 = seg[t1 - 1];
  // the first / last segment of the tile reaches outside it: its rows are
  // the host's (block-uniform: fixed addresses)
  const bool open_lo = t0 > 0 && seg[t0 - 1] == seg0;
  const bool open_hi = t1 < n && seg[t1] == seg1;
  if (open_lo && open_hi && seg0 == seg1) return;  // nothing to finish here

  // local segment numbers are clamped to the row: a nondecreasing seg with
  // steps of at most 1 never reaches the clamp, and s_start stays in bounds
  // whatever seg holds
  const i64 d1 = seg1 - seg0;
  const u32 ls_last = d1 < 0 ? 0u : (d1 > cnt - 1 ? (u32)(cnt - 1) : (u32)d1);

  if (tid == 0) s_long = 0;
  for (int i = tid; i < GROUP_TILE; i += GROUP_BLOCK) {
    if (i < cnt) {
      const i64 sg = seg[t0 + i];
      const i64 d = sg - seg0;
      const u32 ls = d < 0 ? 0u : (d > i ? (u32)i : (u32)d);
      s_key[i] = group_okey(vals[t0 + i], f64 != 0);
      s_meta[i] = (ls << 16) | (u32)i;
      if (i == 0 || seg[t0 + i - 1] != sg) s_start[ls] = (unsigned short)i;
      if (i == cnt - 1) s_start[ls + 1] = (unsigned short)cnt;
    } else {
      s_key[i] = ~0ull;
      s_meta[i] = (GROUP_PAD_SEG << 16) | (u32)i;  // sorts behind every row
    }
  }
  __syncthreads();

  // a segment of the tile's own longer than GROUP_RANK_MAX: the network
  for (int i = tid; i < cnt; i += GROUP_BLOCK) {
    const u32 ls = s_meta[i] >> 16;
    if (s_start[ls] != i) continue;  // heads only
    const bool open = (ls == 0 && open_lo) || (ls == ls_last && open_hi);
    if (!open && (int)s_start[ls + 1] - i > GROUP_RANK_MAX)
      atomicOr(&s_long, 1);
  }
  __syncthreads();

  if (s_long == 0) {  // block-uniform
    // every segment to finish is short: the rank of a row inside its
    // segment is the number of rows ordered before it; lanes of one
    // segment read the same LDS address in the same step (broadcast)
    for (int i = tid; i < cnt; i += GROUP_BLOCK) {
      const u32 ls = s_meta[i] >> 16;
      if ((ls == 0 && open_lo) || (ls == ls_last && open_hi)) continue;
      int a = s_start[ls], b = s_start[ls + 1];
      a = a > i ? i : a;
      b = b <= i ? i + 1 : (b > cnt ? cnt : b);
      const u64 ki = s_key[i];
      int r = 0;
      for (int j = a; j < b; ++j) {
        const u64 kj = s_key[j];
        r += (kj < ki || (kj == ki && j < i)) ? 1 : 0;
      }
      out[t0 + a + r] = vals[t0 + i];  // r <= b - a - 1: inside the tile
      if (PERM) perm[t0 + a + r] = t0 + i;
    }
    return;
  }

  for (int k = 2; k <= GROUP_TILE; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int p = tid; p < GROUP_TILE / 2; p += GROUP_BLOCK) {
        const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
        const int l = i | j;
        const u64 ka = s_key[i], kb = s_key[l];
        const u32 ma = s_meta[i], mb = s_meta[l];
        const bool up = (i & k) == 0;
        if (group_less(kb, mb, ka, ma) == up) {
          s_key[i] = kb;
          s_key[l] = ka;
          s_meta[i] = mb;
          s_meta[l] = ma;
        }
      }
      __syncthreads();
    }
  }

  for (int i = tid; i < cnt; i += GROUP_BLOCK) {
    const int row = (int)(s_meta[i] & 0xFFFFu);
    if (row < cnt) {
      out[t0 + i] = vals[t0 + row];
      if (PERM) perm[t0 + i] = t0 + row;
    }
  }
}

struct GroupSpecs {
  u32 num[GROUP_QMAX];
  u32 den[GROUP_QMAX];
  u32 add[GROUP_QMAX];  // den - 1 under "higher", else 0
};

__global__ __launch_bounds__(GROUP_BLOCK) void group_pick_kernel(
    const i64* __restrict__ off, long nseg, const u64* __restrict__ vals,
    long n, GroupSpecs sp, int nq, u64* __restrict__ out) {
  const long total = nseg * nq;
  const long stride = (long)gridDim.x * GROUP_BLOCK;
  for (long t = (long)blockIdx.x * GROUP_BLOCK + threadIdx.x; t < total;
       t += stride) {
    const long s = t / nq;
    const int q = (int)(t - s * nq);
    const i64 a = off[s], b = off[s + 1];
    u64 v = 0;
    if (a >= 0 && b > a && b <= n) {
      const u64 len = (u64)(b - a);
      const u64 idx = ((u64)sp.num[q] * (len - 1) + sp.add[q]) / sp.den[q];
      if (idx < len) v = vals[a + (long)idx];
    }
    out[t] = v;
  }
}

__global__ __launch_bounds__(GROUP_BLOCK) void group_distinct_flags_kernel(
    const u64* __restrict__ keys, const u64* __restrict__ vals, long n,
    int f64, i64* __restrict__ flags) {
  const long stride = (long)gridDim.x * GROUP_BLOCK;
  for (long i = (long)blockIdx.x * GROUP_BLOCK + threadIdx.x; i < n;
       i += stride) {
    bool head = i == 0 || keys[i] != keys[i - 1];
    if (!head)
      head = group_okey(vals[i], f64 != 0) != group_okey(vals[i - 1], f64 != 0);
    flags[i] = head ? 1 : 0;
  }
}
