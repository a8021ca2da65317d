// Per-key running aggregates over grouped rows: an inclusive segmented scan
// (sum, min, max) of an i64 or f64 value column, and the session flags of a
// time column.  K4/K5 for reducers whose answer is as long as their input.
//
// Segments.  A row is a segment head when it is row 0 or its key differs
// from the previous row's: keys need only be grouped, not sorted.
//
// Values travel as 64-bit patterns.  sum adds them as i64 (wrapping) or as
// f64 (IEEE, in the association described below); min and max compare the
// order keys of group.hip (group_okey: -0.0 equals +0.0, every NaN above
// +inf) and keep the stored bits of the earlier row among equal order keys.
//
// The scanned element is a SegAgg (f, a): a = the aggregate of the rows
// behind the last head of a run of rows (of the whole run when it holds no
// head), f bit 0 = the run holds a head, f bit 1 = the run is not empty.
// (0, 0) is the identity; seg_combine is associative, not commutative, and
// every use below combines runs in row order.
//
// Reduce-then-scan over tiles of SEG_SCAN_TILE rows, three kernels ordered
// by their launch boundaries alone; no block ever waits on another:
//   seg_scan_reduce_kernel  one block per tile -> the tile's SegAgg;
//   seg_scan_carry_kernel   ONE block: the exclusive scan of the tiles'
//                           SegAggs, SEG_CARRY_CHUNK tiles per loop trip
//                           with the running SegAgg kept in registers;
//   seg_scan_apply_kernel   one block per tile: scans its rows again and
//                           combines the tile's carry in front, which
//                           seg_combine drops behind the tile's first head.
// Inside a tile wave w owns rows [512 w, 512 (w + 1)) and takes them in 8
// rounds of 64 consecutive rows (coalesced loads and stores): an inclusive
// wave64 scan by __shfl_up, then the wave's running SegAgg of the earlier
// rounds in front, then lane 63's result broadcast as the new running one.
// The four wave aggregates cross once through LDS.  The f64 sum therefore
// associates as (carry + earlier waves) + ((earlier rounds) + tree over the
// lanes of a round).
//
// Control flow: the shuffles and the one barrier of the tile kernels are in
// block-uniform flow (only loads and stores sit behind the i < n guards; a
// row at or beyond n is the identity).  The carry kernel's loop runs on
// ntiles, a kernel argument, with its two barriers per trip.
//
// Bounds: keys and vals are loaded at i and i - 1 with 0 <= i - 1, i < n;
// out is stored at i < n; the tile arrays are indexed by blockIdx.x <
// ntiles (the host launches exactly ntiles blocks and sizes the arrays to
// ntiles) and by c0 + 4 tid + q < ntiles in the carry kernel; LDS is
// indexed by the wave number, < SEG_SCAN_WAVES.
//
// seg_session_flags_kernel: 1 where a row starts a key or its time exceeds
// the previous row's by more than gap; the difference is that of the two
// i64 order keys in u64 arithmetic, which cannot overflow.  Loads at i and
// i - 1 as above.
#pragma once

#include "common.h"
#include "group.hip"

#define SEG_SCAN_BLOCK 256
#define SEG_SCAN_ITEMS 8
#define SEG_SCAN_TILE (SEG_SCAN_BLOCK * SEG_SCAN_ITEMS)  // rows per tile
#define SEG_SCAN_WAVES (SEG_SCAN_BLOCK / WAVE)
#define SEG_CARRY_ITEMS 4
#define SEG_CARRY_CHUNK (SEG_SCAN_BLOCK * SEG_CARRY_ITEMS)  // tiles per trip

#define SEG_SUM 0
#define SEG_MIN 1
#define SEG_MAX 2

#define SEG_HEAD 1u
#define SEG_FULL 2u

struct SegAgg {
  u32 f;
  u64 a;
};

// a is the earlier operand
template <int OP, bool F64>
DEV u64 seg_op(u64 a, u64 b) {
  if (OP == SEG_SUM) {
    if (F64)
      return (u64)__double_as_longlong(__longlong_as_double((long long)a) +
                                       __longlong_as_double((long long)b));
    return a + b;
  }
  const u64 ka = group_okey(a, F64), kb = group_okey(b, F64);
  if (OP == SEG_MIN) return kb < ka ? b : a;
  return kb > ka ? b : a;
}

// x is the earlier run
template <int OP, bool F64>
DEV SegAgg seg_combine(SegAgg x, SegAgg y) {
  SegAgg r;
  r.f = x.f | y.f;
  const bool take_y = (y.f & SEG_HEAD) || !(x.f & SEG_FULL);
  r.a = !(y.f & SEG_FULL) ? x.a : (take_y ? y.a : seg_op<OP, F64>(x.a, y.a));
  return r;
}

// every lane of the wave calls this
template <int OP, bool F64>
DEV SegAgg seg_wave_incl_scan(SegAgg x, int lane) {
  for (int off = 1; off < WAVE; off <<= 1) {
    SegAgg o;
    o.f = __shfl_up(x.f, off, WAVE);
    o.a = __shfl_up(x.a, off, WAVE);
    if (lane >= off) x = seg_combine<OP, F64>(o, x);
  }
  return x;
}

// The wave's 512 rows from row w0 on: r[j] = the inclusive scan, inside the
// wave, at row w0 + 64 j + lane; returns the wave's aggregate in every lane.
template <int OP, bool F64>
DEV SegAgg seg_wave_rows(const u64* __restrict__ keys,
                         const u64* __restrict__ vals, long n, long w0,
                         int lane, SegAgg (&r)[SEG_SCAN_ITEMS]) {
#pragma unroll
  for (int j = 0; j < SEG_SCAN_ITEMS; ++j) {
    const long i = w0 + j * WAVE + lane;
    r[j].f = 0;
    r[j].a = 0;
    if (i < n) {
      const bool head = i == 0 || keys[i - 1] != keys[i];
      r[j].f = SEG_FULL | (head ? SEG_HEAD : 0u);
      r[j].a = vals[i];
    }
  }
  SegAgg run;
  run.f = 0;
  run.a = 0;
#pragma unroll
  for (int j = 0; j < SEG_SCAN_ITEMS; ++j) {
    SegAgg x = seg_wave_incl_scan<OP, F64>(r[j], lane);
    x = seg_combine<OP, F64>(run, x);
    r[j] = x;
    run.f = __shfl(x.f, WAVE - 1, WAVE);
    run.a = __shfl(x.a, WAVE - 1, WAVE);
  }
  return run;
}

template <int OP, bool F64>
__global__ __launch_bounds__(SEG_SCAN_BLOCK) void seg_scan_reduce_kernel(
    const u64* __restrict__ keys, const u64* __restrict__ vals, long n,
    i64* __restrict__ tile_f, u64* __restrict__ tile_a) {
  __shared__ u32 s_f[SEG_SCAN_WAVES];
  __shared__ u64 s_a[SEG_SCAN_WAVES];
  const int tid = threadIdx.x, wave = tid / WAVE, lane = tid % WAVE;
  const long tile = blockIdx.x;
  SegAgg r[SEG_SCAN_ITEMS];
  const SegAgg w = seg_wave_rows<OP, F64>(
      keys, vals, n, tile * SEG_SCAN_TILE + (long)wave * (WAVE * SEG_SCAN_ITEMS),
      lane, r);
  if (lane == 0) {
    s_f[wave] = w.f;
    s_a[wave] = w.a;
  }
  __syncthreads();
  if (tid == 0) {
    SegAgg t;
    t.f = 0;
    t.a = 0;
    for (int u = 0; u < SEG_SCAN_WAVES; ++u) {
      SegAgg o;
      o.f = s_f[u];
      o.a = s_a[u];
      t = seg_combine<OP, F64>(t, o);
    }
    tile_f[tile] = (i64)t.f;
    tile_a[tile] = t.a;
  }
}

// one block: carry[t] = the SegAgg of tiles [0, t), the identity for t == 0
template <int OP, bool F64>
__global__ __launch_bounds__(SEG_SCAN_BLOCK) void seg_scan_carry_kernel(
    const i64* __restrict__ tile_f, const u64* __restrict__ tile_a,
    long ntiles, i64* __restrict__ carry_f, u64* __restrict__ carry_a) {
  __shared__ u32 s_f[SEG_SCAN_WAVES];
  __shared__ u64 s_a[SEG_SCAN_WAVES];
  const int tid = threadIdx.x, wave = tid / WAVE, lane = tid % WAVE;
  SegAgg run;  // of every tile before the chunk, the same in all threads
  run.f = 0;
  run.a = 0;
  for (long c0 = 0; c0 < ntiles; c0 += SEG_CARRY_CHUNK) {  // block-uniform
    const long b = c0 + (long)tid * SEG_CARRY_ITEMS;
    SegAgg x[SEG_CARRY_ITEMS];
    SegAgg t;
    t.f = 0;
    t.a = 0;
#pragma unroll
    for (int q = 0; q < SEG_CARRY_ITEMS; ++q) {
      x[q].f = 0;
      x[q].a = 0;
      if (b + q < ntiles) {
        x[q].f = (u32)tile_f[b + q];
        x[q].a = tile_a[b + q];
      }
      t = seg_combine<OP, F64>(t, x[q]);
    }
    const SegAgg inc = seg_wave_incl_scan<OP, F64>(t, lane);
    SegAgg ex;  // of the wave's earlier lanes
    ex.f = __shfl_up(inc.f, 1, WAVE);
    ex.a = __shfl_up(inc.a, 1, WAVE);
    if (lane == 0) {
      ex.f = 0;
      ex.a = 0;
    }
    if (lane == WAVE - 1) {
      s_f[wave] = inc.f;
      s_a[wave] = inc.a;
    }
    __syncthreads();
    SegAgg pre = run;
    for (int u = 0; u < SEG_SCAN_WAVES; ++u) {
      SegAgg o;
      o.f = s_f[u];
      o.a = s_a[u];
      if (u < wave) pre = seg_combine<OP, F64>(pre, o);
      run = seg_combine<OP, F64>(run, o);
    }
    pre = seg_combine<OP, F64>(pre, ex);
#pragma unroll
    for (int q = 0; q < SEG_CARRY_ITEMS; ++q) {
      if (b + q < ntiles) {
        carry_f[b + q] = (i64)pre.f;
        carry_a[b + q] = pre.a;
      }
      pre = seg_combine<OP, F64>(pre, x[q]);
    }
    __syncthreads();  // s_f, s_a are rewritten by the next trip
  }
}

template <int OP, bool F64>
__global__ __launch_bounds__(SEG_SCAN_BLOCK) void seg_scan_apply_kernel(
    const u64* __restrict__ keys, const u64* __restrict__ vals, long n,
    const i64* __restrict__ carry_f, const u64* __restrict__ carry_a,
    u64* __restrict__ out) {
  __shared__ u32 s_f[SEG_SCAN_WAVES];
  __shared__ u64 s_a[SEG_SCAN_WAVES];
  const int tid = threadIdx.x, wave = tid / WAVE, lane = tid % WAVE;
  const long tile = blockIdx.x;
  const long w0 =
      tile * SEG_SCAN_TILE + (long)wave * (WAVE * SEG_SCAN_ITEMS);
  SegAgg r[SEG_SCAN_ITEMS];
  const SegAgg w = seg_wave_rows<OP, F64>(keys, vals, n, w0, lane, r);
  if (lane == 0) {
    s_f[wave] = w.f;
    s_a[wave] = w.a;
  }
  __syncthreads();
  SegAgg pre;
  pre.f = (u32)carry_f[tile];
  pre.a = carry_a[tile];
  for (int u = 0; u < SEG_SCAN_WAVES; ++u) {
    SegAgg o;
    o.f = s_f[u];
    o.a = s_a[u];
    if (u < wave) pre = seg_combine<OP, F64>(pre, o);
  }
#pragma unroll
  for (int j = 0; j < SEG_SCAN_ITEMS; ++j) {
    const long i = w0 + j * WAVE + lane;
    if (i < n) out[i] = seg_combine<OP, F64>(pre, r[j]).a;
  }
}

__global__ __launch_bounds__(SEG_SCAN_BLOCK) void seg_session_flags_kernel(
    const u64* __restrict__ keys, const u64* __restrict__ times, long n,
    u64 gap, i64* __restrict__ flags) {
  const long stride = (long)gridDim.x * SEG_SCAN_BLOCK;
  for (long i = (long)blockIdx.x * SEG_SCAN_BLOCK + threadIdx.x; i < n;
       i += stride) {
    bool head = i == 0 || keys[i] != keys[i - 1];
    if (!head)
      head = group_okey(times[i], false) - group_okey(times[i - 1], false) >
             gap;
    flags[i] = head ? 1 : 0;
  }
}
