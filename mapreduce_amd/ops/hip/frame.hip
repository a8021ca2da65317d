// Per-key rolling aggregates: every row i of a relation sorted ascending on
// (key, order key of the time) gets a frame [lo[i], hi[i]) of rows of its
// own key with lo[i] <= i < hi[i], and the sum, min or max of a value column
// over that frame.
//
// Frame bounds (i64 times).  With T = group_okey(t_i), the frame of row i is
// every row j of its key with sat(T - preceding) <= okey(t_j) <=
// sat(T + following); the two ends are u64 and saturate at 0 and 2^64 - 1
// (the arithmetic of seg_session_flags_kernel: no span can overflow).  In
// the notation of asof.hip, over the relation itself,
//   lo = P(k, sat(T - preceding)),  hi = Q(k, sat(T + following)),
// both non-decreasing along the rows.  Two kernels give the same output:
//   frame_bounds_row_kernel     thread per row: each end is bracketed by an
//       exponential search outward from i (row i itself is inside its
//       frame, so i is a perfect hint and a frame of m rows costs about
//       2 log2(m) probes next to i), then asof_bound inside the bracket;
//   frame_bounds_window_kernel  the shape of asof_window_kernel: a block
//       owns tiles of FRAME_TILE rows [t0, t1) (capped grid, stride over
//       tiles).  The relation is joined with itself, so every frame of the
//       tile lies in the window [lo(t0), hi(t1 - 1)): wave 0 finds lo(t0)
//       with asof_bound_wave over the rows [0, t0), wave 1 finds hi(t1 - 1)
//       over the rows [t1, n).  A window of at most FRAME_WIN rows is staged
//       in LDS as keys and order keys and both ends of every row are
//       searched there, the lower one in [wlo, i], the upper one in
//       (i, whi); a longer window is searched in global memory, over the
//       window alone.
//
// Frame reduce.  Values travel as 64-bit patterns and combine by seg_op of
// seg_scan.hip (i64 sums wrap; f64 sums are IEEE; min / max compare order
// keys and keep the EARLIER operand among equal ones), always with the
// earlier rows as the first operand, so min / max return the stored bits of
// the earliest winning row of the frame.  Only disjoint pieces that lie
// inside the frame are combined, never a difference of running totals: a
// f64 sum errs by its own frame's sum |v| alone and a NaN or an inf reaches
// exactly the frames that hold it.  Three kernels over tiles of FRAME_RTILE
// rows, ordered by their launch boundaries alone:
//   frame_tile_kernel   one block per tile: pre[i] = the aggregate of the
//       rows from the tile's first row to i, suf[i] = of the rows from i to
//       the tile's last row, and the tile's own aggregate.  Wave w owns rows
//       [512 w, 512 (w + 1)) in 8 rounds of 64 (seg_wave_incl_scan by
//       __shfl_up for pre; its mirror image by __shfl_down for suf, which
//       still combines in row order); the four wave aggregates cross once
//       through LDS.  A row at or beyond n is an empty SegAgg.
//   frame_tree_kernel   ONE block: the aligned binary tree over the tile
//       aggregates.  Level 0 is the ntiles aggregates; node t of level l
//       covers tiles [t 2^l, (t + 1) 2^l) and level l holds only the
//       ntiles >> l nodes whose span ends inside the column; the levels lie
//       one behind the other (frame_tree_size entries, < 2 ntiles).  A
//       query reads a node only when its whole span lies inside the frame,
//       so a node over the end of the column is never needed and min / max
//       need no identity value.
//   frame_apply_kernel  one block per tile of output rows.  It stages the
//       tile's values in LDS and builds the same kind of tree over them in
//       LDS: 2048 leaves + 2047 nodes in 32 KB, so five blocks (20 waves)
//       share a CU's 160 KiB.  Row i, with tl = lo / R and th = (hi - 1) / R:
//       tl == th   (then both are the block's tile, as lo <= i < hi) a
//                  bottom-up query of the LDS tree over disjoint aligned
//                  nodes: left pieces are appended to a left accumulator in
//                  row order, right pieces put in front of a right one, the
//                  two joined at the end;
//       otherwise  suf[lo], then the whole tiles tl + 1 .. th - 1 by the
//                  same query on the global tree, then pre[hi - 1].
//       The f64 sum of a frame therefore associates as (left pieces in
//       order) + (right pieces in order).
//
// Control flow: every __syncthreads() is in block-uniform flow.  The tile
// loop of the window kernel runs on blockIdx.x, gridDim.x and ntiles; wlo
// and whi reach every thread through LDS between two barriers (the first
// two slots of the staging array, as in asof_window_kernel), so `fits` and
// the staging trip count are block-uniform; the wave == 0 / wave == 1
// branches are wave-uniform, hold no barrier and keep all 64 lanes active
// for the ballot of asof_bound_wave.  The shuffles and the one barrier of
// frame_tile_kernel sit outside the i < n guards.  frame_tree_kernel's
// level loop runs on ntiles, a kernel argument, one barrier per level.  The
// LDS tree of frame_apply_kernel is built by loops on compile-time counts
// with one barrier per level; the per-row queries behind it hold none.
// Every search and query loop has a constant trip bound.
//
// Bounds: keys and times are loaded at i, t0, t1 - 1 (all < n) and at probe
// indices inside the searched range: [0, i] and (i, n) in the row kernel
// (the gallop checks 0 <= i - step and i + step < n before it loads),
// [0, t0) and [t1, n) for the window's ends, [0, wn) over the base wlo with
// wlo <= t0 and wlo + wn = whi <= n inside the window; the LDS copies hold
// wn <= FRAME_WIN rows.  None of this depends on the rows being sorted.
// frame_apply_kernel clamps lo to [0, i] and hi to [i + 1, n] before any
// load, so suf[lo] and pre[hi - 1] are inside the columns, the in-tile
// query stays in [0, FRAME_RTILE) of the block's tile whenever tl == th,
// and the tile query reads nodes of [tl + 1, th) with th <= ntiles - 1,
// each below its level's count ntiles >> l.  pre, suf and out are stored at
// i < n, the tile aggregates at blockIdx.x < ntiles (the host launches
// exactly ntiles blocks).  All indices are 64-bit; fewer than 2^31 rows.
#pragma once

#include "asof.hip"
#include "common.h"
#include "group.hip"
#include "seg_scan.hip"

#define FRAME_BLOCK 256
#define FRAME_TILE 1024   // rows per tile of the window bounds kernel
#define FRAME_WIN 2048    // rows of a window staged in LDS (32 KB)
#define FRAME_ITEMS 8
#define FRAME_RTILE (FRAME_BLOCK * FRAME_ITEMS)  // rows per reduce tile
#define FRAME_WAVES (FRAME_BLOCK / WAVE)

// the two ends of row i's range frame as order keys
DEV void frame_ends(u64 t, u64 pre, u64 fol, u64& tlo, u64& thi) {
  const u64 ot = group_okey(t, false);
  tlo = ot >= pre ? ot - pre : 0;
  thi = ot + fol;
  if (thi < ot) thi = ~(u64)0;
}

// is row j below (k, ot), or at or below it when upper is set?
DEV bool frame_below(const u64* keys, const u64* times, long j, u64 k, u64 ot,
                     bool upper) {
  const u64 mk = keys[j];
  if (mk != k) return mk < k;
  const u64 mt = group_okey(times[j], false);
  return upper ? mt <= ot : mt < ot;
}

__global__ __launch_bounds__(FRAME_BLOCK) void frame_bounds_row_kernel(
    const u64* __restrict__ keys, const u64* __restrict__ times, long n,
    u64 pre, u64 fol, i64* __restrict__ lo, i64* __restrict__ hi) {
  const long stride = (long)gridDim.x * FRAME_BLOCK;
  for (long i = (long)blockIdx.x * FRAME_BLOCK + threadIdx.x; i < n;
       i += stride) {
    const u64 k = keys[i];
    u64 tlo, thi;
    frame_ends(times[i], pre, fol, tlo, thi);
    // row b is not below (k, tlo); row b - step is, or does not exist
    long b = i, step = 1;
    for (int s = 0; s < 64 && b - step >= 0 &&
                    !frame_below(keys, times, b - step, k, tlo, false);
         ++s) {
      b -= step;
      step <<= 1;
    }
    lo[i] = asof_bound<false>(keys, times, b - step >= 0 ? b - step + 1 : 0,
                              b, k, tlo, false, false);
    // row a is at or below (k, thi); row a + step is not, or does not exist
    long a = i;
    step = 1;
    for (int s = 0; s < 64 && a + step < n &&
                    frame_below(keys, times, a + step, k, thi, true);
         ++s) {
      a += step;
      step <<= 1;
    }
    hi[i] = asof_bound<false>(keys, times, a + 1,
                              a + step < n ? a + step : n, k, thi, true,
                              false);
  }
}

__global__ __launch_bounds__(FRAME_BLOCK) void frame_bounds_window_kernel(
    const u64* __restrict__ keys, const u64* __restrict__ times, long n,
    long ntiles, u64 pre, u64 fol, i64* __restrict__ lo,
    i64* __restrict__ hi) {
  // exactly 32 KB: the window's two bounds travel through s_t[0] and s_t[1]
  // before the staging loop overwrites them
  __shared__ u64 s_k[FRAME_WIN];
  __shared__ u64 s_t[FRAME_WIN];  // order keys of the window's times

  const int tid = threadIdx.x;
  const int wave = tid / WAVE;

  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long t0 = tile * FRAME_TILE;
    const long t1 = t0 + FRAME_TILE < n ? t0 + FRAME_TILE : n;

    if (wave == 0) {  // lo(t0), in [0, t0]
      u64 tlo, thi;
      frame_ends(times[t0], pre, fol, tlo, thi);
      const long p =
          asof_bound_wave(keys, times, t0, keys[t0], tlo, false, false);
      if (tid == 0) s_t[0] = (u64)p;
    } else if (wave == 1) {  // hi(t1 - 1), in [t1, n]
      u64 tlo, thi;
      frame_ends(times[t1 - 1], pre, fol, tlo, thi);
      const long q = asof_bound_wave(keys + t1, times + t1, n - t1,
                                     keys[t1 - 1], thi, true, false);
      if (tid == WAVE) s_t[1] = (u64)(t1 + q);
    }
    __syncthreads();
    const long wlo = (long)s_t[0];
    const long whi = (long)s_t[1];
    const long wn = whi - wlo;         // >= t1 - t0 >= 1
    const bool fits = wn <= FRAME_WIN;  // block-uniform
    __syncthreads();  // every thread holds the bounds: s_t may be staged
    if (fits)
      for (int s = tid; s < (int)wn; s += FRAME_BLOCK) {
        s_k[s] = keys[wlo + s];
        s_t[s] = group_okey(times[wlo + s], false);
      }
    __syncthreads();

    for (long i = t0 + tid; i < t1; i += FRAME_BLOCK) {
      const u64 k = keys[i];
      u64 tlo, thi;
      frame_ends(times[i], pre, fol, tlo, thi);
      const long w = i - wlo;  // row i in the window: lo <= w < hi
      long l, h;
      if (fits) {
        l = asof_bound<true>(s_k, s_t, 0, w, k, tlo, false, false);
        h = asof_bound<true>(s_k, s_t, w + 1, wn, k, thi, true, false);
      } else {
        l = asof_bound<false>(keys + wlo, times + wlo, 0, w, k, tlo, false,
                              false);
        h = asof_bound<false>(keys + wlo, times + wlo, w + 1, wn, k, thi,
                              true, false);
      }
      lo[i] = wlo + l;
      hi[i] = wlo + h;
    }
    __syncthreads();  // s_k and s_t are rewritten by the next tile
  }
}

// ------------------------------------------------------------ frame reduce

// entries of the tree over ntiles tile aggregates: ntiles >> l on level l
inline long frame_tree_size(long ntiles) {
  long total = 0;
  for (long c = ntiles; c >= 1; c >>= 1) total += c;
  return total;
}

// every lane of the wave calls this: x = the aggregate of lanes lane..63
template <int OP, bool F64>
DEV SegAgg frame_wave_suffix_scan(SegAgg x, int lane) {
  for (int off = 1; off < WAVE; off <<= 1) {
    SegAgg o;
    o.f = __shfl_down(x.f, off, WAVE);
    o.a = __shfl_down(x.a, off, WAVE);
    if (lane + off < WAVE) x = seg_combine<OP, F64>(x, o);
  }
  return x;
}

template <int OP, bool F64>
__global__ __launch_bounds__(FRAME_BLOCK) void frame_tile_kernel(
    const u64* __restrict__ vals, long n, u64* __restrict__ pre,
    u64* __restrict__ suf, u64* __restrict__ tiles) {
  __shared__ u32 s_f[FRAME_WAVES];
  __shared__ u64 s_a[FRAME_WAVES];
  const int tid = threadIdx.x, wave = tid / WAVE, lane = tid % WAVE;
  const long tile = blockIdx.x;
  const long w0 = tile * FRAME_RTILE + (long)wave * (WAVE * FRAME_ITEMS);
  SegAgg r[FRAME_ITEMS], p[FRAME_ITEMS];
#pragma unroll
  for (int j = 0; j < FRAME_ITEMS; ++j) {
    const long i = w0 + j * WAVE + lane;
    r[j].f = 0;
    r[j].a = 0;
    if (i < n) {
      r[j].f = SEG_FULL;
      r[j].a = vals[i];
    }
  }
  SegAgg run;  // of the wave's earlier rounds, then of the whole wave
  run.f = 0;
  run.a = 0;
#pragma unroll
  for (int j = 0; j < FRAME_ITEMS; ++j) {
    SegAgg x = seg_wave_incl_scan<OP, F64>(r[j], lane);
    x = seg_combine<OP, F64>(run, x);
    p[j] = x;
    run.f = __shfl(x.f, WAVE - 1, WAVE);
    run.a = __shfl(x.a, WAVE - 1, WAVE);
  }
  if (lane == 0) {
    s_f[wave] = run.f;
    s_a[wave] = run.a;
  }
  __syncthreads();
  SegAgg before, after, all;  // the earlier waves, the later ones, the tile
  before.f = after.f = all.f = 0;
  before.a = after.a = all.a = 0;
  for (int u = 0; u < FRAME_WAVES; ++u) {
    SegAgg o;
    o.f = s_f[u];
    o.a = s_a[u];
    if (u < wave) before = seg_combine<OP, F64>(before, o);
    if (u > wave) after = seg_combine<OP, F64>(after, o);
    all = seg_combine<OP, F64>(all, o);
  }
#pragma unroll
  for (int j = 0; j < FRAME_ITEMS; ++j) {
    const long i = w0 + j * WAVE + lane;
    if (i < n) pre[i] = seg_combine<OP, F64>(before, p[j]).a;
  }
  run.f = 0;  // of the wave's later rounds
  run.a = 0;
#pragma unroll
  for (int j = FRAME_ITEMS - 1; j >= 0; --j) {
    SegAgg x = frame_wave_suffix_scan<OP, F64>(r[j], lane);
    x = seg_combine<OP, F64>(x, run);
    run.f = __shfl(x.f, 0, WAVE);
    run.a = __shfl(x.a, 0, WAVE);
    const long i = w0 + j * WAVE + lane;
    if (i < n) suf[i] = seg_combine<OP, F64>(x, after).a;
  }
  if (tid == 0) tiles[tile] = all.a;  // the tile holds row tile * R < n
}

// one block; tree level 0 = tiles, level l node t = node 2t, then node
// 2t + 1, of level l - 1
template <int OP, bool F64>
__global__ __launch_bounds__(FRAME_BLOCK) void frame_tree_kernel(
    const u64* __restrict__ tiles, long ntiles, u64* tree) {
  for (long t = threadIdx.x; t < ntiles; t += FRAME_BLOCK) tree[t] = tiles[t];
  __syncthreads();
  long off = 0;  // of the level below
  for (long cnt = ntiles; cnt >= 2; cnt >>= 1) {  // block-uniform
    const long up = off + cnt;
    for (long t = threadIdx.x; t < (cnt >> 1); t += FRAME_BLOCK)
      tree[up + t] =
          seg_op<OP, F64>(tree[off + 2 * t], tree[off + 2 * t + 1]);
    off = up;
    __syncthreads();
  }
}

// The aggregate of leaves [a, b), a < b, of an aligned tree whose level 0
// holds cnt leaves at node[0] and whose further levels (cnt >> l nodes)
// follow one another.  first / last, when given, are pieces in front of and
// behind the leaves.  Only nodes inside [a, b) are read.
template <int OP, bool F64, bool ENDS, typename PTR>
DEV u64 frame_query(PTR node, long cnt, long a, long b, u64 first, u64 last) {
  u64 left = first, right = last;
  bool hl = ENDS, hr = ENDS;
  long off = 0;
  for (int s = 0; s < 32 && a < b; ++s) {
    if (a & 1) {
      const u64 x = node[off + a];
      left = hl ? seg_op<OP, F64>(left, x) : x;
      hl = true;
      ++a;
    }
    if (b & 1) {
      --b;
      const u64 x = node[off + b];
      right = hr ? seg_op<OP, F64>(x, right) : x;
      hr = true;
    }
    a >>= 1;
    b >>= 1;
    off += cnt;
    cnt >>= 1;
  }
  if (hl && hr) return seg_op<OP, F64>(left, right);
  return hl ? left : right;
}

template <int OP, bool F64>
__global__ __launch_bounds__(FRAME_BLOCK) void frame_apply_kernel(
    const u64* __restrict__ vals, const i64* __restrict__ lo,
    const i64* __restrict__ hi, long n, const u64* __restrict__ pre,
    const u64* __restrict__ suf, const u64* __restrict__ tree, long ntiles,
    u64* __restrict__ out) {
  __shared__ u64 s_tree[2 * FRAME_RTILE];  // 4095 used: 32 KB, 5 blocks/CU
  const int tid = threadIdx.x;
  const long tile = blockIdx.x;
  const long base = tile * FRAME_RTILE;
  for (int s = tid; s < FRAME_RTILE; s += FRAME_BLOCK)
    s_tree[s] = base + s < n ? vals[base + s] : 0;
  __syncthreads();
  int off = 0;  // of the level below
  for (int cnt = FRAME_RTILE; cnt >= 2; cnt >>= 1) {
    const int up = off + cnt;
    for (int s = tid; s < (cnt >> 1); s += FRAME_BLOCK)
      s_tree[up + s] =
          seg_op<OP, F64>(s_tree[off + 2 * s], s_tree[off + 2 * s + 1]);
    off = up;
    __syncthreads();
  }
#pragma unroll 1
  for (int j = 0; j < FRAME_ITEMS; ++j) {
    const long i = base + j * FRAME_BLOCK + tid;
    if (i >= n) continue;
    long l = lo[i], h = hi[i];
    l = l < 0 ? 0 : (l > i ? i : l);
    h = h < i + 1 ? i + 1 : (h > n ? n : h);
    const long tl = l / FRAME_RTILE, th = (h - 1) / FRAME_RTILE;
    if (tl == th)
      out[i] = frame_query<OP, F64, false>(s_tree, (long)FRAME_RTILE,
                                           l - base, h - base, 0, 0);
    else
      out[i] = frame_query<OP, F64, true>(tree, ntiles, tl + 1, th, suf[l],
                                          pre[h - 1]);
  }
}
