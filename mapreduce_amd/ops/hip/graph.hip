// Resident-graph propagation: for every destination row v of a CSR (offsets
// i64[n + 1] over m in-edges, src int32[m]) the sum, min or max of a value
// GATHERED through the edge, out[v] = op over e in [offsets[v], offsets[v+1])
// of x[src[e]].  K4/K5 for iterative reducers over keyed data (PageRank,
// connected components): the graph stays put and x changes per iteration.
//
// Balanced by edge.  The edges are cut into tiles of GRAPH_TILE = 256
// threads x 8 edges whatever the rows look like, so a hub of half the edges
// is spread over half the blocks and a run of empty rows costs nothing: no
// thread ever walks rows, only edges.  The host fills out with the identity
// before the first kernel, which is the whole answer for an empty row.
// Three kernels ordered by their launch boundaries alone; no block waits on
// another, there is no atomic and no spin loop:
//   graph_tile_kernel   one block per tile [e0, e1).
//       1. Stage.  Edge e0 + 256 j + tid (coalesced 4-byte loads of src, then
//          8 independent 8-byte gathers per thread in flight) is stored to
//          LDS at 256 j + tid; a src outside [0, n) is never dereferenced
//          and contributes the identity.  Meanwhile thread 0 finds the row
//          of e0 and thread 64 the row of e1 - 1 by bisection of offsets.
//       2. Walk.  Thread t owns the 8 CONSECUTIVE edges from a = e0 + 8 t.
//          It finds the row of a by bisection between the tile's two rows and
//          then steps: behind the last edge of a row it takes the next row
//          when that one is not empty and bisects again otherwise, so a run
//          of a million empty rows is one search of 20 probes.  Every edge
//          becomes a SegAgg of seg_scan.hip (head = first edge of its row).
//       3. Scan.  The threads' aggregates are scanned exclusively across the
//          block (wave scan by __shfl_up, the four wave aggregates through
//          LDS); each thread then replays its 8 edges behind its carry-in and,
//          at the LAST edge of a row, stores the row: to out when the row's
//          head lies in this tile, else as the tile's lead (row, partial),
//          since the row began in an earlier tile.  The tile's own aggregate
//          goes to (tile_f, tile_a).
//   seg_scan_carry_kernel (seg_scan.hip, ONE block): the exclusive segmented
//       scan of the tile aggregates: carry[t] = what the row open at the start
//       of tile t has gathered in the tiles before t, combined in tile order.
//   graph_lead_kernel   thread per tile: out[lead_row[t]] = carry[t] (+) lead[t].
// The association of a row's f64 sum is therefore a function of where its
// edges lie in the tiles, that is of (offsets, m) alone: 8 edges in order per
// thread, the shuffle tree over a wave's threads, the waves in order, the
// tiles by the carry scan.  x does not influence it, and two calls return
// the same bits.
//
// Control flow: every __syncthreads() and every shuffle of graph_tile_kernel
// is in block-uniform flow; only loads, stores and the searches sit behind
// guards, and the searches hold neither.  Every search has a constant trip
// bound and the edge loops run on compile-time counts.
//
// Bounds, none of which relies on offsets being monotone or src being in
// range.  src is loaded at e0 <= e < e1 <= m only.  x is loaded at s with
// 0 <= s < n (one unsigned compare).  graph_row_of returns a row in
// [lo, hi] for lo <= hi and loads offsets inside [lo, hi] only; its callers
// pass 0 <= lo <= hi <= n - 1, and the walk loads offsets[v], offsets[v + 1]
// and, where v + 1 <= hi, offsets[v + 2], so the largest index is n.  A row
// stored to out or to the lead is one of those v, so it is below n; the lead
// kernel checks 0 <= row < n again.  The tile arrays are indexed by
// blockIdx.x < ntiles (the host launches exactly ntiles blocks over arrays
// of ntiles entries) and by t < ntiles in the lead kernel.  LDS is indexed
// by 256 j + tid and 8 tid + k, both below GRAPH_TILE, and by the wave
// number.  Fewer than 2^31 edges and rows; indices are 64-bit.
//
// pagerank_update_kernel: one grid-stride pass over the nodes (see below).
#pragma once

#include "common.h"
#include "seg_scan.hip"

#define GRAPH_BLOCK 256
#define GRAPH_ITEMS 8
#define GRAPH_TILE (GRAPH_BLOCK * GRAPH_ITEMS)  // edges per tile
#define GRAPH_WAVES (GRAPH_BLOCK / WAVE)
#define GRAPH_PR_BLOCKS 1024  // most blocks (and partials) of the update pass

// the identity of OP as a 64-bit pattern: 0 (also +0.0), INT64_MAX, INT64_MIN
template <int OP>
DEV u64 graph_identity() {
  if (OP == SEG_SUM) return 0;
  if (OP == SEG_MIN) return 0x7FFFFFFFFFFFFFFFull;
  return 0x8000000000000000ull;
}

// the largest row v in [lo, hi] with offsets[v] <= e, or lo when there is
// none; lo <= hi.  With monotone offsets and offsets[lo] <= e this is the
// row that holds edge e, whatever empty rows lie around it.
DEV long graph_row_of(const i64* __restrict__ offsets, long e, long lo,
                      long hi) {
  for (int s = 0; s < 40 && lo < hi; ++s) {
    const long mid = lo + (hi - lo + 1) / 2;  // lo < mid <= hi
    if (offsets[mid] <= e) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

template <int OP, bool F64>
__global__ __launch_bounds__(GRAPH_BLOCK) void graph_tile_kernel(
    const i64* __restrict__ offsets, const int* __restrict__ src,
    const u64* __restrict__ x, long n, long m, u64* __restrict__ out,
    i64* __restrict__ tile_f, u64* __restrict__ tile_a,
    i64* __restrict__ lead_row, u64* __restrict__ lead_a) {
  __shared__ u64 s_val[GRAPH_TILE];
  __shared__ u32 s_f[GRAPH_WAVES];
  __shared__ u64 s_a[GRAPH_WAVES];
  __shared__ long s_rows[2];
  __shared__ long s_lead_row;
  __shared__ u64 s_lead_a;
  const int tid = threadIdx.x, wave = tid / WAVE, lane = tid % WAVE;
  const long tile = blockIdx.x;
  const long e0 = tile * GRAPH_TILE;
  const long e1 = e0 + GRAPH_TILE < m ? e0 + GRAPH_TILE : m;  // e0 < e1
  const u64 ident = graph_identity<OP>();

  // 1. stage the gathered values
  int s[GRAPH_ITEMS];
#pragma unroll
  for (int j = 0; j < GRAPH_ITEMS; ++j) {
    const long e = e0 + j * GRAPH_BLOCK + tid;
    s[j] = e < e1 ? src[e] : -1;
  }
#pragma unroll
  for (int j = 0; j < GRAPH_ITEMS; ++j) {
    u64 v = ident;
    if ((u64)(long)s[j] < (u64)n) v = x[s[j]];
    s_val[j * GRAPH_BLOCK + tid] = v;
  }
  if (tid == 0) {
    s_rows[0] = graph_row_of(offsets, e0, 0, n - 1);
    s_lead_row = -1;
    s_lead_a = 0;
  }
  if (tid == WAVE) s_rows[1] = graph_row_of(offsets, e1 - 1, 0, n - 1);
  __syncthreads();
  const long r_lo = s_rows[0];
  const long r_hi = s_rows[1] > r_lo ? s_rows[1] : r_lo;

  // 2. walk the thread's 8 consecutive edges
  const long a = e0 + (long)tid * GRAPH_ITEMS;
  SegAgg el[GRAPH_ITEMS];
  int vrow[GRAPH_ITEMS];
  u32 lastm = 0;
  long v = 0, rs = 0, re = 0;
  if (a < e1) {
    v = graph_row_of(offsets, a, r_lo, r_hi);
    rs = offsets[v];
    re = offsets[v + 1];
  }
  SegAgg t;
  t.f = 0;
  t.a = 0;
#pragma unroll
  for (int k = 0; k < GRAPH_ITEMS; ++k) {
    const long e = a + k;
    el[k].f = 0;
    el[k].a = 0;
    vrow[k] = 0;
    if (e < e1) {
      if (e >= re && v < r_hi) {  // behind the row: the next row with edges
        const long re2 = offsets[v + 2];
        if (re2 > e) {
          v = v + 1;
          rs = re;
          re = re2;
        } else {
          v = graph_row_of(offsets, e, v + 1, r_hi);
          rs = offsets[v];
          re = offsets[v + 1];
        }
      }
      el[k].f = SEG_FULL | (e == rs ? SEG_HEAD : 0u);
      el[k].a = s_val[tid * GRAPH_ITEMS + k];
      vrow[k] = (int)v;
      if (e + 1 == re) lastm |= 1u << k;
    }
    t = seg_combine<OP, F64>(t, el[k]);
  }

  // 3. the exclusive scan of the threads' aggregates across the block
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
  SegAgg run, whole;
  run.f = 0;
  run.a = 0;
  whole = run;
  for (int u = 0; u < GRAPH_WAVES; ++u) {
    SegAgg o;
    o.f = s_f[u];
    o.a = s_a[u];
    if (u < wave) run = seg_combine<OP, F64>(run, o);
    whole = seg_combine<OP, F64>(whole, o);
  }
  run = seg_combine<OP, F64>(run, ex);
#pragma unroll
  for (int k = 0; k < GRAPH_ITEMS; ++k) {
    run = seg_combine<OP, F64>(run, el[k]);
    if (lastm & (1u << k)) {
      if (run.f & SEG_HEAD) {
        out[vrow[k]] = run.a;
      } else {  // the row began in an earlier tile
        s_lead_row = vrow[k];
        s_lead_a = run.a;
      }
    }
  }
  __syncthreads();
  if (tid == 0) {
    tile_f[tile] = (i64)whole.f;
    tile_a[tile] = whole.a;
    lead_row[tile] = s_lead_row;
    lead_a[tile] = s_lead_a;
  }
}

template <int OP, bool F64>
__global__ __launch_bounds__(GRAPH_BLOCK) void graph_lead_kernel(
    const i64* __restrict__ lead_row, const u64* __restrict__ lead_a,
    const i64* __restrict__ carry_f, const u64* __restrict__ carry_a,
    long ntiles, long n, u64* __restrict__ out) {
  const long stride = (long)gridDim.x * GRAPH_BLOCK;
  for (long t = (long)blockIdx.x * GRAPH_BLOCK + threadIdx.x; t < ntiles;
       t += stride) {
    const long r = lead_row[t];
    if (r < 0 || r >= n) continue;
    SegAgg c, l;
    c.f = (u32)carry_f[t];
    c.a = carry_a[t];
    l.f = SEG_FULL;
    l.a = lead_a[t];
    out[r] = seg_combine<OP, F64>(c, l).a;
  }
}

// One PageRank update over the n nodes:
//   new[v]     = (1 - d) / n + d * (sums[v] + dangling / n)
//   contrib[v] = new[v] * inv_out[v]      (inv_out is 0 without out-edges)
// and per block two partials, partials[2 b] = sum |new - old| and
// partials[2 b + 1] = sum of new over the nodes with inv_out == 0, each over
// the block's nodes v = 256 b + tid + 256 gridDim.x i in a fixed order: a
// thread's nodes in order, the shuffle tree of the wave, the waves in order.
// The host sums the partials over b.  dangling is read from device memory,
// so iterations chain without a host sync.  All loads and stores at v < n,
// partials at blockIdx.x < gridDim.x (the host sizes it so).
__global__ __launch_bounds__(GRAPH_BLOCK) void pagerank_update_kernel(
    const double* __restrict__ sums, const double* __restrict__ old,
    const double* __restrict__ inv_out, long n, double damping,
    const double* __restrict__ dangling, double* __restrict__ nw,
    double* __restrict__ contrib, double* __restrict__ partials) {
  __shared__ double s_d[GRAPH_WAVES];
  __shared__ double s_g[GRAPH_WAVES];
  const int tid = threadIdx.x, wave = tid / WAVE, lane = tid % WAVE;
  const double base = (1.0 - damping) / (double)n;
  const double dn = dangling[0] / (double)n;
  double delta = 0.0, dang = 0.0;
  const long stride = (long)gridDim.x * GRAPH_BLOCK;
  for (long v = (long)blockIdx.x * GRAPH_BLOCK + tid; v < n; v += stride) {
    const double r = base + damping * (sums[v] + dn);
    const double io = inv_out[v];
    nw[v] = r;
    contrib[v] = r * io;
    delta += fabs(r - old[v]);
    if (io == 0.0) dang += r;
  }
  for (int off = WAVE / 2; off > 0; off >>= 1) {
    delta += __shfl_down(delta, off, WAVE);
    dang += __shfl_down(dang, off, WAVE);
  }
  if (lane == 0) {
    s_d[wave] = delta;
    s_g[wave] = dang;
  }
  __syncthreads();
  if (tid == 0) {
    double d = 0.0, g = 0.0;
    for (int u = 0; u < GRAPH_WAVES; ++u) {
      d += s_d[u];
      g += s_g[u];
    }
    partials[2 * blockIdx.x] = d;
    partials[2 * blockIdx.x + 1] = g;
  }
}
