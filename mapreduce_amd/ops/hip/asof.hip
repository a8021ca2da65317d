// As-of join of two relations, each sorted ascending on (key, order key of
// the time): every left row gets the index of ONE right row of its key, the
// latest at or before its time (backward), the earliest at or after it
// (forward) or the closer of the two (nearest), or -1.
//
// Order: keys are u64 bit patterns; times are ordered by group_okey (i64:
// bits ^ 2^63; f64: -0.0 equals +0.0, every NaN one value above +inf).  For
// a left row (k, t) over the right rows in that order,
//   P = the number of right rows <  (k, okey(t)),
//   Q = the number of right rows <= (k, okey(t)).
// The backward candidate is Q - 1 (P - 1 when exact matches are disallowed),
// the forward candidate P (Q when they are).  A candidate c is valid iff
// 0 <= c < nr, rk[c] == k and, with a tolerance, the u64 difference of the
// two order keys is <= tol (the arithmetic of seg_session_flags_kernel: it
// cannot overflow whatever the span).  Nearest takes the valid candidate
// with the smaller u64 distance, the backward one on a tie.
//
// Two kernels give the same output:
//   asof_row_kernel     thread per left row over the whole right side;
//   asof_window_kernel  a block owns tiles of ASOF_TILE left rows (capped
//       grid, stride over tiles).  The left side is sorted, so P and Q are
//       non-decreasing along a tile [t0, t1): wave 0 finds
//       wlo = max(P(row t0) - 1, 0), wave 1 finds
//       whi = min(Q(row t1 - 1) + 1, nr), each with a 64-way search over
//       the whole right side (asof_bound_wave: 4 dependent probes at 2^24
//       rows where one lane takes 24; every tile waits on the two), and
//       every candidate of every row of the tile lies in [wlo, whi).
//       Every right row below wlo is < the tile's first row and every one
//       from whi on is > its last, so P and Q searched inside the window
//       are the global ones minus wlo.  A window of at most ASOF_WIN rows
//       is staged in LDS, keys and ORDER KEYS of the times (computed once
//       per staged row, not per probe), and searched there; a longer one
//       is searched in global memory, but over the window alone.  The
//       window is bounded by the right rows between the tile's first and
//       last left row, so a hot key is spread over as many tiles as it has
//       left rows, not serialised.
//
// Control flow: every __syncthreads() is in block-uniform flow.  The tile
// loop runs on blockIdx.x, gridDim.x and ntiles alone; wlo and whi reach
// every thread through LDS between two barriers (in the first two slots of
// the staging array itself, which keeps the block at 32 KB), so `fits` and
// the staging trip count are block-uniform; the per-row searches hold no
// barrier.  The wave == 0 / wave == 1 branches are wave-uniform and hold no
// barrier; inside them all 64 lanes are active (the block is 4 full waves)
// and share lo and hi, so the ballot of asof_bound_wave sees the whole wave.
// dir, exact, has_tol and f64 are kernel arguments: uniform everywhere.
//
// Bounds: lk and lt loads at t0, t1 - 1 and i, all in [0, nl) (ntiles =
// ceil(nl / ASOF_TILE), so t0 < nl and t1 <= nl).  rk and rt loads: every
// probe index of a search is below the search's current upper bound, itself
// <= the searched length (nr, or wn over the window base wlo with
// wlo + wn <= nr); a candidate is loaded only after 0 <= c < that length
// was checked.  The LDS copies hold wn <= ASOF_WIN rows and are indexed
// below wn.  With nr == 0 no search probes and no candidate passes the
// range check, so rk and rt (null then) are never dereferenced.  ri stores
// at i < nl, consecutive lanes on consecutive i64.  All indices are 64-bit.
#pragma once

#include "common.h"
#include "group.hip"

#define ASOF_BLOCK 256
#define ASOF_TILE 1024  // left rows per tile (4 per thread)
#define ASOF_WIN 2048   // right rows of a window staged in LDS (32 KB)

#define ASOF_BACKWARD 0
#define ASOF_FORWARD 1
#define ASOF_NEAREST 2

// the order key of right row i: rt holds order keys already (the LDS copy)
// or the stored times
template <bool OKEYS>
DEV u64 asof_rot(const u64* rt, long i, bool f64) {
  return OKEYS ? rt[i] : group_okey(rt[i], f64);
}

// the number of rows of (rk, rt)[0, n) that are < (k, ot), or <= (k, ot)
// when upper is set; searched in [lo, n)
template <bool OKEYS>
DEV long asof_bound(const u64* rk, const u64* rt, long lo, long n, u64 k,
                    u64 ot, bool upper, bool f64) {
  long hi = n;
  for (int step = 0; step < 64 && lo < hi; ++step) {
    const long mid = lo + ((hi - lo) >> 1);
    const u64 mk = rk[mid];
    bool below = mk < k;
    if (mk == k) {
      const u64 mt = asof_rot<OKEYS>(rt, mid, f64);
      below = upper ? mt <= ot : mt < ot;
    }
    if (below) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// asof_bound over [0, n) by a whole wave, every lane with the same k and
// ot: each trip the 64 lanes probe 64 evenly spaced rows of [lo, hi) and the
// range shrinks to the gap that holds the bound, so it takes about
// log64(n) dependent loads where one lane takes log2(n).  Probes are at
// lo + floor(len * j / 64), j < 64, all in [lo, hi); when len <= 64 they
// cover every row and the trip ends the search.  Rows below the bound are a
// prefix, so their count c among the probes places it in (probe c - 1,
// probe c].  All 64 lanes must be active.  The loop is bounded: a trip
// leaves at most ceil(len / 64) rows, so 2^63 rows take 11 trips and the
// bound of 12 is never what ends a search.
DEV long asof_bound_wave(const u64* rk, const u64* rt, long n, u64 k, u64 ot,
                         bool upper, bool f64) {
  const long j = threadIdx.x % WAVE;
  long lo = 0, hi = n;
  for (int step = 0; step < 12 && lo < hi; ++step) {  // wave-uniform
    const long a = (hi - lo) / WAVE, b = (hi - lo) % WAVE;
    const long p = lo + a * j + b * j / WAVE;
    const u64 mk = rk[p];
    bool below = mk < k;
    if (mk == k) {
      const u64 mt = group_okey(rt[p], f64);
      below = upper ? mt <= ot : mt < ot;
    }
    const long c = __popcll(__ballot(below));
    if (c < WAVE) hi = lo + a * c + b * c / WAVE;
    if (c > 0) lo = lo + a * (c - 1) + b * (c - 1) / WAVE + 1;
  }
  return lo;
}

// is candidate c a row of key k within the tolerance?  dist = the u64
// distance of its order key from ot (backward: ot - rot, forward: rot - ot;
// both are >= 0 by the definition of P and Q when the keys are equal)
template <bool OKEYS>
DEV bool asof_valid(const u64* rk, const u64* rt, long n, long c, u64 k,
                    u64 ot, bool back, bool has_tol, u64 tol, bool f64,
                    u64& dist) {
  if (c < 0 || c >= n) return false;
  if (rk[c] != k) return false;
  const u64 ct = asof_rot<OKEYS>(rt, c, f64);
  dist = back ? ot - ct : ct - ot;
  return !has_tol || dist <= tol;
}

// one left row (k, ot) over the right rows (rk, rt)[0, n): the matched
// index in [0, n), or -1
template <bool OKEYS>
DEV long asof_match(const u64* rk, const u64* rt, long n, u64 k, u64 ot,
                    int dir, bool exact, bool has_tol, u64 tol, bool f64) {
  // backward needs Q (exact) or P (strict), forward the other one, nearest
  // both; Q >= P, so its search starts at P when P is known
  const bool need_p = dir == ASOF_NEAREST || (dir == ASOF_FORWARD) == exact;
  const bool need_q = dir == ASOF_NEAREST || (dir == ASOF_BACKWARD) == exact;
  long p = 0, q = 0;
  if (need_p) p = asof_bound<OKEYS>(rk, rt, 0, n, k, ot, false, f64);
  if (need_q) q = asof_bound<OKEYS>(rk, rt, p, n, k, ot, true, f64);
  const long cb = exact ? q - 1 : p - 1;
  const long cf = exact ? p : q;
  u64 db = 0, df = 0;
  const bool vb =
      dir != ASOF_FORWARD &&
      asof_valid<OKEYS>(rk, rt, n, cb, k, ot, true, has_tol, tol, f64, db);
  const bool vf =
      dir != ASOF_BACKWARD &&
      asof_valid<OKEYS>(rk, rt, n, cf, k, ot, false, has_tol, tol, f64, df);
  if (vb && (!vf || db <= df)) return cb;
  return vf ? cf : -1;
}

__global__ __launch_bounds__(ASOF_BLOCK) void asof_row_kernel(
    const u64* __restrict__ lk, const u64* __restrict__ lt, long nl,
    const u64* __restrict__ rk, const u64* __restrict__ rt, long nr, int dir,
    int exact, int has_tol, u64 tol, int f64, i64* __restrict__ ri) {
  const long stride = (long)gridDim.x * ASOF_BLOCK;
  for (long i = (long)blockIdx.x * ASOF_BLOCK + threadIdx.x; i < nl;
       i += stride)
    ri[i] = asof_match<false>(rk, rt, nr, lk[i], group_okey(lt[i], f64 != 0),
                              dir, exact != 0, has_tol != 0, tol, f64 != 0);
}

__global__ __launch_bounds__(ASOF_BLOCK) void asof_window_kernel(
    const u64* __restrict__ lk, const u64* __restrict__ lt, long nl,
    const u64* __restrict__ rk, const u64* __restrict__ rt, long nr,
    long ntiles, int dir, int exact_, int has_tol_, u64 tol, int f64_,
    i64* __restrict__ ri) {
  // exactly 32 KB, so five blocks share a CU's 160 KB: the window's two
  // bounds travel through s_rt[0] and s_rt[1] before the staging loop
  // overwrites them (hence the barrier between reading them and staging)
  __shared__ u64 s_rk[ASOF_WIN];
  __shared__ u64 s_rt[ASOF_WIN];  // order keys of the window's times

  const int tid = threadIdx.x;
  const int wave = tid / WAVE;
  const bool exact = exact_ != 0, has_tol = has_tol_ != 0, f64 = f64_ != 0;

  for (long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const long t0 = tile * ASOF_TILE;
    const long t1 = t0 + ASOF_TILE < nl ? t0 + ASOF_TILE : nl;

    // the window [P(first row) - 1, Q(last row) + 1), clipped to [0, nr)
    if (wave == 0) {
      const long p = asof_bound_wave(rk, rt, nr, lk[t0],
                                     group_okey(lt[t0], f64), false, f64);
      if (tid == 0) s_rt[0] = (u64)(p > 0 ? p - 1 : 0);
    } else if (wave == 1) {
      const long q = asof_bound_wave(rk, rt, nr, lk[t1 - 1],
                                     group_okey(lt[t1 - 1], f64), true, f64);
      if (tid == WAVE) s_rt[1] = (u64)(q + 1 < nr ? q + 1 : nr);
    }
    __syncthreads();
    const long wlo = (long)s_rt[0];
    const long whi = (long)s_rt[1];
    const long wn = whi > wlo ? whi - wlo : 0;
    const bool fits = wn <= ASOF_WIN;  // block-uniform
    __syncthreads();  // every thread holds the bounds: s_rt may be staged
    if (fits)
      for (int s = tid; s < (int)wn; s += ASOF_BLOCK) {
        s_rk[s] = rk[wlo + s];
        s_rt[s] = group_okey(rt[wlo + s], f64);
      }
    __syncthreads();

    for (long i = t0 + tid; i < t1; i += ASOF_BLOCK) {
      const u64 k = lk[i];
      const u64 ot = group_okey(lt[i], f64);
      const long m =
          fits ? asof_match<true>(s_rk, s_rt, wn, k, ot, dir, exact, has_tol,
                                  tol, f64)
               : asof_match<false>(rk + wlo, rt + wlo, wn, k, ot, dir, exact,
                                   has_tol, tol, f64);
      ri[i] = m < 0 ? -1 : wlo + m;
    }
    __syncthreads();  // s_rk and s_rt are rewritten by the next tile
  }
}
