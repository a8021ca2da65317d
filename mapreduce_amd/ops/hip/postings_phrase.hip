// Exact-phrase search over the positional inverted index (serving path).
//
// On top of the CSR index of postings_query.hip, posting j (one word in one
// document) owns the ascending token ordinals
// positions[pos_offsets[j] : pos_offsets[j] + tf[j]] (i32) of the word in
// that document.  A query is the ORDERED terms h_0 .. h_{T-1}, duplicates
// kept.  Document d matches iff every term has a posting for d and some
// s >= 0 has s + i in P(h_i, d) for every i; score(d) = the number of such
// s (the phrase frequency; tf for T == 1).  Order, padding, caps and the
// top-k selection are those of postings_search_kernel.
//
// One 256-thread block per query.  The shortest doc list drives (term r,
// ties: the earliest).  Each tile of PQ_BLOCK driver postings runs in two
// phases:
//   A  thread per posting: the doc is binary-searched in the other lists;
//      survivors go into an LDS candidate list;
//   B  wave per candidate: lane o < T locates term o's posting and its
//      position slice, the wave strides the driver's positions p; p < r
//      is rejected (never wrapped), otherwise p - r + i is binary-searched
//      in term i's slice; a wave reduction gives the count.
// One posting with thousands of positions thus occupies 64 lanes, not one.
//
// Control flow: every __syncthreads() is in block-uniform flow — trip
// counts come from the LDS term table, the prune decision from the LDS
// counter and the phase B trip count from the LDS candidate counter, each
// read by every thread between two barriers.  Shuffles sit in wave-uniform
// flow: the candidate index and the position-loop bound are wave-uniform.
//
// Bounds: as postings_search_kernel for keys, offsets, postings and the
// query; pos_offsets loads stay in [0, np) (one per located posting),
// position loads in [0, nocc) (slices are clamped to it).
#pragma once

#include "postings_query.hip"

#define PP_WAVES (PQ_BLOCK / WAVE)

// is v in the ascending slice positions[start, start + len)?
DEV bool pp_has(const int* __restrict__ positions, long start, long len,
                long v) {
  long lo = 0, hi = len;
  for (int step = 0; step < 64 && lo < hi; ++step) {
    long mid = lo + ((hi - lo) >> 1);
    if ((long)positions[start + mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo < len && (long)positions[start + lo] == v;
}

__global__ __launch_bounds__(PQ_BLOCK) void postings_phrase_kernel(
    const u64* __restrict__ keys, long nwords,
    const i64* __restrict__ doc_offsets, const i64* __restrict__ docs,
    const i64* __restrict__ tf, long np, const i64* __restrict__ pos_offsets,
    const int* __restrict__ positions, long nocc,
    const u64* __restrict__ qkeys, long total_terms,
    const i64* __restrict__ qoff, int k, i64* __restrict__ out_docs,
    i64* __restrict__ out_scores, i64* __restrict__ out_n,
    i64* __restrict__ out_hits) {
  __shared__ i64 s_score[PQ_BUF];
  __shared__ i64 s_doc[PQ_BUF];
  __shared__ long t_start[PQ_TMAX];
  __shared__ long t_len[PQ_TMAX];
  __shared__ int c_idx[PQ_BLOCK];  // candidates: posting index in the tile
  __shared__ int c_n;
  __shared__ int s_cnt;
  __shared__ unsigned long long s_hits;

  const int tid = threadIdx.x;
  const int lane = tid & (WAVE - 1);
  const int wave = tid / WAVE;
  const long q = blockIdx.x;

  // the query's term span; a malformed one reads as "no terms"
  long q0 = qoff[q];
  long tq = qoff[q + 1] - q0;
  if (tq < 0 || tq > PQ_TMAX || q0 < 0 || q0 + tq > total_terms) tq = 0;
  const int T = (int)tq;

  // term table: (row start, length); unknown term = empty list
  if (tid < T) {
    u64 h = qkeys[q0 + tid];
    long lo = 0, hi = nwords;
    for (int step = 0; step < 64 && lo < hi; ++step) {
      long mid = lo + ((hi - lo) >> 1);
      if (keys[mid] < h) lo = mid + 1;
      else hi = mid;
    }
    long start = 0, len = 0;
    if (lo < nwords && keys[lo] == h) {
      start = doc_offsets[lo];
      len = doc_offsets[lo + 1] - start;
      if (start < 0 || start > np) {
        start = 0;
        len = 0;
      }
      if (len < 0) len = 0;
      if (len > np - start) len = np - start;
    }
    t_start[tid] = start;
    t_len[tid] = len;
  }
  if (tid == 0) {
    s_cnt = 0;
    s_hits = 0;
    c_n = 0;
  }
  __syncthreads();

  // the shortest list drives (ties: the earliest term); an empty query
  // and an unknown term drive no tile
  int r = 0;
  for (int j = 1; j < T; ++j)
    if (t_len[j] < t_len[r]) r = j;
  const long L = T > 0 ? t_len[r] : 0;
  const long st = T > 0 ? t_start[r] : 0;

  unsigned long long my_hits = 0;
  for (long base = 0; base < L; base += PQ_BLOCK) {
    __syncthreads();  // the previous tile's appends and c_n reads are done
    const int c = s_cnt;
    if (tid == 0) c_n = 0;
    __syncthreads();  // everyone holds the same c before it moves
    if (c + PQ_BLOCK > PQ_BUF) {
      pq_sort(s_score, s_doc, c);
      if (tid == 0) s_cnt = c < k ? c : k;
      __syncthreads();
    }

    // phase A: docs of this tile present in every other list
    const long i = base + tid;
    if (i < L) {
      const i64 d = docs[st + i];
      bool ok = true;
      for (int o = 0; o < T && ok; ++o) {
        if (o == r) continue;
        ok = pq_find(docs, t_start[o], t_len[o], d) >= 0;
      }
      if (ok) c_idx[atomicAdd(&c_n, 1)] = tid;  // < PQ_BLOCK: one per thread
    }
    __syncthreads();
    const int nc = c_n;

    // phase B: one wave per candidate (ci and nc are wave-uniform)
    for (int ci = wave; ci < nc; ci += PP_WAVES) {
      const long jr = st + base + c_idx[ci];  // driver posting, < np
      const i64 d = docs[jr];
      // lane o < T: term o's posting for d and its clamped position slice
      long ps = 0, pl = 0;
      if (lane < T) {
        long j = jr;
        if (lane != r) {
          long f = pq_find(docs, t_start[lane], t_len[lane], d);
          j = f >= 0 ? t_start[lane] + f : -1;  // found in phase A
        }
        if (j >= 0) {
          ps = pos_offsets[j];
          pl = tf[j];
          if (ps < 0 || ps > nocc) {
            ps = 0;
            pl = 0;
          }
          if (pl < 0) pl = 0;
          if (pl > nocc - ps) pl = nocc - ps;
        }
      }
      const long dps = __shfl(ps, r, WAVE);
      const long dpl = __shfl(pl, r, WAVE);
      i64 cnt = 0;
      for (long pb = 0; pb < dpl; pb += WAVE) {  // dpl is wave-uniform
        const long pi = pb + lane;
        const bool act = pi < dpl;
        const long s = act ? (long)positions[dps + pi] - r : -1;
        bool ok = act && s >= 0;  // p < r: no start, never wrapped
        for (int o = 0; o < T; ++o) {
          const long ops_ = __shfl(ps, o, WAVE);
          const long opl = __shfl(pl, o, WAVE);
          if (ok && o != r) ok = pp_has(positions, ops_, opl, s + o);
        }
        if (ok) ++cnt;
      }
      cnt = wave_sum_i64(cnt);
      if (lane == 0 && cnt > 0) {
        int slot = atomicAdd(&s_cnt, 1);
        if (slot < PQ_BUF) {  // always: c + PQ_BLOCK <= PQ_BUF here
          s_score[slot] = cnt;
          s_doc[slot] = d;
        }
        ++my_hits;
      }
    }
  }

  if (my_hits) atomicAdd(&s_hits, my_hits);
  __syncthreads();
  const int c = s_cnt < PQ_BUF ? s_cnt : PQ_BUF;
  __syncthreads();
  pq_sort(s_score, s_doc, c);
  const int n = c < k ? c : k;
  for (int i = tid; i < k; i += PQ_BLOCK) {
    out_docs[q * k + i] = i < n ? s_doc[i] : -1;
    out_scores[q * k + i] = i < n ? s_score[i] : 0;
  }
  if (tid == 0) {
    out_n[q] = n;
    out_hits[q] = (i64)s_hits;
  }
}
