// Ranked multi-term search over the inverted index (serving path).
//
// The index is CSR: keys[nwords] (u64 word hashes, sorted unsigned),
// doc_offsets[nwords + 1] into docs[np] / tf[np], doc ids ascending and
// unique within a word.  One 256-thread block answers one query of up to
// PQ_TMAX terms; a batch of queries is one launch.
//
//   AND  documents present in every term's list.  The shortest list drives
//        (ties: earliest term); each driver doc is binary-searched in the
//        other lists.  An unknown term resolves to an empty list, which
//        then drives: no tiles, empty result.
//   OR   documents present in at least one list, each once: the posting of
//        list j owns its doc iff the doc is in no list j' < j; the owner
//        sums the score over all lists.
//   score = sum over the query's terms present in the doc of
//        tf * weight[term row], wrapping i64; weights == nullptr means 1.
//   order: score descending, doc ascending on equal score.
//
// Selection: matches are appended to an LDS buffer of PQ_BUF (score, doc)
// entries through an LDS counter.  A tile adds at most PQ_BLOCK entries;
// when the next tile could overflow, the block sorts the buffer (bitonic)
// and keeps the best k — exact, because an entry outside the best k of a
// subset is outside the best k of the whole.
//
// Control flow: every __syncthreads() is in block-uniform flow.  Trip
// counts come from the LDS term table and the prune decision from the LDS
// counter, both read by every thread between two barriers; no branch that
// holds a barrier depends on a thread's own match state.
//
// Bounds: key loads stay in [0, nwords), offset loads in [0, nwords],
// posting loads in [0, np) (row spans are clamped to it), query loads in
// the query arrays.  The arrays may be exact-size views of larger
// allocations whose neighbours belong to someone else.
#pragma once

#include "common.h"

#define PQ_BLOCK 256
#define PQ_TMAX 16
#define PQ_KMAX 256
#define PQ_BUF 2048
#define PQ_MODE_AND 0
#define PQ_MODE_OR 1

static_assert(PQ_KMAX + PQ_BLOCK <= PQ_BUF,
              "a pruned buffer must take one more tile");
static_assert((PQ_BUF & (PQ_BUF - 1)) == 0, "bitonic sort wants a power of 2");

// (score, doc) ordering of the result: a comes strictly before b
DEV bool pq_before(i64 sa, i64 da, i64 sb, i64 db) {
  return sa > sb || (sa == sb && da < db);
}

// index of doc d in the ascending list docs[start, start + len), or -1
DEV long pq_find(const i64* __restrict__ docs, long start, long len, i64 d) {
  long lo = 0, hi = len;
  for (int step = 0; step < 64 && lo < hi; ++step) {
    long mid = lo + ((hi - lo) >> 1);
    if (docs[start + mid] < d) lo = mid + 1;
    else hi = mid;
  }
  if (lo < len && docs[start + lo] == d) return lo;
  return -1;
}

// Sort the first cnt buffer entries best-first.  Called by the whole block
// with a block-uniform cnt; ends on a barrier.  Slots [cnt, n2) are padded
// with an entry nothing sorts behind.
DEV void pq_sort(i64* s_score, i64* s_doc, int cnt) {
  const int tid = threadIdx.x;
  int n2 = 2;
  while (n2 < cnt) n2 <<= 1;  // cnt <= PQ_BUF: at most 10 doublings
  for (int i = cnt + tid; i < n2; i += PQ_BLOCK) {
    s_score[i] = INT64_MIN;
    s_doc[i] = INT64_MAX;
  }
  __syncthreads();
  for (int kk = 2; kk <= n2; kk <<= 1) {
    for (int j = kk >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < n2; i += PQ_BLOCK) {
        int p = i ^ j;
        if (p > i) {
          i64 sa = s_score[i], da = s_doc[i];
          i64 sb = s_score[p], db = s_doc[p];
          bool up = (i & kk) == 0;
          if (pq_before(sb, db, sa, da) == up) {
            s_score[i] = sb;
            s_doc[i] = db;
            s_score[p] = sa;
            s_doc[p] = da;
          }
        }
      }
      __syncthreads();
    }
  }
}

__global__ __launch_bounds__(PQ_BLOCK) void postings_search_kernel(
    const u64* __restrict__ keys, long nwords,
    const i64* __restrict__ doc_offsets, const i64* __restrict__ docs,
    const i64* __restrict__ tf, long np, const i64* __restrict__ weights,
    const u64* __restrict__ qkeys, long total_terms,
    const i64* __restrict__ qoff, int k, int mode,
    i64* __restrict__ out_docs, i64* __restrict__ out_scores,
    i64* __restrict__ out_n, i64* __restrict__ out_hits) {
  __shared__ i64 s_score[PQ_BUF];
  __shared__ i64 s_doc[PQ_BUF];
  __shared__ long t_start[PQ_TMAX];
  __shared__ long t_len[PQ_TMAX];
  __shared__ i64 t_w[PQ_TMAX];
  __shared__ int s_cnt;
  __shared__ unsigned long long s_hits;

  const int tid = threadIdx.x;
  const long q = blockIdx.x;

  // the query's term span; a malformed one reads as "no terms"
  long q0 = qoff[q];
  long tq = qoff[q + 1] - q0;
  if (tq < 0 || tq > PQ_TMAX || q0 < 0 || q0 + tq > total_terms) tq = 0;
  const int T = (int)tq;

  // term table: (row start, length, weight); unknown term = empty list
  if (tid < T) {
    u64 h = qkeys[q0 + tid];
    long lo = 0, hi = nwords;
    for (int step = 0; step < 64 && lo < hi; ++step) {
      long mid = lo + ((hi - lo) >> 1);
      if (keys[mid] < h) lo = mid + 1;
      else hi = mid;
    }
    long start = 0, len = 0;
    i64 w = 1;
    if (lo < nwords && keys[lo] == h) {
      start = doc_offsets[lo];
      len = doc_offsets[lo + 1] - start;
      if (start < 0 || start > np) {
        start = 0;
        len = 0;
      }
      if (len < 0) len = 0;
      if (len > np - start) len = np - start;
      if (weights) w = weights[lo];
    }
    t_start[tid] = start;
    t_len[tid] = len;
    t_w[tid] = w;
  }
  if (tid == 0) {
    s_cnt = 0;
    s_hits = 0;
  }
  __syncthreads();

  // lists whose postings generate candidates: AND = the shortest list
  // (none for an empty query), OR = every list
  int jbeg = 0, jend = T;
  if (mode == PQ_MODE_AND) {
    int drv = 0;
    for (int j = 1; j < T; ++j)
      if (t_len[j] < t_len[drv]) drv = j;
    jbeg = drv;
    jend = T > 0 ? drv + 1 : 0;
  }

  unsigned long long my_hits = 0;
  for (int j = jbeg; j < jend; ++j) {
    const long L = t_len[j];
    const long st = t_start[j];
    const i64 wj = t_w[j];
    for (long base = 0; base < L; base += PQ_BLOCK) {
      __syncthreads();  // the previous tile's appends are done
      const int c = s_cnt;
      __syncthreads();  // everyone holds the same c before it moves
      if (c + PQ_BLOCK > PQ_BUF) {
        pq_sort(s_score, s_doc, c);
        if (tid == 0) s_cnt = c < k ? c : k;
        __syncthreads();
      }
      const long i = base + tid;
      if (i < L) {
        const i64 d = docs[st + i];
        i64 sc = tf[st + i] * wj;
        bool ok = true;
        for (int o = 0; o < T && ok; ++o) {
          if (o == j) continue;
          long p = pq_find(docs, t_start[o], t_len[o], d);
          if (p >= 0) {
            if (mode == PQ_MODE_OR && o < j) ok = false;  // list o owns d
            else sc += tf[t_start[o] + p] * t_w[o];
          } else if (mode == PQ_MODE_AND) {
            ok = false;
          }
        }
        if (ok) {
          int slot = atomicAdd(&s_cnt, 1);
          if (slot < PQ_BUF) {  // always: c + PQ_BLOCK <= PQ_BUF here
            s_score[slot] = sc;
            s_doc[slot] = d;
          }
          ++my_hits;
        }
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
