// Lexicographic ordering of the exemplar dictionary (K1 string form).
//
// Strings live in a u8 text buffer and are named by packed positions
// (off << 16 | len).  lex_chunk_keys turns the d-th 8-byte chunk of each
// string into a big-endian u64, so the existing u64 radix sort orders
// strings bytewise one chunk at a time; lex_refine splits tied segments
// after each chunk; lex_lower_bound binary-searches the finished
// permutation (prefix / range serving).
//
// Bounds discipline (all three kernels): a string is first clamped to
// [0, text_len), and no load touches a byte outside
// [text, text + text_len) — the buffer may be a view at any storage
// offset and of any size, and its neighbours belong to someone else.
#pragma once

#include "common.h"

// (start, len) of a packed position, clamped to the buffer
DEV void lex_span(u64 p, long text_len, long& start, long& len) {
  start = (long)(p >> 16);
  len = (long)(p & 0xFFFF);
  if (start >= text_len) {
    start = 0;
    len = 0;
  } else if (len > text_len - start) {
    len = text_len - start;
  }
}

// The aligned 8-byte word at absolute address `a` (a % 8 == 0), little
// endian.  One 8-byte load when the whole word lies inside [lo, hi);
// otherwise guarded byte loads, out-of-range bytes reading as zero.
DEV u64 lex_load_word(uintptr_t a, uintptr_t lo, uintptr_t hi) {
  if (a >= lo && a + 8 <= hi) return *reinterpret_cast<const u64*>(a);
  u64 w = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    uintptr_t b = a + j;
    if (b >= lo && b < hi)
      w |= (u64)(*reinterpret_cast<const u8*>(b)) << (8 * j);
  }
  return w;
}

// out_keys[i] = big-endian u64 of bytes [8d, 8d+8) of string idx[i]
// (idx == nullptr: identity), zero beyond the string's length — so
// unsigned u64 order == bytewise order of the zero-padded chunk.
// Every string start is unaligned; instead of 8 dependent byte loads the
// chunk is cut from the (at most two) aligned words that cover it with a
// funnel shift, then byte-swapped.  Alignment comes from the absolute
// address, so a text view with a nonzero storage offset stays on the
// aligned-load path.
__global__ void lex_chunk_keys_kernel(const u8* __restrict__ text,
                                      long text_len,
                                      const u64* __restrict__ pos,
                                      const i64* __restrict__ idx, long m,
                                      long d, u64* __restrict__ out_keys) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  const uintptr_t lo = reinterpret_cast<uintptr_t>(text);
  const uintptr_t hi = lo + (uintptr_t)text_len;
  for (; i < m; i += stride) {
    long s = idx ? (long)idx[i] : i;
    long start, len;
    lex_span(pos[s], text_len, start, len);
    long rem = len - 8 * d;  // bytes of the string from this chunk on
    u64 v = 0;
    if (rem > 0) {
      int need = rem < 8 ? (int)rem : 8;
      uintptr_t addr = lo + (uintptr_t)(start + 8 * d);
      int sh = (int)(addr & 7);
      uintptr_t a0 = addr - sh;
      v = lex_load_word(a0, lo, hi) >> (8 * sh);
      if (sh + need > 8)  // chunk crosses into the next aligned word
        v |= lex_load_word(a0 + 8, lo, hi) << (64 - 8 * sh);
      if (need < 8) v &= (~0ull) >> (64 - 8 * need);
      v = __builtin_bswap64(v);
    }
    out_keys[i] = v;
  }
}

// After the active elements were sorted by (seg, chunk-d key): an element
// heads a new segment iff its (seg, key) pair differs from its
// predecessor's; more[i] = string idx[i] still has bytes beyond chunk d
// (the host loop keeps refining only segments that hold >= 2 of those).
__global__ void lex_refine_kernel(const i64* __restrict__ seg,
                                  const u64* __restrict__ keys,
                                  const u64* __restrict__ pos,
                                  const i64* __restrict__ idx, long m, long d,
                                  i64* __restrict__ flags,
                                  i64* __restrict__ more) {
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  for (; i < m; i += stride) {
    flags[i] = (i == 0) || seg[i] != seg[i - 1] || keys[i] != keys[i - 1];
    long len = (long)(pos[idx[i]] & 0xFFFF);
    more[i] = len > 8 * (d + 1);
  }
}

// One thread per query: out[q] = smallest j with string(perm[j]) >= query
// (bytewise unsigned over the common length, shorter first on a tie).
// Serving path, nq small: plain guarded byte loads.
__global__ void lex_lower_bound_kernel(const u8* __restrict__ text,
                                       long text_len,
                                       const u64* __restrict__ pos,
                                       const i64* __restrict__ perm, long n,
                                       const u8* __restrict__ qblob,
                                       const i64* __restrict__ qoff, long nq,
                                       i64* __restrict__ out) {
  long q = (long)blockIdx.x * blockDim.x + threadIdx.x;
  long stride = (long)gridDim.x * blockDim.x;
  for (; q < nq; q += stride) {
    long q0 = qoff[q];
    long qlen = qoff[q + 1] - q0;
    long lo = 0, hi = n;
    while (lo < hi) {
      long mid = lo + ((hi - lo) >> 1);
      long start, len;
      lex_span(pos[perm[mid]], text_len, start, len);
      long common = len < qlen ? len : qlen;
      int cmp = 0;  // sign of string(perm[mid]) - query
      for (long j = 0; j < common; ++j) {
        int a = text[start + j], b = qblob[q0 + j];
        if (a != b) {
          cmp = a < b ? -1 : 1;
          break;
        }
      }
      if (cmp == 0) cmp = len < qlen ? -1 : 0;
      if (cmp < 0) lo = mid + 1;
      else hi = mid;
    }
    out[q] = lo;
  }
}
