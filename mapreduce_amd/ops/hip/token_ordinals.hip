// Token ordinals: the 0-based index of a word among the words of its
// document (the position unit of the positional index and of phrase
// search), computed without sorting the occurrences.
//
//   word start       a non-whitespace byte whose predecessor is whitespace
//                    or which is byte 0 of the text
//   starts_before(x) number of word starts at offsets < x
//   doc(off)         index of the last split offset <= off (ub_minus1, the
//                    rule of the composite tokenizer)
//   ord(off)         starts_before(off) - starts_before(starts[doc])
//
// A split that begins mid-word holds no start for that fragment, like the
// tokenizer, which tokenizes the whole text and gives a word to the
// document of its first byte.
//
// Three passes: tord_count_kernel streams the text once and counts the
// starts of every TORD_GRANULE-byte granule (8 lanes x 8 bytes, ws_mask8 +
// popcount, carry between lanes by shuffle); the host scans the counts;
// tord_before_kernel / tord_resolve_kernel add to a granule's prefix the
// popcount of the start mask of the partial granule below x.
//
// Bounds: text loads stay in [0, n).  Byte -1 reads as whitespace (the
// carry into the first granule) and bytes >= n as whitespace (they hold no
// start); neither is loaded.  8-byte loads are taken only when whole and
// 8-aligned on the absolute address, so text may be an exact-size view at
// any offset of a larger allocation.  prefix has ngran + 1 entries, pos m,
// starts nstarts >= 1, doc_sb nstarts.
#pragma once

#include "common.h"

#define TORD_GRANULE 64
#define TORD_BLOCK 256

static_assert(TORD_GRANULE == 64, "8 lanes of 8 bytes make one granule");

// the 8 bytes at offset off >= 0 as a little-endian u64; bytes at or past n
// read as ' ' without being loaded
DEV u64 tord_load8(const u8* __restrict__ text, long n, long off) {
  if (off + 8 <= n && (((uintptr_t)(text + off)) & 7) == 0)
    return *reinterpret_cast<const u64*>(text + off);
  u64 x = 0;
  for (int b = 0; b < 8; ++b) {
    u64 c = off + b < n ? (u64)text[off + b] : (u64)' ';
    x |= c << (8 * b);
  }
  return x;
}

// word-start mask of 8 bytes from their whitespace mask and "the byte
// before them is whitespace"
DEV u32 tord_starts8(u32 ws, bool carry_ws) {
  u32 prev = ((ws << 1) | (carry_ws ? 1u : 0u)) & 0xFF;
  return ~ws & prev & 0xFF;
}

// gcount[g] = word starts in text[64 g, 64 g + 64)
__global__ __launch_bounds__(TORD_BLOCK) void tord_count_kernel(
    const u8* __restrict__ text, long n, int* __restrict__ gcount,
    long ngran) {
  const long units = ngran * (TORD_GRANULE / 8);  // 8-byte units
  const int lane = threadIdx.x & (WAVE - 1);
  const long stride = (long)gridDim.x * TORD_BLOCK;
  // u0 is wave-uniform, so every lane of a wave takes the shuffles together
  for (long u0 = (long)blockIdx.x * TORD_BLOCK + (threadIdx.x - lane);
       u0 < units; u0 += stride) {
    const long u = u0 + lane;
    const long off = u * 8;
    const u32 ws = ws_mask8(tord_load8(text, n, off));
    const u32 up = __shfl_up(ws, 1, WAVE);
    bool carry;
    if (lane == 0) carry = off == 0 || off > n || is_ws(text[off - 1]);
    else carry = (up >> 7) & 1;
    int c = __popc(tord_starts8(ws, carry));
    c += __shfl_xor(c, 1, WAVE);
    c += __shfl_xor(c, 2, WAVE);
    c += __shfl_xor(c, 4, WAVE);
    if ((lane & 7) == 0 && u < units) gcount[u >> 3] = c;
  }
}

// starts_before(x), x clamped to [0, n]
DEV int tord_before(const u8* __restrict__ text, long n,
                    const int* __restrict__ prefix, long x) {
  if (x < 0) x = 0;
  if (x > n) x = n;
  const long g = x / TORD_GRANULE;  // <= n / 64 <= ngran
  int cnt = prefix[g];
  long off = g * TORD_GRANULE;
  if (off >= x) return cnt;
  bool carry = off == 0 || is_ws(text[off - 1]);  // off - 1 < x <= n
  for (; off < x; off += 8) {
    const u32 ws = ws_mask8(tord_load8(text, n, off));
    u32 st = tord_starts8(ws, carry);
    const long rem = x - off;
    if (rem < 8) st &= (1u << rem) - 1;
    cnt += __popc(st);
    carry = (ws >> 7) & 1;
  }
  return cnt;
}

// out[i] = starts_before(x[i])
__global__ __launch_bounds__(TORD_BLOCK) void tord_before_kernel(
    const u8* __restrict__ text, long n, const int* __restrict__ prefix,
    const i64* __restrict__ x, long m, int* __restrict__ out) {
  const long stride = (long)gridDim.x * TORD_BLOCK;
  for (long i = (long)blockIdx.x * TORD_BLOCK + threadIdx.x; i < m;
       i += stride)
    out[i] = tord_before(text, n, prefix, x[i]);
}

// per occurrence pos = off << 16 | len: its document and its ordinal there
__global__ __launch_bounds__(TORD_BLOCK) void tord_resolve_kernel(
    const u8* __restrict__ text, long n, const int* __restrict__ prefix,
    const u64* __restrict__ pos, long m, const i64* __restrict__ starts,
    int nstarts, const int* __restrict__ doc_sb, i64* __restrict__ out_doc,
    int* __restrict__ out_ord) {
  const long stride = (long)gridDim.x * TORD_BLOCK;
  for (long i = (long)blockIdx.x * TORD_BLOCK + threadIdx.x; i < m;
       i += stride) {
    const i64 off = (i64)(pos[i] >> 16);
    const int d = ub_minus1(starts, nstarts, off);
    const int dc = d < 0 ? 0 : d;  // d <= nstarts - 1 by construction
    out_doc[i] = d;
    out_ord[i] = tord_before(text, n, prefix, off) - doc_sb[dc];
  }
}
