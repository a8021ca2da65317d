// Torch extension glue for the MapReduce CDNA4 kernels (single TU).
//
// Tensors use int64 storage for 64-bit keys; kernels reinterpret the bits as
// u64 (all ordering/partitioning comparisons happen inside kernels, so
// torch's signed view never matters).  Everything launches on the current
// HIP stream; nothing here synchronizes except the explicitly named *_count
// readbacks, which callers do lazily.

#include <ATen/hip/HIPContext.h>
#include <torch/extension.h>

#include <limits>
#include <map>
#include <mutex>
#include <optional>
#include <utility>

#include "asof.hip"
#include "extract_sorted.hip"
#include "frame.hip"
#include "gradsum.hip"
#include "graph.hip"
#include "group.hip"
#include "join.hip"
#include "lex_order.hip"
#include "mr_kernels.hip"
#include "postings_phrase.hip"
#include "postings_query.hip"
#include "radix_sort.hip"
#include "seg_scan.hip"
#include "token_ordinals.hip"

namespace {

constexpr int kBlock = 256;
// G11: memory-bound grid-stride kernels cap the grid and stride the rest
constexpr long kMaxBlocks = 2048;

long grid_for(long n, long per_thread = 1) {
  long want = (n + (long)kBlock * per_thread - 1) / ((long)kBlock * per_thread);
  if (want < 1) want = 1;
  return want < kMaxBlocks ? want : kMaxBlocks;
}

hipStream_t cur_stream() { return at::hip::getCurrentHIPStream(); }

// Grid of the LDS-cached tokenizer launches.  Every block carries fixed
// costs (a cold word cache, an end-of-kernel flush of that cache into the
// global table, one stranded spill chunk per wave), and whatever it leaves
// free on a CU is what the drain kernels of the previous job run in when
// jobs are pipelined.  So the grid is ONE round of at most kTokWavesPerCu
// waves per CU, never more blocks than the kernel's registers + LDS admit
// (occupancy query, once per instantiation and device), never more than
// kMaxBlocks (the spill slack and the cpos side buffers are sized for
// that many).  Measured on the bench shape, pipelined ms/step: 1024
// blocks 1.29-1.35, 2048 (the old fixed grid) 1.37-1.44, 768 1.39-1.42,
// 1280 (all the query admits) 1.38-1.42, 1536 1.48-1.49 — the grid also
// sets total cache capacity and how many 2048-entry spill chunks a wave
// strands (profiles/tokenizer_occupancy_r04.md).
constexpr int kTokWavesPerCu = 16;

struct TokOccupancy {
  int blocks_per_cu = 0;
  int cus = 0;
};

TokOccupancy tok_occupancy(const void* kfn, int blockn) {
  static std::mutex mu;
  static std::map<std::pair<const void*, int>, TokOccupancy> cache;
  int dev = 0;
  C10_HIP_CHECK(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(mu);
  auto it = cache.find({kfn, dev});
  if (it != cache.end()) return it->second;
  TokOccupancy o;
  C10_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(
      &o.blocks_per_cu, kfn, blockn, 0));
  C10_HIP_CHECK(hipDeviceGetAttribute(
      &o.cus, hipDeviceAttributeMultiprocessorCount, dev));
  TORCH_CHECK(o.blocks_per_cu > 0 && o.cus > 0,
              "tokenizer occupancy query returned ", o.blocks_per_cu,
              " blocks/CU on ", o.cus, " CUs");
  cache[{kfn, dev}] = o;
  return o;
}

template <typename K>
long tok_grid(K kfn, int blockn, long n, long tile_bytes) {
  long tiles = (n + tile_bytes - 1) / tile_bytes;
  if (tiles < 1) tiles = 1;
  TokOccupancy o = tok_occupancy(reinterpret_cast<const void*>(kfn), blockn);
  int per_cu = kTokWavesPerCu / (blockn / WAVE);
  if (per_cu > o.blocks_per_cu) per_cu = o.blocks_per_cu;
  long resident = (long)per_cu * o.cus;
  long blocks = tiles < resident ? tiles : resident;
  return blocks < kMaxBlocks ? blocks : kMaxBlocks;
}

// LDS-staged scatter is the default — direct scatter (v1) measured
// ~2.5x slower on write coalescing; MR_RADIX_V1=1 switches back for A/B.
// The staged scatter ranks once from registers (v3, radix_sort.hip);
// MR_RADIX_V2=1 selects its predecessor with the per-round block barriers
// (v2, same output bit for bit), and the bucketize histogram that went
// with it, for A/B inside one session.  Both switches are read once per
// process.
// MR_RS_ITEMS ∈ {4, 8}: radix tile = 256*ITEMS.  8 = longer digit runs
// (better write coalescing), 4 = half the LDS stage (38->22 KB, 4->7
// blocks/CU).  v1 (direct scatter) stays ITEMS=8.
int rs_items() {
  static int v = -1;
  if (v < 0) {
    const char* e = getenv("MR_RS_ITEMS");
    const char* v1 = getenv("MR_RADIX_V1");  // v1 kernel is ITEMS=8 only
    v = (e && atoi(e) == 4 && !(v1 && v1[0] == '1')) ? 4 : 8;
  }
  return v;
}

long rs_tile() { return (long)RS_BLOCK * rs_items(); }

bool radix_v1_forced() {
  const char* v = getenv("MR_RADIX_V1");
  return v && v[0] == '1';
}

bool radix_v2_forced() {
  static int f = -1;
  if (f < 0) {
    const char* v = getenv("MR_RADIX_V2");
    f = (v && v[0] == '1') ? 1 : 0;
  }
  return f == 1;
}

// The tokenizer body of the cached word-count, spill-all and composite
// launches is tokenize_v7_kernel (next tile prefetched into registers, a
// word's first chunk extracted with byte-aligns); MR_TOKENIZE_V6=1, read
// once per process, selects its predecessor for A/B inside one session.
// Both cache and spill the same words, so results are the same.
bool tok_v6_forced() {
  static int f = -1;
  if (f < 0) {
    const char* v = getenv("MR_TOKENIZE_V6");
    f = (v && v[0] == '1') ? 1 : 0;
  }
  return f == 1;
}

static_assert(kBlock == TOK_THREADS, "v6 / v7 launches use kBlock threads");

// Which body the most recent v6/v7 tokenizer launch of this process
// dispatched ("v7", "v6", or "none" before the first): set where the kernel
// pointer is chosen, so tests see the launchers' decision itself.
const char* g_tok_last_body = "none";

// max_blocks of the tokenizer bindings: 0 keeps the launcher's grid,
// anything else caps it (clamped to [1, kMaxBlocks]) so that a small input
// can make one block walk several tiles.
long tok_cap_blocks(long blocks, long max_blocks) {
  if (max_blocks == 0) return blocks;
  long m = max_blocks < 1 ? 1 : (max_blocks > kMaxBlocks ? kMaxBlocks
                                                         : max_blocks);
  return blocks < m ? blocks : m;
}

// the staged scatter this process runs, for one set of template arguments.
// LATE (v3 only) = fetch the payload at staging time instead of up front:
// faster for the full sorts (TeraSort's 671M-record passes: 8.7 against
// 10.4 ms, v2 9.4), while the spill drain's bucketize, which shares the chip
// with the next job's tokenizer, steps faster with everything in flight at
// once (profiles/scatter_rank_r06.md).
#define RS_STAGED_SCATTER(VT, SKIP, BT, LATE)                              \
  (radix_v2_forced()                                                       \
       ? (rs_items() == 4 ? radix_scatter_v2_kernel<4, VT, SKIP, BT>       \
                          : radix_scatter_v2_kernel<8, VT, SKIP, BT>)      \
       : (rs_items() == 4 ? radix_scatter_v3_kernel<4, VT, SKIP, BT, LATE> \
                          : radix_scatter_v3_kernel<8, VT, SKIP, BT, LATE>))

void launch_radix_hist(const u64* kin, long n, int shift, long ntiles,
                       i64* hist) {
  auto kfn = rs_items() == 4 ? radix_hist_kernel<4> : radix_hist_kernel<8>;
  hipLaunchKernelGGL(kfn, dim3(ntiles), dim3(RS_BLOCK), 0, cur_stream(),
                     kin, n, shift, ntiles, hist);
}

void launch_radix_scatter(const u64* kin, const u64* vin, long n, int shift,
                          long ntiles, const i64* base, u64* kout,
                          u64* vout) {
  static int use_v1 = -1;
  if (use_v1 < 0) use_v1 = radix_v1_forced() ? 1 : 0;
  if (use_v1)
    hipLaunchKernelGGL(radix_scatter_kernel, dim3(ntiles), dim3(RS_BLOCK), 0,
                       cur_stream(), kin, vin, n, shift, ntiles, base, kout,
                       vout);
  else {
    auto kfn = RS_STAGED_SCATTER(u64, false, i64, true);
    hipLaunchKernelGGL(kfn, dim3(ntiles), dim3(RS_BLOCK),
                       0, cur_stream(), kin, vin, n, shift, ntiles, base,
                       kout, vout);
  }
}

void launch_radix_scatter32(const u64* kin, const u32* vin, long n,
                            int shift, long ntiles, const i64* base,
                            u64* kout, u32* vout) {
  auto kfn = RS_STAGED_SCATTER(u32, false, i64, true);
  hipLaunchKernelGGL(kfn, dim3(ntiles), dim3(RS_BLOCK), 0, cur_stream(),
                     kin, vin, n, shift, ntiles, base, kout, vout);
}

// bucketize launches: u32 histogram/base, optional HT_EMPTY skip (the
// skip and payload type are template parameters, so the full-sort
// instantiations above are untouched)
template <bool SKIP>
void launch_bucketize_hist(const u64* kin, long n, int shift, long ntiles,
                           u32* hist) {
  // wide loads (WIDE): measured on this histogram only, 46 -> 40 us per
  // job; MR_RADIX_V2=1 brings the narrow form back with the old scatter
  auto kfn = rs_items() == 4 ? radix_hist_kernel<4, SKIP, u32, true>
                             : radix_hist_kernel<8, SKIP, u32, true>;
  if (radix_v2_forced())
    kfn = rs_items() == 4 ? radix_hist_kernel<4, SKIP, u32>
                          : radix_hist_kernel<8, SKIP, u32>;
  hipLaunchKernelGGL(kfn, dim3(ntiles), dim3(RS_BLOCK), 0, cur_stream(),
                     kin, n, shift, ntiles, hist);
}

template <typename VT, bool SKIP>
void launch_bucketize_scatter(const u64* kin, const VT* vin, long n,
                              int shift, long ntiles, const u32* base,
                              u64* kout, VT* vout) {
  auto kfn = RS_STAGED_SCATTER(VT, SKIP, u32, false);
  hipLaunchKernelGGL(kfn, dim3(ntiles), dim3(RS_BLOCK), 0, cur_stream(),
                     kin, vin, n, shift, ntiles, base, kout, vout);
}

u64* u64p(torch::Tensor& t) { return reinterpret_cast<u64*>(t.data_ptr<i64>()); }
const u64* u64cp(const torch::Tensor& t) {
  return reinterpret_cast<const u64*>(t.data_ptr<i64>());
}

void check_dev_i64(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.scalar_type() == torch::kInt64, name, " must be int64");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

unsigned long long* ullp(torch::Tensor& t) {
  return reinterpret_cast<unsigned long long*>(t.data_ptr<i64>());
}

// GPOS side buffer: the block caches' exemplar positions live in global
// memory instead of LDS (written once per distinct word per block).  One
// persistent buffer per device, grown to the largest request; a kernel only
// reads what it wrote itself, so launches share it.
u64* tok_cpos_buffer(const torch::Device& dev, long entries) {
  static std::map<int, torch::Tensor> bufs;
  torch::Tensor& b = bufs[dev.index()];
  if (!b.defined() || b.numel() < entries)
    b = torch::empty({entries},
                     torch::TensorOptions().device(dev).dtype(torch::kInt64));
  return u64p(b);
}

// What a v6 / v7 launch takes besides its grid.
struct TokArgs {
  torch::Tensor text;
  long pos_base;
  u64* tkeys;  // global table (spill-all passes a dummy)
  i64* tvals;
  u64* texm;
  u64 cap_mask;
  u64* out_hash;  // spill stream
  u64* out_pos;
  unsigned long long* counter;
  long spill_cap;
  unsigned long long* nwords;
  const i64* split_off = nullptr;  // COMPOSITE only
  int nsplit_off = 0;
  long doc_base = 0;
};

// The one place that picks the tokenizer body (tok_v6_forced) for a set of
// template arguments and launches it.
template <int CACHE_N, bool GPOS, bool SPILL_ALL = false,
          bool COMPOSITE = false, int SCHUNK = 512>
struct Tok {
  static auto kernel() {
    auto kfn = tokenize_v7_kernel<CACHE_N, GPOS, SPILL_ALL, COMPOSITE, SCHUNK>;
    if (tok_v6_forced())
      kfn = tokenize_v6_kernel<CACHE_N, GPOS, SPILL_ALL, COMPOSITE, SCHUNK>;
    return kfn;
  }

  static void launch(long blocks, TokArgs a) {
    g_tok_last_body = tok_v6_forced() ? "v6" : "v7";
    u64* cpos =
        GPOS ? tok_cpos_buffer(a.text.device(), blocks * CACHE_N) : nullptr;
    auto kfn = kernel();
    hipLaunchKernelGGL(kfn, dim3(blocks), dim3(kBlock), 0, cur_stream(),
                       a.text.data_ptr<u8>(), (long)a.text.numel(),
                       (u64)a.pos_base, a.tkeys, a.tvals, a.texm, a.cap_mask,
                       a.out_hash, a.out_pos, a.counter, a.spill_cap,
                       a.nwords, cpos, a.split_off, a.nsplit_off, a.doc_base);
  }
};

}  // namespace

// ---------------------------------------------------------------------- K2/K3
std::vector<torch::Tensor> tokenize(torch::Tensor text, long cap) {
  TORCH_CHECK(text.is_cuda() && text.scalar_type() == torch::kUInt8 &&
              text.is_contiguous(), "text must be contiguous u8 on GPU");
  long n = text.numel();
  auto opts = torch::TensorOptions().device(text.device()).dtype(torch::kInt64);
  auto out_hash = torch::empty({cap}, opts);
  auto out_pos = torch::empty({cap}, opts);
  auto counter = torch::zeros({1}, opts);
  long blocks = grid_for(n, TOK_BYTES);
  hipLaunchKernelGGL(tokenize_kernel, dim3(blocks), dim3(kBlock), 0,
                     cur_stream(), text.data_ptr<u8>(), n, u64p(out_hash),
                     u64p(out_pos),
                     reinterpret_cast<unsigned long long*>(counter.data_ptr<i64>()),
                     cap);
  return {out_hash, out_pos, counter};
}

// ------------------------------------------------------------------ K2+K5
void tokenize_count(torch::Tensor text, long pos_base, torch::Tensor tkeys,
                    torch::Tensor tvals, torch::Tensor texm,
                    torch::Tensor nwords) {
  TORCH_CHECK(text.is_cuda() && text.scalar_type() == torch::kUInt8 &&
              text.is_contiguous(), "text must be contiguous u8 on GPU");
  long n = text.numel();
  long cap = tkeys.numel();
  TORCH_CHECK((cap & (cap - 1)) == 0, "table capacity must be a power of 2");
  if (!n) return;
  hipLaunchKernelGGL(tokenize_count_kernel, dim3(grid_for(n, TOK_BYTES)),
                     dim3(kBlock), 0, cur_stream(), text.data_ptr<u8>(), n,
                     (u64)pos_base, u64p(tkeys), tvals.data_ptr<i64>(),
                     texm.numel() ? u64p(texm) : nullptr, (u64)(cap - 1),
                     reinterpret_cast<unsigned long long*>(nwords.data_ptr<i64>()));
}

// ------------------------------------------------------ K2 streaming (v2)
// every word spilled via the wave-chunked allocator (no cache) — chunk
// tails are HT_EMPTY-padded, so consumers must filter/skip them.  The
// inverted-index tokenize path.
std::vector<torch::Tensor> tokenize_spill_v2(torch::Tensor text,
                                             long pos_base, long cap,
                                             long max_blocks) {
  TORCH_CHECK(text.is_cuda() && text.scalar_type() == torch::kUInt8 &&
              text.is_contiguous(), "text must be contiguous u8 on GPU");
  long n = text.numel();
  auto opts = torch::TensorOptions().device(text.device()).dtype(torch::kInt64);
  auto out_hash = torch::empty({cap}, opts);
  auto out_pos = torch::empty({cap}, opts);
  auto counter = torch::zeros({1}, opts);
  auto nwords = torch::zeros({1}, opts);
  if (n) {
    auto dummy = torch::empty({16}, opts);  // table unused in SPILL_ALL
    // SCHUNK stays 512 for SPILL_ALL: every word spills (~6000/wave), so
    // 512 already amortizes reservations per-entry; 2048 quadruples the
    // padded chunk tails flowing through radix+bucket (measured 12.4 vs
    // 9.9 ms on the inverted-index job)
    // spill-all keeps the kMaxBlocks-capped grid: it has no per-block
    // cache to warm or flush, and the inverted index measured 8.05-8.08
    // ms/job on the one-round grid vs 8.03-8.06 on this one (parent
    // 8.02-8.07; profiles/tokenizer_occupancy_r04.md)
    Tok<16, false, true>::launch(
        tok_cap_blocks(grid_for(n, TOK_BYTES), max_blocks),
        {text, pos_base, u64p(dummy), dummy.data_ptr<i64>(), nullptr, (u64)15,
         u64p(out_hash), u64p(out_pos), ullp(counter), cap, ullp(nwords)});
  }
  return {out_hash, out_pos, counter, nwords};
}

std::vector<torch::Tensor> tokenize_spill_composite(
    torch::Tensor text, long pos_base, long cap, torch::Tensor split_off,
    long doc_base, long max_blocks) {
  TORCH_CHECK(text.is_cuda() && text.scalar_type() == torch::kUInt8 &&
              text.is_contiguous(), "text must be contiguous u8 on GPU");
  check_dev_i64(split_off, "split_off");
  long n = text.numel();
  auto opts = torch::TensorOptions().device(text.device()).dtype(torch::kInt64);
  auto out_hash = torch::empty({cap}, opts);
  auto out_pos = torch::empty({cap}, opts);
  auto counter = torch::zeros({1}, opts);
  auto nwords = torch::zeros({1}, opts);
  if (n) {
    auto dummy = torch::empty({16}, opts);
    Tok<16, false, true, true>::launch(
        tok_cap_blocks(grid_for(n, TOK_BYTES), max_blocks),
        {text, pos_base, u64p(dummy), dummy.data_ptr<i64>(), nullptr, (u64)15,
         u64p(out_hash), u64p(out_pos), ullp(counter), cap, ullp(nwords),
         split_off.data_ptr<i64>(), (int)split_off.numel(), doc_base});
  }
  return {out_hash, out_pos, counter, nwords};
}

// Cached composite tokenizer: the LDS cache absorbs the Zipf head of
// (word, doc) composite keys too — a block's ~124 KB tile span stays
// inside one ~1.3 MB document, so composite keys inherit the word
// head's temporal locality.  Cuts the spill from every word (~49M) to
// cache misses (~15M), shrinking the radix bucketize + bucket_count
// drain ~3x (the spill-all path's two largest costs after tokenize).
void tokenize_cache_spill_composite(
    torch::Tensor text, long pos_base, torch::Tensor tkeys,
    torch::Tensor tvals, torch::Tensor texm, long spill_cap,
    torch::Tensor nwords, torch::Tensor out_hash, torch::Tensor out_pos,
    torch::Tensor counter, torch::Tensor split_off, long doc_base,
    long max_blocks) {
  TORCH_CHECK(text.is_cuda() && text.scalar_type() == torch::kUInt8 &&
              text.is_contiguous(), "text must be contiguous u8 on GPU");
  check_dev_i64(split_off, "split_off");
  long n = text.numel();
  long cap = tkeys.numel();
  TORCH_CHECK((cap & (cap - 1)) == 0, "table capacity must be a power of 2");
  TORCH_CHECK(out_hash.numel() >= spill_cap && out_pos.numel() >= spill_cap,
              "spill arrays too small");
  if (!n) return;
  using T = Tok<2048, true, false, true, 2048>;
  T::launch(
      tok_cap_blocks(tok_grid(T::kernel(), kBlock, n, 4096), max_blocks),
      {text, pos_base, u64p(tkeys), tvals.data_ptr<i64>(),
       texm.numel() ? u64p(texm) : nullptr, (u64)(cap - 1), u64p(out_hash),
       u64p(out_pos), ullp(counter), spill_cap, ullp(nwords),
       split_off.data_ptr<i64>(), (int)split_off.numel(), doc_base});
}

// ---------------------------------------------------------------- K2+K5
// Word count: the LDS cache counts the Zipf head, misses spill.  The out
// arrays + counter are caller-owned so several map-job launches can append
// into ONE spill stream (atomic counter composes across launches).
//
// The shape is fixed at what the sweeps chose (ms/step on the bench shape):
// 2048 cache slots per block (512 = 5.52, 1024 = 5.26, 2048 = 4.94 — fewer
// spills beat occupancy here) and, with GPOS, 2048-entry spill chunks:
// reservation-stall amortization vs HT_EMPTY pad waste measured 128 = 3.86,
// 512 = 1.93, 1024 = 1.92, 2048 = 1.84, 4096 = 3.09 over ~15M real misses
// and 8192 waves — one grab per wave is the sweet spot; 4096 doubles the
// reserved entries (19M pads flood the radix+bucket pipeline at ~75 ns
// each).  An 8 KB tile and 512-thread blocks measured slower.
// MR_TOK_GPOS=0 keeps the exemplar positions in LDS (default on: 4.90 vs
// 5.05 ms); that shape keeps its 512-entry chunks.
void tokenize_cache_spill(
    torch::Tensor text, long pos_base, torch::Tensor tkeys,
    torch::Tensor tvals, torch::Tensor texm, long spill_cap,
    torch::Tensor nwords, torch::Tensor out_hash, torch::Tensor out_pos,
    torch::Tensor counter, long max_blocks) {
  TORCH_CHECK(text.is_cuda() && text.scalar_type() == torch::kUInt8 &&
              text.is_contiguous(), "text must be contiguous u8 on GPU");
  long n = text.numel();
  long cap = tkeys.numel();
  TORCH_CHECK((cap & (cap - 1)) == 0, "table capacity must be a power of 2");
  TORCH_CHECK(out_hash.numel() >= spill_cap && out_pos.numel() >= spill_cap,
              "spill arrays too small");
  if (!n) return;
  const char* gp = getenv("MR_TOK_GPOS");
  bool gpos = !(gp && gp[0] == '0');
  TokArgs a{text, pos_base, u64p(tkeys), tvals.data_ptr<i64>(),
            texm.numel() ? u64p(texm) : nullptr, (u64)(cap - 1),
            u64p(out_hash), u64p(out_pos), ullp(counter), spill_cap,
            ullp(nwords)};
  if (gpos) {
    using T = Tok<2048, true, false, false, 2048>;
    T::launch(
        tok_cap_blocks(tok_grid(T::kernel(), kBlock, n, 4096), max_blocks), a);
  } else {
    using T = Tok<2048, false>;
    T::launch(
        tok_cap_blocks(tok_grid(T::kernel(), kBlock, n, 4096), max_blocks), a);
  }
}

// ---------------------------------------------------------- K5 bucket count
void bucket_count(torch::Tensor hashes, torch::Tensor pos,
                  torch::Tensor bucket_off, long nbuckets, long slices,
                  torch::Tensor tkeys, torch::Tensor tvals,
                  torch::Tensor texm, long region_stride, long slots_arg) {
  check_dev_i64(hashes, "hashes");
  check_dev_i64(pos, "pos");
  check_dev_i64(bucket_off, "bucket_off");
  check_dev_i64(tkeys, "tkeys");
  check_dev_i64(tvals, "tvals");
  if (texm.numel()) check_dev_i64(texm, "texm");
  TORCH_CHECK(pos.numel() >= hashes.numel(),
              "pos must hold one entry per hash");
  TORCH_CHECK(nbuckets >= 1 && slices >= 1, "nbuckets and slices >= 1");
  TORCH_CHECK(nbuckets * slices < (1L << 31), "nbuckets * slices too large");
  long cap = tkeys.numel();
  TORCH_CHECK(cap > 0 && (cap & (cap - 1)) == 0,
              "table capacity must be a power of 2");
  TORCH_CHECK(tvals.numel() == cap &&
                  (texm.numel() == 0 || texm.numel() == cap),
              "tvals (and texm, when tracked) must match tkeys");
  // region_stride > 0: bucket_off holds per-bucket LENGTHS and bucket b's
  // data lives at [b*stride, b*stride+len[b]) (fixed-stride regions)
  TORCH_CHECK(bucket_off.numel() >= (region_stride > 0 ? nbuckets
                                                       : nbuckets + 1),
              "bucket_off size");
  TORCH_CHECK(region_stride <= 0 ||
                  hashes.numel() >= nbuckets * region_stride,
              "hashes must hold nbuckets regions of region_stride entries");
  // slots: caller picks (1024 = 8 blocks/CU is now the winner for BOTH
  // wordcount and the inverted index — r2 joint sweep showed slots and
  // slices interact: smaller tables buy occupancy that more slices
  // convert into block-level parallelism; overflow falls back to
  // per-element ht_add, never wrong); MR_BKT_SLOTS env overrides for A/B
  const char* bs = getenv("MR_BKT_SLOTS");
  int slots = bs ? atoi(bs) : (int)slots_arg;
  if (slots != 512 && slots != 1024 && slots != 2048) slots = 2048;
  // MR_BKT_ILP ∈ {1, 2, 4}: independent probe chains per thread (the
  // kernel is latency-bound at full occupancy — see kernel comment)
  const char* bi = getenv("MR_BKT_ILP");
  int ilp = bi ? atoi(bi) : 1;
  auto kfn = bucket_count_kernel<2048, 1>;
  if (ilp == 4) {
    kfn = bucket_count_kernel<2048, 4>;
    if (slots == 1024) kfn = bucket_count_kernel<1024, 4>;
    else if (slots == 512) kfn = bucket_count_kernel<512, 4>;
  } else if (ilp == 2) {
    kfn = bucket_count_kernel<2048, 2>;
    if (slots == 1024) kfn = bucket_count_kernel<1024, 2>;
    else if (slots == 512) kfn = bucket_count_kernel<512, 2>;
  } else {
    if (slots == 1024) kfn = bucket_count_kernel<1024, 1>;
    else if (slots == 512) kfn = bucket_count_kernel<512, 1>;
  }
  hipLaunchKernelGGL(kfn, dim3(nbuckets * slices),
                     dim3(kBlock), 0, cur_stream(), u64cp(hashes),
                     u64cp(pos), bucket_off.data_ptr<i64>(), (int)nbuckets,
                     (int)slices, u64p(tkeys), tvals.data_ptr<i64>(),
                     texm.numel() ? u64p(texm) : nullptr, (u64)(cap - 1),
                     region_stride);
}

// ----------------------------------------------------------------------- K5a
void hash_insert_count(torch::Tensor keys, torch::Tensor pos,
                       torch::Tensor tkeys, torch::Tensor tvals,
                       torch::Tensor texm, long n) {
  check_dev_i64(keys, "keys");
  long cap = tkeys.numel();
  TORCH_CHECK((cap & (cap - 1)) == 0, "table capacity must be a power of 2");
  hipLaunchKernelGGL(hash_insert_count_kernel, dim3(grid_for(n)), dim3(kBlock),
                     0, cur_stream(), u64cp(keys),
                     pos.numel() ? u64cp(pos) : nullptr, n, u64p(tkeys),
                     tvals.data_ptr<i64>(),
                     texm.numel() ? u64p(texm) : nullptr, (u64)(cap - 1));
}

void hash_insert_sum_i64(torch::Tensor keys, torch::Tensor vals,
                         torch::Tensor tkeys, torch::Tensor tvals, long n) {
  check_dev_i64(keys, "keys");
  long cap = tkeys.numel();
  TORCH_CHECK((cap & (cap - 1)) == 0, "table capacity must be a power of 2");
  hipLaunchKernelGGL(hash_insert_sum_i64_kernel, dim3(grid_for(n)),
                     dim3(kBlock), 0, cur_stream(), u64cp(keys),
                     vals.data_ptr<i64>(), n, u64p(tkeys),
                     tvals.data_ptr<i64>(), (u64)(cap - 1));
}

std::vector<torch::Tensor> hash_extract(torch::Tensor tkeys,
                                        torch::Tensor tvals,
                                        torch::Tensor texm) {
  long cap = tkeys.numel();
  auto opts = tkeys.options();
  auto okeys = torch::empty({cap}, opts);
  auto ovals = torch::empty({cap}, opts);
  bool exm = texm.numel() > 0;
  auto opos = torch::empty({exm ? cap : 0}, opts);
  auto counter = torch::zeros({1}, opts);
  hipLaunchKernelGGL(hash_extract_kernel, dim3(grid_for(cap)), dim3(kBlock), 0,
                     cur_stream(), u64cp(tkeys), tvals.data_ptr<i64>(),
                     exm ? u64cp(texm) : nullptr, cap, u64p(okeys),
                     ovals.data_ptr<i64>(), exm ? u64p(opos) : nullptr,
                     reinterpret_cast<unsigned long long*>(counter.data_ptr<i64>()));
  return {okeys, ovals, opos, counter};
}

std::vector<torch::Tensor> hash_extract_v2(torch::Tensor tkeys,
                                           torch::Tensor tvals,
                                           torch::Tensor texm) {
  long cap = tkeys.numel();
  auto opts = tkeys.options();
  long waves = (2048L * kBlock) / 64;
  long ocap = cap + waves * 256;  // chunk-tail padding slack
  auto okeys = torch::empty({ocap}, opts);
  auto ovals = torch::empty({ocap}, opts);
  bool exm = texm.numel() > 0;
  auto opos = torch::empty({exm ? ocap : 0}, opts);
  auto counter = torch::zeros({1}, opts);
  hipLaunchKernelGGL(hash_extract_v2_kernel, dim3(2048), dim3(kBlock), 0,
                     cur_stream(), u64cp(tkeys), tvals.data_ptr<i64>(),
                     exm ? u64cp(texm) : nullptr, cap, u64p(okeys),
                     ovals.data_ptr<i64>(), exm ? u64p(opos) : nullptr,
                     reinterpret_cast<unsigned long long*>(counter.data_ptr<i64>()),
                     ocap);
  return {okeys, ovals, opos, counter};
}

// Table -> (packed [keys | counts | lens] at stride n in a 3 * cap buffer,
// pos, offs, meta = [n, total_bytes, overflow] on the HOST), keys ascending
// in u64 order.  Seven launches (one zero fill + six kernels; five without
// exemplars) and one readback, the meta copy, which is the op's only sync.
// overflow != 0: some bin outgrew the rank kernel's LDS and its keys were
// not written — the caller must take the general path instead.
std::vector<torch::Tensor> extract_sorted(torch::Tensor tkeys,
                                          torch::Tensor tvals,
                                          torch::Tensor texm) {
  check_dev_i64(tkeys, "tkeys");
  check_dev_i64(tvals, "tvals");
  if (texm.numel()) check_dev_i64(texm, "texm");
  long cap = tkeys.numel();
  TORCH_CHECK(cap > 0 && (cap & (cap - 1)) == 0,
              "table capacity must be a power of 2");
  TORCH_CHECK(cap < (1L << 31), "extract_sorted slots are u32: cap < 2^31");
  TORCH_CHECK(tvals.numel() == cap &&
                  (texm.numel() == 0 || texm.numel() == cap),
              "tvals (and texm, when tracked) must match tkeys");
  bool exm = texm.numel() > 0;
  auto opts = tkeys.options();
  auto o32 = opts.dtype(torch::kInt32);
  long nbins = cap / XS_SLOTS_PER_BIN;
  if (nbins < 1) nbins = 1;
  int shift = 64;
  for (long b = nbins; b > 1; b >>= 1) --shift;
  long ntiles = (cap + XS_SCAN_TILE - 1) / XS_SCAN_TILE;
  auto packed = torch::empty({3 * cap}, opts);
  auto pos = torch::empty({exm ? cap : 0}, opts);
  auto offs = torch::empty({exm ? cap : 0}, opts);
  auto meta = torch::empty({3}, opts);
  auto bins = torch::zeros({nbins}, o32);
  auto bin_off = torch::empty({nbins + 1}, o32);
  auto bkeys = torch::empty({cap}, opts);
  auto bslot = torch::empty({cap}, o32);
  auto tile_sums = torch::empty({ntiles}, opts);
  u32* binp = reinterpret_cast<u32*>(bins.data_ptr<int>());
  u32* offp = reinterpret_cast<u32*>(bin_off.data_ptr<int>());
  u32* slotp = reinterpret_cast<u32*>(bslot.data_ptr<int>());
  hipStream_t st = cur_stream();
  hipLaunchKernelGGL(xs_hist_kernel, dim3(grid_for(cap)), dim3(XS_BLOCK), 0,
                     st, u64cp(tkeys), cap, shift, binp);
  hipLaunchKernelGGL(xs_bin_scan_kernel, dim3(1), dim3(XS_BINSCAN_BLOCK), 0,
                     st, binp, (int)nbins, offp, meta.data_ptr<i64>());
  hipLaunchKernelGGL(xs_scatter_kernel, dim3(grid_for(cap)), dim3(XS_BLOCK),
                     0, st, u64cp(tkeys), cap, shift, binp, offp,
                     u64p(bkeys), slotp);
  hipLaunchKernelGGL(xs_rank_kernel,
                     dim3((nbins + XS_WAVES - 1) / XS_WAVES), dim3(XS_BLOCK),
                     0, st, u64cp(bkeys), slotp, offp, (int)nbins,
                     tvals.data_ptr<i64>(), exm ? u64cp(texm) : nullptr,
                     meta.data_ptr<i64>(), packed.data_ptr<i64>(),
                     exm ? u64p(pos) : nullptr);
  if (exm) {
    hipLaunchKernelGGL(xs_tile_sums_kernel, dim3(ntiles), dim3(XS_BLOCK), 0,
                       st, packed.data_ptr<i64>(), meta.data_ptr<i64>(),
                       tile_sums.data_ptr<i64>());
    hipLaunchKernelGGL(xs_offs_scan_kernel, dim3(ntiles), dim3(XS_BLOCK), 0,
                       st, packed.data_ptr<i64>(), meta.data_ptr<i64>(),
                       tile_sums.data_ptr<i64>(), offs.data_ptr<i64>());
  }
  return {packed, pos, offs, meta.cpu()};
}

std::vector<long> extract_sorted_caps() { return {XS_RANK_M, XS_SCAN_TILE}; }

// ----------------------------------------------------------------------- K5b
torch::Tensor head_flags(torch::Tensor keys) {
  check_dev_i64(keys, "keys");
  long n = keys.numel();
  auto flags = torch::empty({n}, keys.options());
  if (n)
    hipLaunchKernelGGL(head_flags_kernel, dim3(grid_for(n)), dim3(kBlock), 0,
                       cur_stream(), u64cp(keys), n, flags.data_ptr<i64>());
  return flags;
}

std::vector<torch::Tensor> seg_reduce_i64(torch::Tensor keys,
                                          torch::Tensor vals,
                                          torch::Tensor seg, long nseg) {
  check_dev_i64(keys, "keys");
  long n = keys.numel();
  auto okeys = torch::empty({nseg}, keys.options());
  auto ovals = torch::zeros({nseg}, keys.options());
  if (n)
    hipLaunchKernelGGL(seg_scatter_i64_kernel, dim3(grid_for(n)), dim3(kBlock),
                       0, cur_stream(), u64cp(keys),
                       vals.numel() ? vals.data_ptr<i64>() : nullptr,
                       seg.data_ptr<i64>(), n, u64p(okeys),
                       ovals.data_ptr<i64>());
  return {okeys, ovals};
}

std::vector<torch::Tensor> seg_reduce_i64_minmax(torch::Tensor keys,
                                                 torch::Tensor vals,
                                                 torch::Tensor seg, long nseg,
                                                 bool is_min) {
  check_dev_i64(keys, "keys");
  long n = keys.numel();
  auto okeys = torch::empty({nseg}, keys.options());
  auto ovals = torch::full({nseg},
                           is_min ? std::numeric_limits<i64>::max()
                                  : std::numeric_limits<i64>::min(),
                           keys.options());
  if (n) {
    if (is_min)
      hipLaunchKernelGGL(seg_scatter_i64_minmax_kernel<true>,
                         dim3(grid_for(n)), dim3(kBlock), 0, cur_stream(),
                         u64cp(keys), vals.data_ptr<i64>(),
                         seg.data_ptr<i64>(), n, u64p(okeys),
                         ovals.data_ptr<i64>());
    else
      hipLaunchKernelGGL(seg_scatter_i64_minmax_kernel<false>,
                         dim3(grid_for(n)), dim3(kBlock), 0, cur_stream(),
                         u64cp(keys), vals.data_ptr<i64>(),
                         seg.data_ptr<i64>(), n, u64p(okeys),
                         ovals.data_ptr<i64>());
  }
  return {okeys, ovals};
}

std::vector<torch::Tensor> seg_reduce_f64_minmax(torch::Tensor keys,
                                                 torch::Tensor vals,
                                                 torch::Tensor seg, long nseg,
                                                 bool is_min) {
  check_dev_i64(keys, "keys");
  long n = keys.numel();
  auto okeys = torch::empty({nseg}, keys.options());
  auto ovals = torch::full({nseg},
                           is_min ? std::numeric_limits<double>::infinity()
                                  : -std::numeric_limits<double>::infinity(),
                           vals.options());
  if (n) {
    if (is_min)
      hipLaunchKernelGGL(seg_scatter_f64_minmax_kernel<true>,
                         dim3(grid_for(n)), dim3(kBlock), 0, cur_stream(),
                         u64cp(keys), vals.data_ptr<double>(),
                         seg.data_ptr<i64>(), n, u64p(okeys),
                         ovals.data_ptr<double>());
    else
      hipLaunchKernelGGL(seg_scatter_f64_minmax_kernel<false>,
                         dim3(grid_for(n)), dim3(kBlock), 0, cur_stream(),
                         u64cp(keys), vals.data_ptr<double>(),
                         seg.data_ptr<i64>(), n, u64p(okeys),
                         ovals.data_ptr<double>());
  }
  return {okeys, ovals};
}

torch::Tensor seg_first_u64(torch::Tensor aux, torch::Tensor seg, long nseg) {
  long n = aux.numel();
  auto oaux = torch::zeros({nseg}, aux.options());
  if (n)
    hipLaunchKernelGGL(seg_first_u64_kernel, dim3(grid_for(n)), dim3(kBlock),
                       0, cur_stream(), u64cp(aux), seg.data_ptr<i64>(), n,
                       u64p(oaux));
  return oaux;
}

std::vector<torch::Tensor> seg_reduce_f64(torch::Tensor keys,
                                          torch::Tensor vals,
                                          torch::Tensor seg, long nseg) {
  check_dev_i64(keys, "keys");
  long n = keys.numel();
  auto okeys = torch::empty({nseg}, keys.options());
  auto ovals = torch::zeros({nseg}, vals.options());
  if (n)
    hipLaunchKernelGGL(seg_scatter_f64_kernel, dim3(grid_for(n)), dim3(kBlock),
                       0, cur_stream(), u64cp(keys), vals.data_ptr<double>(),
                       seg.data_ptr<i64>(), n, u64p(okeys),
                       ovals.data_ptr<double>());
  return {okeys, ovals};
}

// ------------------------------------------------------------------------ K2
torch::Tensor partition_hist(torch::Tensor keys, long nparts) {
  check_dev_i64(keys, "keys");
  TORCH_CHECK(nparts <= MAX_PARTS, "nparts too large");
  long n = keys.numel();
  auto hist = torch::zeros({nparts}, keys.options());
  if (n)
    hipLaunchKernelGGL(partition_hist_kernel, dim3(grid_for(n)), dim3(kBlock),
                       0, cur_stream(), u64cp(keys), n, (u32)nparts,
                       hist.data_ptr<i64>());
  return hist;
}

// --------------------------------------------------------------------- K7/K8
torch::Tensor pos_len(torch::Tensor pos) {
  long n = pos.numel();
  auto lens = torch::empty({n}, pos.options());
  if (n)
    hipLaunchKernelGGL(pos_len_kernel, dim3(grid_for(n)), dim3(kBlock), 0,
                       cur_stream(), u64cp(pos), n, lens.data_ptr<i64>());
  return lens;
}

torch::Tensor gather_bytes(torch::Tensor text, torch::Tensor pos,
                           torch::Tensor out_off, long total) {
  long n = pos.numel();
  auto out = torch::zeros({total},
                          torch::TensorOptions().device(text.device())
                              .dtype(torch::kUInt8));
  if (n)
    hipLaunchKernelGGL(gather_bytes_kernel, dim3(grid_for(n)), dim3(kBlock), 0,
                       cur_stream(), text.data_ptr<u8>(), u64cp(pos),
                       out_off.data_ptr<i64>(), n, out.data_ptr<u8>());
  return out;
}

// ------------------------------------------------------------------------ K6
torch::Tensor grad_colsum(torch::Tensor grads, bool use_mfma) {
  TORCH_CHECK(grads.is_cuda() && grads.dim() == 2 &&
              grads.scalar_type() == torch::kFloat32 && grads.is_contiguous(),
              "grads must be contiguous f32 [G, D] on GPU");
  long G = grads.size(0), D = grads.size(1);
  auto out = torch::empty({D}, grads.options());
  if (use_mfma) {
    long ntiles = (D + 15) / 16;
    long blocks = ntiles < 4096 ? (ntiles ? ntiles : 1) : 4096;
    hipLaunchKernelGGL(colsum_f32_mfma_kernel, dim3(blocks), dim3(64), 0,
                       cur_stream(), grads.data_ptr<float>(), G, D,
                       out.data_ptr<float>());
  } else {
    hipLaunchKernelGGL(colsum_f32_valu_kernel, dim3(grid_for(D, 4)),
                       dim3(kBlock), 0, cur_stream(),
                       grads.data_ptr<float>(), G, D, out.data_ptr<float>());
  }
  return out;
}

// ------------------------------------------------------------------------ K1
// single partition pass on one 8-bit digit; returns (keys, vals, per-digit
// totals) — used to bucketize by top byte before LDS counting
std::vector<torch::Tensor> radix_pass(torch::Tensor keys, torch::Tensor vals,
                                      long shift) {
  check_dev_i64(keys, "keys");
  long n = keys.numel();
  bool has_vals = vals.numel() > 0;
  auto opts = keys.options();
  long ntiles = (n + rs_tile() - 1) / rs_tile();
  if (ntiles == 0) ntiles = 1;
  auto kout = torch::empty({n}, opts);
  auto vout = has_vals ? torch::empty({n}, opts) : torch::empty({0}, opts);
  auto hist = torch::zeros({(long)RS_BINS * ntiles}, opts);
  if (n) {
    launch_radix_hist(u64cp(keys), n, (int)shift, ntiles,
                      hist.data_ptr<i64>());
    auto scanned = torch::cumsum(hist, 0);
    auto base = scanned - hist;
    launch_radix_scatter(u64cp(keys), has_vals ? u64cp(vals) : nullptr, n,
                         (int)shift, ntiles, base.data_ptr<i64>(),
                         u64p(kout), has_vals ? u64p(vout) : nullptr);
  }
  auto totals = hist.view({(long)RS_BINS, ntiles}).sum(1);
  return {kout, vout, totals};
}

// The spill drain's bucketize: one partition pass on an 8-bit digit with
// the scan done natively (u32 histogram -> rs_row_totals + rs_row_scan,
// no ATen glue, no zero fill).  vals: int64 or int32 payload, or empty.
// Returns (keys_out, vals_out, bucket_off[257]); outputs keep length n and
// the first bucket_off[256] entries are defined.  skip_empty (default
// off; spill drains only) drops HT_EMPTY-keyed records, so bucket_off
// counts survivors; off, all-ones keys are ordinary data.  No host sync.
// The direct-scatter A/B kernel (MR_RADIX_V1=1) has no skip predicate
// and no u32 base, so this entry point refuses to run with it.
std::vector<torch::Tensor> radix_bucketize(torch::Tensor keys,
                                           torch::Tensor vals, long shift,
                                           bool skip_empty) {
  check_dev_i64(keys, "keys");
  long n = keys.numel();
  bool has_vals = vals.numel() > 0;
  bool v32 = has_vals && vals.scalar_type() == torch::kInt32;
  if (has_vals) {
    TORCH_CHECK(vals.is_cuda() && vals.is_contiguous() && vals.numel() == n,
                "vals must be contiguous on GPU, one per key");
    TORCH_CHECK(v32 || vals.scalar_type() == torch::kInt64,
                "vals must be int64 or int32");
  }
  TORCH_CHECK(shift >= 0 && shift <= 56, "shift in [0,56]");
  TORCH_CHECK(n < (1L << 32), "bucketize positions are u32: n < 2^32");
  TORCH_CHECK(!radix_v1_forced(),
              "radix_bucketize has no direct-scatter (MR_RADIX_V1=1) form");
  auto opts = keys.options();
  auto kout = torch::empty({n}, opts);
  auto vout = has_vals ? torch::empty({n}, vals.options())
                       : torch::empty({0}, opts);
  if (n == 0) return {kout, vout, torch::zeros({RS_BINS + 1}, opts)};
  long ntiles = (n + rs_tile() - 1) / rs_tile();
  auto bucket_off = torch::empty({RS_BINS + 1}, opts);
  auto totals = torch::empty({RS_BINS}, opts);
  auto hist = torch::empty({(long)RS_BINS * ntiles}, opts.dtype(torch::kInt32));
  u32* hp = reinterpret_cast<u32*>(hist.data_ptr<int>());
  int sh = (int)shift;
  if (skip_empty) launch_bucketize_hist<true>(u64cp(keys), n, sh, ntiles, hp);
  else launch_bucketize_hist<false>(u64cp(keys), n, sh, ntiles, hp);
  hipLaunchKernelGGL(rs_row_totals_kernel, dim3(RS_BINS), dim3(RS_BLOCK), 0,
                     cur_stream(), hp, ntiles, totals.data_ptr<i64>());
  hipLaunchKernelGGL(rs_row_scan_kernel, dim3(RS_BINS), dim3(RS_BLOCK), 0,
                     cur_stream(), hp, ntiles, totals.data_ptr<i64>(),
                     bucket_off.data_ptr<i64>());
  if (v32) {
    const u32* vi = reinterpret_cast<const u32*>(vals.data_ptr<int>());
    u32* vo = reinterpret_cast<u32*>(vout.data_ptr<int>());
    if (skip_empty)
      launch_bucketize_scatter<u32, true>(u64cp(keys), vi, n, sh, ntiles, hp,
                                          u64p(kout), vo);
    else
      launch_bucketize_scatter<u32, false>(u64cp(keys), vi, n, sh, ntiles,
                                           hp, u64p(kout), vo);
  } else {
    const u64* vi = has_vals ? u64cp(vals) : nullptr;
    u64* vo = has_vals ? u64p(vout) : nullptr;
    if (skip_empty)
      launch_bucketize_scatter<u64, true>(u64cp(keys), vi, n, sh, ntiles, hp,
                                          u64p(kout), vo);
    else
      launch_bucketize_scatter<u64, false>(u64cp(keys), vi, n, sh, ntiles,
                                           hp, u64p(kout), vo);
  }
  return {kout, vout, bucket_off};
}

// what this process's sorts run: (records per tile, 1 if the direct-scatter
// kernel of MR_RADIX_V1=1 is selected else 0) — both are fixed at first use
std::vector<long> radix_sort_caps() {
  return {rs_tile(), radix_v1_forced() ? 1L : 0L};
}

std::vector<torch::Tensor> radix_sort_pairs(torch::Tensor keys,
                                            torch::Tensor vals, int bits) {
  check_dev_i64(keys, "keys");
  long n = keys.numel();
  bool has_vals = vals.numel() > 0;
  if (has_vals) {
    TORCH_CHECK(vals.is_cuda() && vals.is_contiguous() && vals.numel() == n,
                "vals must be contiguous on GPU, one per key");
    TORCH_CHECK(vals.scalar_type() == torch::kInt64, "vals must be int64");
    TORCH_CHECK(vals.device() == keys.device(),
                "vals must be on the keys' device");
  }
  if (n == 0) return {keys, vals};
  TORCH_CHECK(bits >= 1 && bits <= 64, "bits in [1,64]");
  int passes = (bits + 7) / 8;
  long ntiles = (n + rs_tile() - 1) / rs_tile();
  auto opts = keys.options();
  auto kbuf = torch::empty({n}, opts);
  auto vbuf = has_vals ? torch::empty({n}, opts) : torch::empty({0}, opts);
  auto hist = torch::empty({(long)RS_BINS * ntiles}, opts);

  // inputs are NEVER mutated: pass 0 reads the caller's tensors, then
  // the ping-pong runs over two scratch buffers (the old swap scheme
  // scattered back INTO the input from pass 1 — a caller reusing its
  // tensor after the sort read sorted data; caught by the idx32 tests)
  torch::Tensor kin = keys, vin = vals, kout = kbuf, vout = vbuf;
  for (int p = 0; p < passes; ++p) {
    int shift = p * 8;
    launch_radix_hist(u64cp(kin), n, shift, ntiles, hist.data_ptr<i64>());
    // exclusive scan over the digit-major flat histogram = base[d][t]
    auto scanned = torch::cumsum(hist, 0);
    auto base = scanned - hist;
    launch_radix_scatter(u64cp(kin), has_vals ? u64cp(vin) : nullptr, n,
                         shift, ntiles, base.data_ptr<i64>(), u64p(kout),
                         has_vals ? u64p(vout) : nullptr);
    if (p == 0 && passes > 1) {
      kin = kout;
      kout = torch::empty({n}, opts);
      if (has_vals) {
        vin = vout;
        vout = torch::empty({n}, opts);
      }
    } else {
      std::swap(kin, kout);
      if (has_vals) std::swap(vin, vout);
    }
  }
  return {kin, vin};
}

std::vector<torch::Tensor> radix_sort_idx32(torch::Tensor keys, int bits) {
  // Sort u64 keys carrying a 4-byte iota payload; returns
  // {sorted_keys, perm (Int32)}.  Per-pass traffic drops from 32 B/elem
  // (u64 payload) to 24 B — callers gather their real payloads ONCE
  // through perm (gather_by_u32) instead of through all 8 passes.
  check_dev_i64(keys, "keys");
  long n = keys.numel();
  TORCH_CHECK(n < (1L << 31), "idx32 sort needs n < 2^31");
  auto iopts =
      torch::TensorOptions().device(keys.device()).dtype(torch::kInt32);
  auto vin_t = torch::arange(n, iopts);
  if (n == 0) return {keys, vin_t};
  TORCH_CHECK(bits >= 1 && bits <= 64, "bits in [1,64]");
  int passes = (bits + 7) / 8;
  long ntiles = (n + rs_tile() - 1) / rs_tile();
  auto opts = keys.options();
  auto kbuf = torch::empty({n}, opts);
  auto vbuf = torch::empty({n}, iopts);
  auto hist = torch::empty({(long)RS_BINS * ntiles}, opts);
  // input keys are never mutated (see radix_sort_pairs); the iota
  // payload vin_t is ours, so only the key side needs the pass-0 fork
  torch::Tensor kin = keys, vin = vin_t, kout = kbuf, vout = vbuf;
  for (int p = 0; p < passes; ++p) {
    int shift = p * 8;
    launch_radix_hist(u64cp(kin), n, shift, ntiles, hist.data_ptr<i64>());
    auto scanned = torch::cumsum(hist, 0);
    auto base = scanned - hist;
    launch_radix_scatter32(
        u64cp(kin), reinterpret_cast<const u32*>(vin.data_ptr<int>()), n,
        shift, ntiles, base.data_ptr<i64>(), u64p(kout),
        reinterpret_cast<u32*>(vout.data_ptr<int>()));
    if (p == 0 && passes > 1) {
      kin = kout;
      kout = torch::empty({n}, opts);
      std::swap(vin, vout);
    } else {
      std::swap(kin, kout);
      std::swap(vin, vout);
    }
  }
  return {kin, vin};
}

torch::Tensor gather_by_u32(torch::Tensor vals, torch::Tensor idx) {
  // out[i] = vals[idx[i]] with a u32 index vector (one streaming pass)
  check_dev_i64(vals, "vals");
  TORCH_CHECK(idx.is_cuda() && idx.scalar_type() == torch::kInt32 &&
                  idx.is_contiguous(),
              "idx must be contiguous int32 on GPU");
  long n = idx.numel();
  auto out = torch::empty({n}, vals.options());
  if (n)
    hipLaunchKernelGGL(gather_i64_u32_kernel, dim3(grid_for(n)),
                       dim3(kBlock), 0, cur_stream(),
                       vals.data_ptr<i64>(),
                       reinterpret_cast<const u32*>(idx.data_ptr<int>()), n,
                       out.data_ptr<i64>());
  return out;
}

// ------------------------------------------------------- lexicographic order
namespace {
void check_text_u8(const torch::Tensor& text) {
  // a view with a storage offset is fine (the kernels align on the
  // absolute address); only unit stride is required
  TORCH_CHECK(text.is_cuda() && text.scalar_type() == torch::kUInt8 &&
              text.dim() == 1 && text.is_contiguous(),
              "text must be contiguous 1-D u8 on GPU");
}
}  // namespace

// keys[i] = big-endian chunk d of string idx[i] (idx empty: identity)
torch::Tensor lex_chunk_keys(torch::Tensor text, torch::Tensor pos,
                             torch::Tensor idx, long d) {
  check_text_u8(text);
  check_dev_i64(pos, "pos");
  bool has_idx = idx.numel() > 0;
  if (has_idx) check_dev_i64(idx, "idx");
  TORCH_CHECK(d >= 0 && d < 8192, "chunk index out of range");
  long m = has_idx ? idx.numel() : pos.numel();
  auto out = torch::empty({m}, pos.options());
  if (m)
    hipLaunchKernelGGL(lex_chunk_keys_kernel, dim3(grid_for(m)), dim3(kBlock),
                       0, cur_stream(), text.data_ptr<u8>(), text.numel(),
                       u64cp(pos), has_idx ? idx.data_ptr<i64>() : nullptr, m,
                       d, u64p(out));
  return out;
}

// -> (head flags, "string continues past chunk d" flags) of the active set
std::vector<torch::Tensor> lex_refine(torch::Tensor seg, torch::Tensor keys,
                                      torch::Tensor pos, torch::Tensor idx,
                                      long d) {
  check_dev_i64(seg, "seg");
  check_dev_i64(keys, "keys");
  check_dev_i64(pos, "pos");
  check_dev_i64(idx, "idx");
  long m = keys.numel();
  TORCH_CHECK(seg.numel() == m && idx.numel() == m,
              "seg, keys and idx must have one entry per active element");
  auto flags = torch::empty({m}, keys.options());
  auto more = torch::empty({m}, keys.options());
  if (m)
    hipLaunchKernelGGL(lex_refine_kernel, dim3(grid_for(m)), dim3(kBlock), 0,
                       cur_stream(), seg.data_ptr<i64>(), u64cp(keys),
                       u64cp(pos), idx.data_ptr<i64>(), m, d,
                       flags.data_ptr<i64>(), more.data_ptr<i64>());
  return {flags, more};
}

// out[q] = first j with string(perm[j]) >= query q; queries packed in
// qblob with offsets qoff[nq + 1]
torch::Tensor lex_lower_bound(torch::Tensor text, torch::Tensor pos,
                              torch::Tensor perm, torch::Tensor qblob,
                              torch::Tensor qoff) {
  check_text_u8(text);
  check_dev_i64(pos, "pos");
  check_dev_i64(perm, "perm");
  check_dev_i64(qoff, "qoff");
  TORCH_CHECK(qblob.is_cuda() && qblob.scalar_type() == torch::kUInt8 &&
              qblob.is_contiguous(), "qblob must be contiguous u8 on GPU");
  TORCH_CHECK(perm.numel() == pos.numel(), "perm must permute pos");
  TORCH_CHECK(qoff.numel() >= 1, "qoff holds nq + 1 offsets");
  long nq = qoff.numel() - 1;
  auto out = torch::empty({nq}, pos.options());
  if (nq)
    hipLaunchKernelGGL(lex_lower_bound_kernel, dim3(grid_for(nq)),
                       dim3(kBlock), 0, cur_stream(), text.data_ptr<u8>(),
                       text.numel(), u64cp(pos), perm.data_ptr<i64>(),
                       perm.numel(), qblob.data_ptr<u8>(),
                       qoff.data_ptr<i64>(), nq, out.data_ptr<i64>());
  return out;
}

// ------------------------------------------------------- ranked index search
// caps of postings_search: (terms per query, k, LDS candidate buffer)
std::vector<long> postings_search_caps() {
  return {PQ_TMAX, PQ_KMAX, PQ_BUF};
}

// One block per query over the CSR index; queries packed in qkeys with
// offsets qoff[nq + 1].  -> (docs[nq, k], scores[nq, k], n[nq], hits[nq]);
// unused slots hold doc = -1, score = 0.  weights: i64[nwords] or empty
// (= all 1).  mode: 0 = AND, 1 = OR.  No host sync.
std::vector<torch::Tensor> postings_search(
    torch::Tensor keys, torch::Tensor doc_offsets, torch::Tensor docs,
    torch::Tensor tf, torch::Tensor weights, torch::Tensor qkeys,
    torch::Tensor qoff, long k, long mode) {
  check_dev_i64(keys, "keys");
  check_dev_i64(doc_offsets, "doc_offsets");
  check_dev_i64(docs, "docs");
  check_dev_i64(tf, "tf");
  check_dev_i64(qkeys, "qkeys");
  check_dev_i64(qoff, "qoff");
  bool has_w = weights.numel() > 0;
  if (has_w) check_dev_i64(weights, "weights");
  long nwords = keys.numel();
  TORCH_CHECK(doc_offsets.numel() == nwords + 1,
              "doc_offsets holds nwords + 1 offsets");
  TORCH_CHECK(tf.numel() == docs.numel(), "tf must have one entry per doc");
  TORCH_CHECK(!has_w || weights.numel() == nwords,
              "weights must be empty or one per word");
  TORCH_CHECK(qoff.numel() >= 1, "qoff holds nq + 1 offsets");
  TORCH_CHECK(k >= 1 && k <= PQ_KMAX, "k must be in [1, ", PQ_KMAX, "]");
  TORCH_CHECK(mode == PQ_MODE_AND || mode == PQ_MODE_OR,
              "mode must be 0 (AND) or 1 (OR)");
  long nq = qoff.numel() - 1;
  auto opts = keys.options();
  auto out_docs = torch::empty({nq, k}, opts);
  auto out_scores = torch::empty({nq, k}, opts);
  auto out_n = torch::empty({nq}, opts);
  auto out_hits = torch::empty({nq}, opts);
  if (nq)
    hipLaunchKernelGGL(postings_search_kernel, dim3(nq), dim3(PQ_BLOCK), 0,
                       cur_stream(), u64cp(keys), nwords,
                       doc_offsets.data_ptr<i64>(), docs.data_ptr<i64>(),
                       tf.data_ptr<i64>(), docs.numel(),
                       has_w ? weights.data_ptr<i64>() : nullptr,
                       u64cp(qkeys), qkeys.numel(), qoff.data_ptr<i64>(),
                       (int)k, (int)mode, out_docs.data_ptr<i64>(),
                       out_scores.data_ptr<i64>(), out_n.data_ptr<i64>(),
                       out_hits.data_ptr<i64>());
  return {out_docs, out_scores, out_n, out_hits};
}

// ------------------------------------------------ positional index / phrases
// caps of token_ordinals: (bytes per counted granule)
std::vector<long> token_ordinals_caps() { return {TORD_GRANULE}; }

// Per occurrence pos = off << 16 | len: (doc i64[m], ord i32[m]), doc the
// index of the last starts[] entry <= off (-1 if none) and ord the 0-based
// token ordinal of the word within that document.  One streaming pass over
// the text counts word starts per granule, a scan turns the counts into
// prefixes, one thread per occurrence resolves.  No host sync.
std::vector<torch::Tensor> token_ordinals(torch::Tensor text,
                                          torch::Tensor pos,
                                          torch::Tensor starts) {
  check_text_u8(text);
  check_dev_i64(pos, "pos");
  check_dev_i64(starts, "starts");
  long n = text.numel();
  long m = pos.numel();
  long nstarts = starts.numel();
  TORCH_CHECK(n < (1L << 31), "token_ordinals: text of ", n,
              " bytes; ordinals are 32-bit");
  TORCH_CHECK(nstarts >= 1 && nstarts < (1L << 31),
              "starts holds ndocs + 1 offsets");
  auto i32 = torch::TensorOptions().device(text.device()).dtype(torch::kInt32);
  long ngran = (n + TORD_GRANULE - 1) / TORD_GRANULE;
  auto prefix = torch::zeros({ngran + 1}, i32);
  if (ngran) {
    auto gcount = torch::empty({ngran}, i32);
    hipLaunchKernelGGL(tord_count_kernel, dim3(grid_for(ngran * 8)),
                       dim3(TORD_BLOCK), 0, cur_stream(),
                       text.data_ptr<u8>(), n, gcount.data_ptr<int>(), ngran);
    prefix.slice(0, 1).copy_(gcount.cumsum(0, torch::kInt32));
  }
  auto doc_sb = torch::empty({nstarts}, i32);
  hipLaunchKernelGGL(tord_before_kernel, dim3(grid_for(nstarts)),
                     dim3(TORD_BLOCK), 0, cur_stream(), text.data_ptr<u8>(), n,
                     prefix.data_ptr<int>(), starts.data_ptr<i64>(), nstarts,
                     doc_sb.data_ptr<int>());
  auto out_doc = torch::empty({m}, pos.options());
  auto out_ord = torch::empty({m}, i32);
  if (m)
    hipLaunchKernelGGL(tord_resolve_kernel, dim3(grid_for(m)),
                       dim3(TORD_BLOCK), 0, cur_stream(), text.data_ptr<u8>(),
                       n, prefix.data_ptr<int>(), u64cp(pos), m,
                       starts.data_ptr<i64>(), (int)nstarts,
                       doc_sb.data_ptr<int>(), out_doc.data_ptr<i64>(),
                       out_ord.data_ptr<int>());
  return {out_doc, out_ord};
}

// Exact-phrase twin of postings_search: ordered terms, score = phrase
// frequency.  pos_offsets i64[np + 1] into positions i32[nocc].
std::vector<torch::Tensor> postings_phrase(
    torch::Tensor keys, torch::Tensor doc_offsets, torch::Tensor docs,
    torch::Tensor tf, torch::Tensor pos_offsets, torch::Tensor positions,
    torch::Tensor qkeys, torch::Tensor qoff, long k) {
  check_dev_i64(keys, "keys");
  check_dev_i64(doc_offsets, "doc_offsets");
  check_dev_i64(docs, "docs");
  check_dev_i64(tf, "tf");
  check_dev_i64(pos_offsets, "pos_offsets");
  check_dev_i64(qkeys, "qkeys");
  check_dev_i64(qoff, "qoff");
  TORCH_CHECK(positions.is_cuda() &&
                  positions.scalar_type() == torch::kInt32 &&
                  positions.is_contiguous(),
              "positions must be contiguous int32 on GPU");
  long nwords = keys.numel();
  long np = docs.numel();
  TORCH_CHECK(doc_offsets.numel() == nwords + 1,
              "doc_offsets holds nwords + 1 offsets");
  TORCH_CHECK(tf.numel() == np, "tf must have one entry per doc");
  TORCH_CHECK(pos_offsets.numel() == np + 1,
              "pos_offsets holds one offset per posting + 1");
  TORCH_CHECK(qoff.numel() >= 1, "qoff holds nq + 1 offsets");
  TORCH_CHECK(k >= 1 && k <= PQ_KMAX, "k must be in [1, ", PQ_KMAX, "]");
  long nq = qoff.numel() - 1;
  auto opts = keys.options();
  auto out_docs = torch::empty({nq, k}, opts);
  auto out_scores = torch::empty({nq, k}, opts);
  auto out_n = torch::empty({nq}, opts);
  auto out_hits = torch::empty({nq}, opts);
  if (nq)
    hipLaunchKernelGGL(postings_phrase_kernel, dim3(nq), dim3(PQ_BLOCK), 0,
                       cur_stream(), u64cp(keys), nwords,
                       doc_offsets.data_ptr<i64>(), docs.data_ptr<i64>(),
                       tf.data_ptr<i64>(), np, pos_offsets.data_ptr<i64>(),
                       positions.data_ptr<int>(), positions.numel(),
                       u64cp(qkeys), qkeys.numel(), qoff.data_ptr<i64>(),
                       (int)k, out_docs.data_ptr<i64>(),
                       out_scores.data_ptr<i64>(), out_n.data_ptr<i64>(),
                       out_hits.data_ptr<i64>());
  return {out_docs, out_scores, out_n, out_hits};
}

// ------------------------------------------------------------ sorted equi-join
// caps of the join kernels: (output rows per tile, off entries in LDS)
std::vector<long> join_caps() { return {JOIN_TILE, JOIN_LDS_ROWS}; }

// caps of the windowed bounds pass: (left rows per tile, window keys in LDS)
std::vector<long> join_bounds_caps() { return {JOIN_BTILE, JOIN_WIN}; }

// Pass 1 over two key columns sorted ascending in u64 bit order:
// (lo i64[nl], cnt i64[nl]), lo[i] the first right index with rk >= lk[i]
// and cnt[i] the number of right rows equal to lk[i].  window picks the
// block-window kernel over the thread-per-row one (same outputs).  No host
// sync.
std::vector<torch::Tensor> join_bounds(torch::Tensor lkeys,
                                       torch::Tensor rkeys, bool window) {
  check_dev_i64(lkeys, "lkeys");
  check_dev_i64(rkeys, "rkeys");
  TORCH_CHECK(lkeys.device() == rkeys.device(),
              "lkeys and rkeys must be on the same device");
  long nl = lkeys.numel();
  long nr = rkeys.numel();
  auto lo = torch::empty({nl}, lkeys.options());
  auto cnt = torch::empty({nl}, lkeys.options());
  const u64* rp = nr ? u64cp(rkeys) : nullptr;
  if (nl && window) {
    long ntiles = (nl + JOIN_BTILE - 1) / JOIN_BTILE;
    long blocks = ntiles < kMaxBlocks ? ntiles : kMaxBlocks;
    hipLaunchKernelGGL(join_bounds_window_kernel, dim3(blocks),
                       dim3(JOIN_BLOCK), 0, cur_stream(), u64cp(lkeys), nl,
                       rp, nr, ntiles, lo.data_ptr<i64>(),
                       cnt.data_ptr<i64>());
  } else if (nl) {
    hipLaunchKernelGGL(join_bounds_kernel, dim3(grid_for(nl)),
                       dim3(JOIN_BLOCK), 0, cur_stream(), u64cp(lkeys), nl,
                       rp, nr, lo.data_ptr<i64>(), cnt.data_ptr<i64>());
  }
  return {lo, cnt};
}

// Pass 2: off i64[nl + 1] = exclusive cumsum of the per-left-row output
// counts with off[nl] == total (read back by the caller, who sizes the
// output with it).  -> (li i64[total], ri i64[total]), ri == -1 on the
// output row of a left row with cnt == 0.
std::vector<torch::Tensor> join_expand(torch::Tensor off, torch::Tensor lo,
                                       torch::Tensor cnt, long total) {
  check_dev_i64(off, "off");
  check_dev_i64(lo, "lo");
  check_dev_i64(cnt, "cnt");
  TORCH_CHECK(off.device() == lo.device() && off.device() == cnt.device(),
              "off, lo and cnt must be on the same device");
  long nl = lo.numel();
  TORCH_CHECK(cnt.numel() == nl && off.numel() == nl + 1,
              "off holds one offset per left row + 1, cnt one count per row");
  TORCH_CHECK(total >= 0 && (total == 0 || nl > 0),
              "total must be >= 0, and 0 without left rows");
  auto li = torch::empty({total}, off.options());
  auto ri = torch::empty({total}, off.options());
  if (total) {
    long ntiles = (total + JOIN_TILE - 1) / JOIN_TILE;
    long blocks = ntiles < kMaxBlocks ? ntiles : kMaxBlocks;
    hipLaunchKernelGGL(join_expand_kernel, dim3(blocks), dim3(JOIN_BLOCK), 0,
                       cur_stream(), off.data_ptr<i64>(), nl,
                       lo.data_ptr<i64>(), cnt.data_ptr<i64>(), total, ntiles,
                       li.data_ptr<i64>(), ri.data_ptr<i64>());
  }
  return {li, ri};
}

// ----------------------------------------------------------- sorted as-of join
// caps of the windowed as-of kernel: (left rows per tile, right rows of a
// window staged in LDS)
std::vector<long> asof_caps() { return {ASOF_TILE, ASOF_WIN}; }

// Both sides sorted ascending on (key, order key of the time); times are
// int64 views, f64 says they hold doubles.  -> ri i64[nl]: the matched right
// row of every left row, or -1.  direction 0 backward, 1 forward, 2 nearest;
// row picks the thread-per-row kernel over the block-window one (same
// output).  No host sync.
torch::Tensor asof_sorted(torch::Tensor lkeys, torch::Tensor ltimes,
                          torch::Tensor rkeys, torch::Tensor rtimes,
                          long direction, std::optional<int64_t> tolerance,
                          bool allow_exact, bool f64, bool row) {
  check_dev_i64(lkeys, "lkeys");
  check_dev_i64(ltimes, "ltimes");
  check_dev_i64(rkeys, "rkeys");
  check_dev_i64(rtimes, "rtimes");
  TORCH_CHECK(lkeys.device() == ltimes.device() &&
                  lkeys.device() == rkeys.device() &&
                  lkeys.device() == rtimes.device(),
              "lkeys, ltimes, rkeys and rtimes must be on the same device");
  long nl = lkeys.numel();
  long nr = rkeys.numel();
  TORCH_CHECK(ltimes.numel() == nl, "ltimes must hold one time per left key");
  TORCH_CHECK(rtimes.numel() == nr, "rtimes must hold one time per right key");
  TORCH_CHECK(direction >= ASOF_BACKWARD && direction <= ASOF_NEAREST,
              "direction must be 0 (backward), 1 (forward) or 2 (nearest), "
              "got ", direction);
  TORCH_CHECK(!tolerance || *tolerance >= 0,
              "tolerance must be in [0, 2^63), got ", tolerance.value_or(0));
  TORCH_CHECK(!tolerance || !f64, "a tolerance needs int64 times");
  auto ri = torch::empty({nl}, lkeys.options());
  if (!nl) return ri;
  const u64* rkp = nr ? u64cp(rkeys) : nullptr;
  const u64* rtp = nr ? u64cp(rtimes) : nullptr;
  const int has_tol = tolerance ? 1 : 0;
  const u64 tol = (u64)tolerance.value_or(0);
  if (row) {
    hipLaunchKernelGGL(asof_row_kernel, dim3(grid_for(nl)), dim3(ASOF_BLOCK),
                       0, cur_stream(), u64cp(lkeys), u64cp(ltimes), nl, rkp,
                       rtp, nr, (int)direction, (int)allow_exact, has_tol, tol,
                       (int)f64, ri.data_ptr<i64>());
  } else {
    long ntiles = (nl + ASOF_TILE - 1) / ASOF_TILE;
    long blocks = ntiles < kMaxBlocks ? ntiles : kMaxBlocks;
    hipLaunchKernelGGL(asof_window_kernel, dim3(blocks), dim3(ASOF_BLOCK), 0,
                       cur_stream(), u64cp(lkeys), u64cp(ltimes), nl, rkp, rtp,
                       nr, ntiles, (int)direction, (int)allow_exact, has_tol,
                       tol, (int)f64, ri.data_ptr<i64>());
  }
  return ri;
}

// ------------------------------------------------- per-key order statistics
// caps of the group kernels: (rows per tile, rank specifications per pick)
std::vector<long> group_caps() { return {GROUP_TILE, GROUP_QMAX}; }

// the longest segment the tile kernel's rank-counting pass takes; a tile
// holding a longer one to finish runs the bitonic network
long group_rank_max() { return GROUP_RANK_MAX; }

namespace {
void check_group_rows(long n) {
  TORCH_CHECK(n < (1L << 31), "group ops take fewer than 2^31 rows, got ", n);
}
}  // namespace

// the u64 order key of each value (int64 view of an i64 or f64 column)
torch::Tensor group_order_keys(torch::Tensor vals, bool f64) {
  check_dev_i64(vals, "vals");
  long n = vals.numel();
  check_group_rows(n);
  auto out = torch::empty({n}, vals.options());
  if (n)
    hipLaunchKernelGGL(group_order_keys_kernel, dim3(grid_for(n)),
                       dim3(GROUP_BLOCK), 0, cur_stream(), u64cp(vals), n,
                       (int)f64, u64p(out));
  return out;
}

// seg i64[n]: nondecreasing segment id of every key-sorted row.  -> a fresh
// column with the values of every segment that lies inside one tile of
// GROUP_TILE rows in order; rows of other segments are unspecified (a tile
// inside one such segment is not written at all).  No host sync.
torch::Tensor group_tile_sort(torch::Tensor seg, torch::Tensor vals,
                              bool f64) {
  check_dev_i64(seg, "seg");
  check_dev_i64(vals, "vals");
  TORCH_CHECK(seg.device() == vals.device(),
              "seg and vals must be on the same device");
  long n = vals.numel();
  TORCH_CHECK(seg.numel() == n, "seg must hold one segment id per value");
  check_group_rows(n);
  auto out = torch::empty({n}, vals.options());
  if (n) {
    long ntiles = (n + GROUP_TILE - 1) / GROUP_TILE;
    hipLaunchKernelGGL(group_tile_sort_kernel<false>, dim3(ntiles),
                       dim3(GROUP_BLOCK), 0, cur_stream(),
                       seg.data_ptr<i64>(), u64cp(vals), n, (int)f64,
                       u64p(out), (i64*)nullptr);
  }
  return out;
}

// group_tile_sort plus perm i64[n]: out[i] == vals[perm[i]] wherever out[i]
// is specified; perm is unspecified exactly where out is.  No host sync.
std::vector<torch::Tensor> group_tile_sort_perm(torch::Tensor seg,
                                                torch::Tensor vals,
                                                bool f64) {
  check_dev_i64(seg, "seg");
  check_dev_i64(vals, "vals");
  TORCH_CHECK(seg.device() == vals.device(),
              "seg and vals must be on the same device");
  long n = vals.numel();
  TORCH_CHECK(seg.numel() == n, "seg must hold one segment id per value");
  check_group_rows(n);
  auto out = torch::empty({n}, vals.options());
  auto perm = torch::empty({n}, vals.options());
  if (n) {
    long ntiles = (n + GROUP_TILE - 1) / GROUP_TILE;
    hipLaunchKernelGGL(group_tile_sort_kernel<true>, dim3(ntiles),
                       dim3(GROUP_BLOCK), 0, cur_stream(),
                       seg.data_ptr<i64>(), u64cp(vals), n, (int)f64,
                       u64p(out), perm.data_ptr<i64>());
  }
  return {out, perm};
}

// out[s, q] = vals[off[s] + (num[q] * (len - 1) + add[q]) / den[q]], add =
// den - 1 where higher[q] else 0; 0 for an empty segment.  No host sync.
torch::Tensor group_pick(torch::Tensor offsets, torch::Tensor vals,
                         std::vector<long> num, std::vector<long> den,
                         std::vector<bool> higher) {
  check_dev_i64(offsets, "offsets");
  check_dev_i64(vals, "vals");
  TORCH_CHECK(offsets.device() == vals.device(),
              "offsets and vals must be on the same device");
  TORCH_CHECK(offsets.numel() >= 1, "offsets holds nseg + 1 entries");
  long nq = (long)num.size();
  TORCH_CHECK(nq >= 1 && nq <= GROUP_QMAX, "Q must be in [1, ", GROUP_QMAX,
              "], got ", nq);
  TORCH_CHECK((long)den.size() == nq && (long)higher.size() == nq,
              "num, den and higher must have one entry per specification");
  long n = vals.numel();
  check_group_rows(n);
  GroupSpecs sp;
  for (long q = 0; q < nq; ++q) {
    TORCH_CHECK(den[q] >= 1 && den[q] <= 1000000,
                "den must be in [1, 10^6], got ", den[q]);
    TORCH_CHECK(num[q] >= 0 && num[q] <= den[q],
                "num must be in [0, den], got ", num[q], "/", den[q]);
    sp.num[q] = (u32)num[q];
    sp.den[q] = (u32)den[q];
    sp.add[q] = higher[q] ? (u32)(den[q] - 1) : 0u;
  }
  for (long q = nq; q < GROUP_QMAX; ++q) {
    sp.num[q] = 0;
    sp.den[q] = 1;
    sp.add[q] = 0;
  }
  long nseg = offsets.numel() - 1;
  auto out = torch::empty({nseg, nq}, vals.options());
  if (nseg)
    hipLaunchKernelGGL(group_pick_kernel, dim3(grid_for(nseg * nq)),
                       dim3(GROUP_BLOCK), 0, cur_stream(),
                       offsets.data_ptr<i64>(), nseg, u64cp(vals), n, sp,
                       (int)nq, u64p(out));
  return out;
}

// flags i64[n]: 1 where a key-sorted row starts a segment or its order key
// differs from the previous row's.  No host sync.
torch::Tensor group_distinct_flags(torch::Tensor keys, torch::Tensor vals,
                                   bool f64) {
  check_dev_i64(keys, "keys");
  check_dev_i64(vals, "vals");
  TORCH_CHECK(keys.device() == vals.device(),
              "keys and vals must be on the same device");
  long n = keys.numel();
  TORCH_CHECK(vals.numel() == n, "vals must hold one value per key");
  check_group_rows(n);
  auto flags = torch::empty({n}, keys.options());
  if (n)
    hipLaunchKernelGGL(group_distinct_flags_kernel, dim3(grid_for(n)),
                       dim3(GROUP_BLOCK), 0, cur_stream(), u64cp(keys),
                       u64cp(vals), n, (int)f64, flags.data_ptr<i64>());
  return flags;
}

// ------------------------------------------------- per-key running aggregates
// caps of the scan kernels: (rows per tile, tiles per trip of the carry pass)
std::vector<long> seg_scan_caps() { return {SEG_SCAN_TILE, SEG_CARRY_CHUNK}; }

namespace {
void check_seg_rows(long n) {
  TORCH_CHECK(n < (1L << 31), "scan ops take fewer than 2^31 rows, got ", n);
}

long check_seg_scan_cols(const torch::Tensor& keys,
                         const torch::Tensor& vals, long op) {
  check_dev_i64(keys, "keys");
  check_dev_i64(vals, "vals");
  TORCH_CHECK(keys.device() == vals.device(),
              "keys and vals must be on the same device");
  long n = keys.numel();
  TORCH_CHECK(vals.numel() == n, "vals must hold one value per key");
  check_seg_rows(n);
  TORCH_CHECK(op >= SEG_SUM && op <= SEG_MAX,
              "op must be 0 (sum), 1 (min) or 2 (max), got ", op);
  return n;
}

void check_seg_tiles(const torch::Tensor& f, const torch::Tensor& a,
                     const torch::Tensor& like, long ntiles,
                     const char* what) {
  check_dev_i64(f, what);
  check_dev_i64(a, what);
  TORCH_CHECK(f.device() == like.device() && a.device() == like.device(),
              what, " must be on the device of the rows");
  TORCH_CHECK(f.numel() == ntiles && a.numel() == ntiles, what,
              " must hold one entry per tile (", ntiles, ")");
}

// one launch of KERNEL<op, f64> with the given grid
#define SEG_SCAN_LAUNCH(KERNEL, grid, ...)                                  \
  do {                                                                      \
    dim3 g_(grid), b_(SEG_SCAN_BLOCK);                                      \
    if (op == SEG_SUM && !f64)                                              \
      hipLaunchKernelGGL((KERNEL<SEG_SUM, false>), g_, b_, 0, cur_stream(), \
                         __VA_ARGS__);                                      \
    else if (op == SEG_SUM)                                                 \
      hipLaunchKernelGGL((KERNEL<SEG_SUM, true>), g_, b_, 0, cur_stream(),  \
                         __VA_ARGS__);                                      \
    else if (op == SEG_MIN && !f64)                                         \
      hipLaunchKernelGGL((KERNEL<SEG_MIN, false>), g_, b_, 0, cur_stream(), \
                         __VA_ARGS__);                                      \
    else if (op == SEG_MIN)                                                 \
      hipLaunchKernelGGL((KERNEL<SEG_MIN, true>), g_, b_, 0, cur_stream(),  \
                         __VA_ARGS__);                                      \
    else if (!f64)                                                          \
      hipLaunchKernelGGL((KERNEL<SEG_MAX, false>), g_, b_, 0, cur_stream(), \
                         __VA_ARGS__);                                      \
    else                                                                    \
      hipLaunchKernelGGL((KERNEL<SEG_MAX, true>), g_, b_, 0, cur_stream(),  \
                         __VA_ARGS__);                                      \
  } while (0)
}  // namespace

// Pass 1 of scan_by_key_sorted: (tile_f, tile_a) i64[ntiles], the head flag
// bits and the aggregate behind the last head of every tile of
// SEG_SCAN_TILE rows.  vals is the int64 view of an i64 or f64 column.
std::vector<torch::Tensor> seg_scan_reduce(torch::Tensor keys,
                                           torch::Tensor vals, long op,
                                           bool f64) {
  long n = check_seg_scan_cols(keys, vals, op);
  long ntiles = (n + SEG_SCAN_TILE - 1) / SEG_SCAN_TILE;
  auto tf = torch::empty({ntiles}, keys.options());
  auto ta = torch::empty({ntiles}, keys.options());
  if (ntiles)
    SEG_SCAN_LAUNCH(seg_scan_reduce_kernel, ntiles, u64cp(keys), u64cp(vals),
                    n, tf.data_ptr<i64>(), u64p(ta));
  return {tf, ta};
}

// Pass 2: (carry_f, carry_a) i64[ntiles], the exclusive segmented scan of
// the tile pairs, by one block.
std::vector<torch::Tensor> seg_scan_carry(torch::Tensor tile_f,
                                          torch::Tensor tile_a, long op,
                                          bool f64) {
  long ntiles = tile_f.numel();
  check_seg_tiles(tile_f, tile_a, tile_f, ntiles, "tile_f and tile_a");
  TORCH_CHECK(op >= SEG_SUM && op <= SEG_MAX,
              "op must be 0 (sum), 1 (min) or 2 (max), got ", op);
  auto cf = torch::empty({ntiles}, tile_f.options());
  auto ca = torch::empty({ntiles}, tile_f.options());
  if (ntiles)
    SEG_SCAN_LAUNCH(seg_scan_carry_kernel, 1, tile_f.data_ptr<i64>(),
                    u64cp(tile_a), ntiles, cf.data_ptr<i64>(), u64p(ca));
  return {cf, ca};
}

// Pass 3: the running column, every tile rescanned behind its carry.
torch::Tensor seg_scan_apply(torch::Tensor keys, torch::Tensor vals,
                             torch::Tensor carry_f, torch::Tensor carry_a,
                             long op, bool f64) {
  long n = check_seg_scan_cols(keys, vals, op);
  long ntiles = (n + SEG_SCAN_TILE - 1) / SEG_SCAN_TILE;
  check_seg_tiles(carry_f, carry_a, keys, ntiles, "carry_f and carry_a");
  auto out = torch::empty({n}, vals.options());
  if (ntiles)
    SEG_SCAN_LAUNCH(seg_scan_apply_kernel, ntiles, u64cp(keys), u64cp(vals),
                    n, carry_f.data_ptr<i64>(), u64cp(carry_a), u64p(out));
  return out;
}

// running[i] = op over the rows of i's segment up to and including i; a
// segment starts at row 0 and wherever the key changes.  Three launches, no
// host sync; the inputs are never written.
torch::Tensor scan_by_key_sorted(torch::Tensor keys, torch::Tensor vals,
                                 long op, bool f64) {
  long n = check_seg_scan_cols(keys, vals, op);
  if (!n) return torch::empty({0}, vals.options());
  auto t = seg_scan_reduce(keys, vals, op, f64);
  auto c = seg_scan_carry(t[0], t[1], op, f64);
  return seg_scan_apply(keys, vals, c[0], c[1], op, f64);
}

// flags i64[n]: 1 where a row starts a key or its i64 time exceeds the
// previous row's by more than gap (times ascending within each key).  No
// host sync.
torch::Tensor session_flags(torch::Tensor keys, torch::Tensor times,
                            long gap) {
  check_dev_i64(keys, "keys");
  check_dev_i64(times, "times");
  TORCH_CHECK(keys.device() == times.device(),
              "keys and times must be on the same device");
  long n = keys.numel();
  TORCH_CHECK(times.numel() == n, "times must hold one time per key");
  check_seg_rows(n);
  TORCH_CHECK(gap >= 0, "gap must be in [0, 2^63), got ", gap);
  auto flags = torch::empty({n}, keys.options());
  if (n)
    hipLaunchKernelGGL(seg_session_flags_kernel, dim3(grid_for(n)),
                       dim3(SEG_SCAN_BLOCK), 0, cur_stream(), u64cp(keys),
                       u64cp(times), n, (u64)gap, flags.data_ptr<i64>());
  return flags;
}

// ------------------------------------------------- per-key rolling aggregates
// caps of the frame kernels: (rows per tile of the window bounds kernel, rows
// of a window staged in LDS, rows per tile of the reduce kernels)
std::vector<long> frame_caps() { return {FRAME_TILE, FRAME_WIN, FRAME_RTILE}; }

namespace {
static_assert(FRAME_BLOCK == SEG_SCAN_BLOCK,
              "the frame kernels are launched by SEG_SCAN_LAUNCH");

long check_frame_op(const torch::Tensor& vals, long op) {
  check_dev_i64(vals, "vals");
  long n = vals.numel();
  TORCH_CHECK(n < (1L << 31), "frame ops take fewer than 2^31 rows, got ", n);
  TORCH_CHECK(op >= SEG_SUM && op <= SEG_MAX,
              "op must be 0 (sum), 1 (min) or 2 (max), got ", op);
  return n;
}

void check_frame_col(const torch::Tensor& t, const torch::Tensor& like,
                     long n, const char* name) {
  check_dev_i64(t, name);
  TORCH_CHECK(t.device() == like.device(), name,
              " must be on the device of the rows");
  TORCH_CHECK(t.numel() == n, name, " must hold ", n, " entries, got ",
              t.numel());
}
}  // namespace

// Rows sorted ascending on (key, order key of the i64 time).  -> (lo, hi)
// i64[n]: row i's frame is the rows [lo[i], hi[i]) of its key whose time lies
// in [t_i - preceding, t_i + following], both ends saturating.  row picks
// the thread-per-row kernel over the block-window one (same output).  No
// host sync.
std::vector<torch::Tensor> frame_bounds(torch::Tensor keys,
                                        torch::Tensor times, long preceding,
                                        long following, bool row) {
  check_dev_i64(keys, "keys");
  check_dev_i64(times, "times");
  TORCH_CHECK(keys.device() == times.device(),
              "keys and times must be on the same device");
  long n = keys.numel();
  TORCH_CHECK(times.numel() == n, "times must hold one time per key");
  TORCH_CHECK(n < (1L << 31), "frame ops take fewer than 2^31 rows, got ", n);
  TORCH_CHECK(preceding >= 0, "preceding must be in [0, 2^63), got ",
              preceding);
  TORCH_CHECK(following >= 0, "following must be in [0, 2^63), got ",
              following);
  auto lo = torch::empty({n}, keys.options());
  auto hi = torch::empty({n}, keys.options());
  if (!n) return {lo, hi};
  if (row) {
    hipLaunchKernelGGL(frame_bounds_row_kernel, dim3(grid_for(n)),
                       dim3(FRAME_BLOCK), 0, cur_stream(), u64cp(keys),
                       u64cp(times), n, (u64)preceding, (u64)following,
                       lo.data_ptr<i64>(), hi.data_ptr<i64>());
  } else {
    long ntiles = (n + FRAME_TILE - 1) / FRAME_TILE;
    long blocks = ntiles < kMaxBlocks ? ntiles : kMaxBlocks;
    hipLaunchKernelGGL(frame_bounds_window_kernel, dim3(blocks),
                       dim3(FRAME_BLOCK), 0, cur_stream(), u64cp(keys),
                       u64cp(times), n, ntiles, (u64)preceding,
                       (u64)following, lo.data_ptr<i64>(),
                       hi.data_ptr<i64>());
  }
  return {lo, hi};
}

// Pass 1 of frame_reduce: (pre, suf) i64[n], the aggregate from the first
// row of a row's tile of FRAME_RTILE rows up to the row and from the row to
// the tile's last row, and tiles i64[ntiles], the tiles' own aggregates.
// vals is the int64 view of an i64 or f64 column.
std::vector<torch::Tensor> frame_tile(torch::Tensor vals, long op, bool f64) {
  long n = check_frame_op(vals, op);
  long ntiles = (n + FRAME_RTILE - 1) / FRAME_RTILE;
  auto pre = torch::empty({n}, vals.options());
  auto suf = torch::empty({n}, vals.options());
  auto tiles = torch::empty({ntiles}, vals.options());
  if (ntiles)
    SEG_SCAN_LAUNCH(frame_tile_kernel, ntiles, u64cp(vals), n, u64p(pre),
                    u64p(suf), u64p(tiles));
  return {pre, suf, tiles};
}

// Pass 2: the aligned binary tree over the tile aggregates, by one block:
// level l holds the ntiles >> l nodes whose 2^l tiles all exist, the levels
// one behind the other from level 0 (the tiles themselves) up.
torch::Tensor frame_tree(torch::Tensor tiles, long op, bool f64) {
  long ntiles = check_frame_op(tiles, op);
  auto tree = torch::empty({frame_tree_size(ntiles)}, tiles.options());
  if (ntiles)
    SEG_SCAN_LAUNCH(frame_tree_kernel, 1, u64cp(tiles), ntiles, u64p(tree));
  return tree;
}

// Pass 3: out[i] = op over vals[lo[i]:hi[i]], lo clamped to [0, i] and hi to
// [i + 1, n].
torch::Tensor frame_apply(torch::Tensor vals, torch::Tensor lo,
                          torch::Tensor hi, torch::Tensor pre,
                          torch::Tensor suf, torch::Tensor tree, long op,
                          bool f64) {
  long n = check_frame_op(vals, op);
  check_frame_col(lo, vals, n, "lo");
  check_frame_col(hi, vals, n, "hi");
  check_frame_col(pre, vals, n, "pre");
  check_frame_col(suf, vals, n, "suf");
  long ntiles = (n + FRAME_RTILE - 1) / FRAME_RTILE;
  check_frame_col(tree, vals, frame_tree_size(ntiles), "tree");
  auto out = torch::empty({n}, vals.options());
  if (ntiles)
    SEG_SCAN_LAUNCH(frame_apply_kernel, ntiles, u64cp(vals),
                    lo.data_ptr<i64>(), hi.data_ptr<i64>(), n, u64cp(pre),
                    u64cp(suf), u64cp(tree), ntiles, u64p(out));
  return out;
}

// out[i] = op over the rows lo[i] <= j < hi[i] of vals, the earlier row
// first; every frame holds its own row.  Three launches, no host sync; the
// inputs are never written.
torch::Tensor frame_reduce(torch::Tensor vals, torch::Tensor lo,
                           torch::Tensor hi, long op, bool f64) {
  long n = check_frame_op(vals, op);
  check_frame_col(lo, vals, n, "lo");
  check_frame_col(hi, vals, n, "hi");
  if (!n) return torch::empty({0}, vals.options());
  auto t = frame_tile(vals, op, f64);
  auto tree = frame_tree(t[2], op, f64);
  return frame_apply(vals, lo, hi, t[0], t[1], tree, op, f64);
}

// ------------------------------------------------ resident-graph propagation
// caps of the graph kernels: (edges per tile, most blocks of the update pass)
std::vector<long> graph_caps() { return {GRAPH_TILE, GRAPH_PR_BLOCKS}; }

namespace {
static_assert(GRAPH_BLOCK == SEG_SCAN_BLOCK,
              "the graph kernels are launched by SEG_SCAN_LAUNCH");

void check_graph_f64(const torch::Tensor& t, const torch::Tensor& like,
                     long n, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.scalar_type() == torch::kFloat64, name, " must be float64");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.device() == like.device(), name,
              " must be on the device of sums");
  TORCH_CHECK(t.numel() == n, name, " must hold ", n, " entries, got ",
              t.numel());
}
}  // namespace

// out[v] = op over e in [offsets[v], offsets[v + 1]) of x[src[e]]; x is the
// int64 view of an i64 or f64 column of n rows, offsets i64[n + 1], src
// int32[m].  A src outside [0, n) contributes the identity (0, INT64_MAX,
// INT64_MIN) and an empty row is the identity.  Three launches behind one
// fill, no host sync; the inputs are never written.
torch::Tensor graph_propagate(torch::Tensor offsets, torch::Tensor src,
                              torch::Tensor x, long op, bool f64) {
  check_dev_i64(offsets, "offsets");
  check_dev_i64(x, "x");
  TORCH_CHECK(src.is_cuda(), "src must be on GPU");
  TORCH_CHECK(src.scalar_type() == torch::kInt32, "src must be int32");
  TORCH_CHECK(src.is_contiguous(), "src must be contiguous");
  TORCH_CHECK(offsets.device() == x.device() && src.device() == x.device(),
              "offsets, src and x must be on the same device");
  long n = x.numel(), m = src.numel();
  TORCH_CHECK(offsets.numel() == n + 1, "offsets must hold ", n + 1,
              " entries, got ", offsets.numel());
  TORCH_CHECK(n < (1L << 31) && m < (1L << 31),
              "graph ops take fewer than 2^31 edges and rows, got ", m,
              " and ", n);
  TORCH_CHECK(op >= SEG_SUM && op <= SEG_MAX,
              "op must be 0 (sum), 1 (min) or 2 (max), got ", op);
  TORCH_CHECK(op == SEG_SUM || !f64, "graph min / max take int64 values");
  const i64 ident = op == SEG_SUM ? 0
                    : op == SEG_MIN ? std::numeric_limits<i64>::max()
                                    : std::numeric_limits<i64>::min();
  auto out = torch::full({n}, ident, x.options());
  if (!n || !m) return out;
  long ntiles = (m + GRAPH_TILE - 1) / GRAPH_TILE;
  auto tf = torch::empty({ntiles}, x.options());
  auto ta = torch::empty({ntiles}, x.options());
  auto lr = torch::empty({ntiles}, x.options());
  auto la = torch::empty({ntiles}, x.options());
  SEG_SCAN_LAUNCH(graph_tile_kernel, ntiles, offsets.data_ptr<i64>(),
                  src.data_ptr<int>(), u64cp(x), n, m, u64p(out),
                  tf.data_ptr<i64>(), u64p(ta), lr.data_ptr<i64>(), u64p(la));
  auto c = seg_scan_carry(tf, ta, op, f64);
  SEG_SCAN_LAUNCH(graph_lead_kernel, grid_for(ntiles), lr.data_ptr<i64>(),
                  u64cp(la), c[0].data_ptr<i64>(), u64cp(c[1]), ntiles, n,
                  u64p(out));
  return out;
}

// One PageRank update over n nodes -> (new, contrib, partials f64[blocks, 2]);
// partials[:, 0] sums to |new - old|_1 and partials[:, 1] to the rank held by
// nodes whose inv_out is 0.  dangling is a 0-dim (or 1-element) device
// tensor.  No host sync.
std::vector<torch::Tensor> pagerank_update(torch::Tensor sums,
                                           torch::Tensor old,
                                           torch::Tensor inv_out,
                                           double damping,
                                           torch::Tensor dangling) {
  long n = sums.numel();
  check_graph_f64(sums, sums, n, "sums");
  check_graph_f64(old, sums, n, "old");
  check_graph_f64(inv_out, sums, n, "inv_out");
  check_graph_f64(dangling, sums, 1, "dangling");
  TORCH_CHECK(n < (1L << 31), "graph ops take fewer than 2^31 rows, got ", n);
  auto nw = torch::empty({n}, sums.options());
  auto contrib = torch::empty({n}, sums.options());
  long blocks = n ? grid_for(n) : 0;
  if (blocks > GRAPH_PR_BLOCKS) blocks = GRAPH_PR_BLOCKS;
  auto partials = torch::empty({blocks, 2}, sums.options());
  if (blocks)
    hipLaunchKernelGGL(pagerank_update_kernel, dim3(blocks),
                       dim3(GRAPH_BLOCK), 0, cur_stream(),
                       sums.data_ptr<double>(), old.data_ptr<double>(),
                       inv_out.data_ptr<double>(), n, damping,
                       dangling.data_ptr<double>(), nw.data_ptr<double>(),
                       contrib.data_ptr<double>(),
                       partials.data_ptr<double>());
  return {nw, contrib, partials};
}

// Occupancy of the default word-count tokenizer instantiation on the
// current device, as the runtime sees it (blocks/CU clips the grid; the
// register count and static LDS are what decide it), and which body this
// process runs ("v7", or "v6" under MR_TOKENIZE_V6=1).
py::dict tokenizer_occupancy() {
  auto kfn = Tok<2048, true, false, false, 2048>::kernel();
  TokOccupancy o = tok_occupancy(reinterpret_cast<const void*>(kfn), kBlock);
  hipFuncAttributes fa;
  C10_HIP_CHECK(hipFuncGetAttributes(&fa, reinterpret_cast<const void*>(kfn)));
  py::dict d;
  d["blocks_per_cu"] = o.blocks_per_cu;
  d["cus"] = o.cus;
  d["num_regs"] = fa.numRegs;
  d["lds_bytes"] = (long)fa.sharedSizeBytes;
  d["body"] = tok_v6_forced() ? "v6" : "v7";
  return d;
}

std::string tokenizer_last_body() { return g_tok_last_body; }

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("tokenizer_last_body", &tokenizer_last_body,
        "body of the last v6/v7 tokenizer launch: v7, v6 or none");
  m.def("group_caps", &group_caps, "(TILE, QMAX) of the group kernels");
  m.def("group_rank_max", &group_rank_max,
        "longest segment of the tile kernel's rank-counting pass");
  m.def("group_order_keys", &group_order_keys,
        "u64 order key of each i64 / f64 value");
  m.def("group_tile_sort", &group_tile_sort,
        "values ordered inside every segment that fits one tile");
  m.def("group_tile_sort_perm", &group_tile_sort_perm,
        "group_tile_sort plus the input row of every value");
  m.def("seg_scan_caps", &seg_scan_caps,
        "(TILE, CARRY_CHUNK) of the segmented scan");
  m.def("scan_by_key_sorted", &scan_by_key_sorted,
        "inclusive sum/min/max scan within runs of equal keys");
  m.def("seg_scan_reduce", &seg_scan_reduce,
        "pass 1 of scan_by_key_sorted: per-tile (flags, aggregate)");
  m.def("seg_scan_carry", &seg_scan_carry,
        "pass 2 of scan_by_key_sorted: per-tile carry-in");
  m.def("seg_scan_apply", &seg_scan_apply,
        "pass 3 of scan_by_key_sorted: the running column");
  m.def("session_flags", &session_flags,
        "1 where a row starts a key or follows a gap in time");
  m.def("graph_caps", &graph_caps,
        "(TILE, PR_BLOCKS) of the graph kernels");
  m.def("graph_propagate", &graph_propagate,
        "sum / min / max over every row's in-edges of a gathered column");
  m.def("pagerank_update", &pagerank_update,
        "one PageRank update -> (new, contrib, partials)");
  m.def("frame_caps", &frame_caps,
        "(TILE, WIN, RTILE) of the frame kernels");
  m.def("frame_bounds", &frame_bounds, py::arg("keys"), py::arg("times"),
        py::arg("preceding"), py::arg("following"), py::arg("row") = false,
        "range frames of (key, time)-sorted rows -> (lo, hi)");
  m.def("frame_reduce", &frame_reduce,
        "sum / min / max of a value column over per-row frames");
  m.def("frame_tile", &frame_tile,
        "frame_reduce pass 1: (pre, suf, tile aggregates)");
  m.def("frame_tree", &frame_tree,
        "frame_reduce pass 2: the tree over the tile aggregates");
  m.def("frame_apply", &frame_apply,
        "frame_reduce pass 3: one range query per row");
  m.def("group_pick", &group_pick,
        "values at exact rank fractions of each ordered segment");
  m.def("group_distinct_flags", &group_distinct_flags,
        "1 where a row starts a segment or a new value");
  m.def("join_bounds", &join_bounds, py::arg("lkeys"), py::arg("rkeys"),
        py::arg("window") = true,
        "(lo, cnt) of each left key in the sorted right keys");
  m.def("join_bounds_caps", &join_bounds_caps,
        "(BTILE, WIN) of the windowed join_bounds");
  m.def("join_expand", &join_expand,
        "(li, ri) row pairs from the bounds and their exclusive cumsum");
  m.def("join_caps", &join_caps, "(TILE, LDS_ROWS) of join_expand");
  m.def("asof_sorted", &asof_sorted, py::arg("lkeys"), py::arg("ltimes"),
        py::arg("rkeys"), py::arg("rtimes"), py::arg("direction") = 0,
        py::arg("tolerance") = py::none(), py::arg("allow_exact") = true,
        py::arg("f64") = false, py::arg("row") = false,
        "matched right row (or -1) of each left row of two sorted relations");
  m.def("asof_caps", &asof_caps, "(TILE, WIN) of the windowed asof_sorted");
  m.def("tokenizer_occupancy", &tokenizer_occupancy,
        "blocks/CU, registers and static LDS of the default tokenizer");
  m.def("postings_search", &postings_search,
        "ranked AND/OR top-k over the inverted index, one block per query");
  m.def("postings_search_caps", &postings_search_caps,
        "(TMAX, KMAX, BUF) of postings_search");
  m.def("postings_phrase", &postings_phrase,
        "exact-phrase top-k over the positional index, one block per query");
  m.def("token_ordinals", &token_ordinals,
        "(doc, token ordinal within doc) of each occurrence");
  m.def("token_ordinals_caps", &token_ordinals_caps,
        "(GRANULE) of token_ordinals");
  m.def("lex_chunk_keys", &lex_chunk_keys,
        "big-endian 8-byte chunk d of each string as a sortable u64");
  m.def("lex_refine", &lex_refine,
        "(seg, key) head flags + unfinished-string flags");
  m.def("lex_lower_bound", &lex_lower_bound,
        "binary search of byte-string queries in a lex permutation");
  m.def("radix_sort_idx32", &radix_sort_idx32,
        "sort u64 keys with a u32 iota payload -> (keys, perm)");
  m.def("gather_by_u32", &gather_by_u32, "out[i] = vals[idx[i]] (u32 idx)");
  m.def("tokenize", &tokenize, "tokenize text -> (hash, pos, count)");
  m.def("tokenize_count", &tokenize_count,
        "fused tokenize + hash-table count");
  m.def("tokenize_spill_composite", &tokenize_spill_composite,
        py::arg("text"), py::arg("pos_base"), py::arg("cap"),
        py::arg("split_off"), py::arg("doc_base"), py::arg("max_blocks") = 0,
        "spill-all with fused (word,doc) composite keys");
  m.def("tokenize_cache_spill_composite", &tokenize_cache_spill_composite,
        py::arg("text"), py::arg("pos_base"), py::arg("tkeys"),
        py::arg("tvals"), py::arg("texm"), py::arg("spill_cap"),
        py::arg("nwords"), py::arg("out_hash"), py::arg("out_pos"),
        py::arg("counter"), py::arg("split_off"), py::arg("doc_base"),
        py::arg("max_blocks") = 0,
        "composite keys with the LDS cache (misses spill)");
  m.def("tokenize_spill_v2", &tokenize_spill_v2, py::arg("text"),
        py::arg("pos_base"), py::arg("cap"), py::arg("max_blocks") = 0,
        "spill-all tokenizer (chunk-padded; filter HT_EMPTY)");
  m.def("tokenize_cache_spill",&tokenize_cache_spill, py::arg("text"),
        py::arg("pos_base"), py::arg("tkeys"), py::arg("tvals"),
        py::arg("texm"), py::arg("spill_cap"), py::arg("nwords"),
        py::arg("out_hash"), py::arg("out_pos"), py::arg("counter"),
        py::arg("max_blocks") = 0,
        "tokenize; LDS cache counts the head, misses spill");
  m.def("bucket_count", &bucket_count,
        "LDS count of bucket-partitioned (hash,pos)");
  m.def("hash_insert_count", &hash_insert_count);
  m.def("hash_insert_sum_i64", &hash_insert_sum_i64);
  m.def("hash_extract", &hash_extract);
  m.def("hash_extract_v2", &hash_extract_v2,
        "chunked compaction (HT_EMPTY-padded; mask/trim downstream)");
  m.def("extract_sorted", &extract_sorted,
        "table -> (packed keys|counts|lens, pos, offs, host meta), sorted");
  m.def("extract_sorted_caps", &extract_sorted_caps,
        "(RANK_M, SCAN_TILE) of extract_sorted");
  m.def("head_flags", &head_flags);
  m.def("seg_reduce_i64", &seg_reduce_i64);
  m.def("seg_reduce_i64_minmax", &seg_reduce_i64_minmax);
  m.def("seg_reduce_f64_minmax", &seg_reduce_f64_minmax);
  m.def("seg_first_u64", &seg_first_u64);
  m.def("seg_reduce_f64", &seg_reduce_f64);
  m.def("partition_hist", &partition_hist);
  m.def("pos_len", &pos_len);
  m.def("gather_bytes", &gather_bytes);
  m.def("radix_sort_pairs", &radix_sort_pairs);
  m.def("radix_sort_caps", &radix_sort_caps,
        "(tile records, direct scatter 0/1) of this process's radix sorts");
  m.def("radix_pass", &radix_pass);
  m.def("radix_bucketize", &radix_bucketize, py::arg("keys"),
        py::arg("vals"), py::arg("shift"), py::arg("skip_empty") = false,
        "one-digit partition with native scan -> (keys, vals, bucket_off)");
  m.def("grad_colsum", &grad_colsum, "sum G gradient rows -> D (K6)");
}
