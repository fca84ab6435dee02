// The suffix array of an FM index's text by prefix doubling over prims::radix_sort_pairs_u64, and the arrays that are
// made from it: gfx950, wave64.
//
// The text is the 2-bit codes of all segments back to back, no separators, with the sentinel -- smaller than every
// base -- at position n.  Row 0 of the suffix array is therefore always the sentinel's; the n real suffixes are sorted
// here and row i + 1 is the i-th of them.
//
//   round 0    key = the first kSaFirstBases bases of the suffix, first base most significant, read from the packed
//              text (bases past the end read as code 0: the text is zero-padded).  A suffix SHORTER than the key is a
//              prefix of whatever shares its padded key and must come first, the shortest first of all.  The pairs go
//              into the sort in DESCENDING position order and the sort is stable, so among equal keys the shortest
//              suffix is first already; such a suffix is its own group (sa_first_heads_kernel), which is the tie rule
//              "by remaining length" without a key bit spent on it.
//   round k    ranks after a round of width h: equal <=> the first h bases are equal and both suffixes are at least h
//              long.  key = (rank[p], rank[p + h]) with rank 0 for p + h >= n -- below every real rank, because the
//              suffix that ends there is the shorter one -- sorted over the 2 * bitlen(groups) bits in use; h doubles.
//   ranks      head flag = key differs from the row in front; prims::inclusive_sum_u32 of the flags = dense ranks
//              1..groups; the host reads `groups` once per round.
// The loop ends when groups == n or h >= n + 1, whichever is first: with kSaFirstBases = 30 at most 32 rounds whatever
// the kernels compute.  Groups left at that point are a bug and an error, never a longer loop.
//
// From the order: the BWT symbol of row i is text[sa[i] - 1]; sa_bwt_kernel packs the two bit planes of 32 rows with
// wave ballots (lane 0 and lane 32 of a wave each write one block's planes) and counts the symbols per block,
// prims::exclusive_sum_u32 turns the counts into "symbols before the block", sa_occ_kernel writes every block's cnt[4]
// and the superblock words, sa_rows_kernel the 8-byte rows.  Every output word has exactly one writer.
#include "sa_build.hpp"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <vector>

#include "prims.hpp"

namespace mrg {

namespace {

constexpr uint32_t kThreads = 256u;

// code of text base q
__device__ __forceinline__ uint32_t base_at(const uint32_t* __restrict__ text, uint32_t q) { return (text[q >> 4] >> ((q & 15u) * 2u)) & 3u; }

// (position, key) of the suffixes in descending position order; text has at least (p >> 4) + 3 words for every p < n
__global__ void __launch_bounds__(kThreads) sa_first_keys_kernel(const uint32_t* __restrict__ text, uint32_t n, uint64_t* __restrict__ keys,
                                                                 uint32_t* __restrict__ vals) {
  const uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (j >= n) return;
  const uint32_t p = n - 1u - (uint32_t)j;
  const uint32_t w = p >> 4, sh = (p & 15u) * 2u;
  const uint64_t lo = (uint64_t)text[w] | ((uint64_t)text[w + 1u] << 32), t2 = text[w + 2u];
  uint64_t win = sh ? (lo >> sh) | (t2 << (64u - sh)) : lo;
  win &= (1ull << (2u * kSaFirstBases)) - 1ull;
  // first base most significant: reverse all bits, then put the two bits of every base back in order
  uint64_t r = __brevll(win);
  r = ((r >> 1) & 0x5555555555555555ull) | ((r & 0x5555555555555555ull) << 1);
  keys[j] = r >> (64u - 2u * kSaFirstBases);
  vals[j] = p;
}

__global__ void __launch_bounds__(kThreads) sa_first_heads_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                                  uint32_t n, uint32_t* __restrict__ head) {
  const uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (j >= n) return;
  bool h = true;
  if (j) {
    const bool short_here = (uint64_t)vals[j] + kSaFirstBases > n, short_prev = (uint64_t)vals[j - 1] + kSaFirstBases > n;
    h = keys[j] != keys[j - 1] || short_here || short_prev;
  }
  head[j] = h ? 1u : 0u;
}

__global__ void __launch_bounds__(kThreads) sa_heads_kernel(const uint64_t* __restrict__ keys, uint32_t n, uint32_t* __restrict__ head) {
  const uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (j >= n) return;
  head[j] = (j == 0 || keys[j] != keys[j - 1]) ? 1u : 0u;
}

__global__ void __launch_bounds__(kThreads) sa_rank_scatter_kernel(const uint32_t* __restrict__ vals, const uint32_t* __restrict__ incl,
                                                                   uint32_t n, uint32_t* __restrict__ rank) {
  const uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (j >= n) return;
  const uint32_t p = vals[j];
  if (p < n) rank[p] = incl[j];
}

__global__ void __launch_bounds__(kThreads) sa_next_keys_kernel(const uint32_t* __restrict__ vals, const uint32_t* __restrict__ incl,
                                                                const uint32_t* __restrict__ rank, uint32_t n, uint64_t h, uint32_t bits,
                                                                uint64_t* __restrict__ keys) {
  const uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (j >= n) return;
  const uint64_t q = (uint64_t)vals[j] + h;
  const uint64_t second = q < n ? rank[q] : 0u;
  keys[j] = ((uint64_t)incl[j] << bits) | second;
}

// text position of row i: the sentinel's in row 0, order[i - 1] behind it
__device__ __forceinline__ uint32_t row_pos(const uint32_t* __restrict__ order, uint32_t n, uint32_t i) { return i ? order[i - 1u] : n; }

// one thread per row of nblk * 32 rows (rows >= m hold nothing); no thread leaves before the ballots
__global__ void __launch_bounds__(kThreads) sa_bwt_kernel(const uint32_t* __restrict__ order, const uint32_t* __restrict__ text, uint32_t n,
                                                          uint32_t nblk, uint32_t* __restrict__ blocks, uint32_t* __restrict__ counts,
                                                          uint32_t* __restrict__ primary) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  const uint64_t m = (uint64_t)n + 1u;
  const bool row = i < m;
  uint32_t p = row ? row_pos(order, n, (uint32_t)i) : 0u;
  if (p > n) p = 0u;  // (cannot be: order holds text positions)
  const bool sym = row && p != 0u;
  const uint32_t c = sym ? base_at(text, p - 1u) : 0u;
  if (row && p == 0u) *primary = (uint32_t)i;
  const uint64_t lo = __ballot(sym && (c & 1u)), hi = __ballot(sym && (c & 2u)), any = __ballot(sym);
  const uint32_t lane = threadIdx.x & 63u;
  if ((lane & 31u) == 0u) {
    const uint64_t blk = i >> 5;
    if (blk < nblk) {
      const uint32_t sh = lane;  // 0 or 32
      const uint32_t l = (uint32_t)(lo >> sh), h = (uint32_t)(hi >> sh), a = (uint32_t)(any >> sh);
      blocks[4u * blk + 2u] = l;
      blocks[4u * blk + 3u] = h;
      counts[0ull * nblk + blk] = __popc(a & ~l & ~h);
      counts[1ull * nblk + blk] = __popc(a & l & ~h);
      counts[2ull * nblk + blk] = __popc(a & ~l & h);
      counts[3ull * nblk + blk] = __popc(a & l & h);
    }
  }
}

// before[c * nblk + b] = symbols c in the rows before block b
__global__ void __launch_bounds__(kThreads) sa_occ_kernel(const uint32_t* __restrict__ before, uint32_t nblk, uint32_t nsup, uint32_t c0,
                                                          uint32_t c1, uint32_t c2, uint32_t c3, uint32_t* __restrict__ blocks,
                                                          uint32_t* __restrict__ super) {
  const uint64_t b = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (b >= nblk) return;
  constexpr uint32_t kPerSuper = 1u << (kSuperShift - 5u);
  const uint64_t sb = b & ~(uint64_t)(kPerSuper - 1u);
  const uint32_t C[4] = {c0, c1, c2, c3};
  uint32_t rel[4];
#pragma unroll
  for (uint32_t c = 0; c < 4u; ++c) {
    const uint32_t run = before[(uint64_t)c * nblk + b];
    rel[c] = (run - before[(uint64_t)c * nblk + sb]) & 0xFFFFu;
    if (b == sb && (b >> (kSuperShift - 5u)) < nsup) super[4u * (b >> (kSuperShift - 5u)) + c] = C[c] + run;
  }
  blocks[4u * b] = rel[0] | (rel[1] << 16);
  blocks[4u * b + 1u] = rel[2] | (rel[3] << 16);
}

__global__ void __launch_bounds__(kThreads) sa_rows_kernel(const uint32_t* __restrict__ order, uint32_t n, const uint32_t* __restrict__ seg_start,
                                                           const uint32_t* __restrict__ chunk_seg, uint32_t nseg, uint64_t* __restrict__ rows) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i > n) return;
  const uint32_t p = row_pos(order, n, (uint32_t)i);
  uint64_t row = p;
  if (p < n && nseg) {
    uint32_t sg = chunk_seg[p >> 5];
    if (sg >= nseg) sg = nseg - 1u;
    while (sg + 1u < nseg && seg_start[sg + 1u] <= p) ++sg;
    const uint32_t before = min(255u, p - seg_start[sg]), after = min(255u, seg_start[sg + 1u] - p);
    const uint32_t sid = nseg <= 0xFFFFu ? sg : 0xFFFFu;
    row |= (uint64_t)before << 32 | (uint64_t)after << 40 | (uint64_t)sid << 48;
  } else {
    row |= (uint64_t)0xFFFFu << 48;
  }
  rows[i] = row;
}

inline uint32_t blocks_for(uint64_t n) { return (uint32_t)((n + kThreads - 1u) / kThreads); }
inline uint64_t align256(uint64_t x) { return (x + 255u) & ~(uint64_t)255u; }

void hip_check(hipError_t e, const char* what) {
  if (e != hipSuccess) throw SaBuildError(std::string("device index build: ") + what + " failed: " + hipGetErrorString(e), false);
}
#define SA_TRY(expr) hip_check((expr), #expr)

// the buffers of one build, carved from ONE allocation; freed whatever happens
struct Arena {
  char* base = nullptr;
  uint64_t used = 0, size = 0;
  ~Arena() { (void)hipFree(base); }
  template <class T>
  T* take(uint64_t count) {
    T* p = (T*)(base + used);
    used += align256(count * sizeof(T));
    return p;
  }
};

struct Layout {
  uint64_t n, m, nblk, nsup, nseg, text_words, tmp;
  uint64_t total() const {
    return 2 * align256(m * 8) + 2 * align256(n * 4 + 4) + 2 * align256(n * 4 + 4)  // keys, positions, ranks + flags
           + align256(text_words * 4) + align256((nseg + 1) * 4) + align256(((n >> 5) + 2) * 4) + align256(nblk * 16) +
           align256(nblk * 16) + align256(nsup * 16) + align256(tmp) + 256;
  }
};

Layout layout_of(uint32_t n, uint32_t n_seg) {
  Layout L;
  L.n = n;
  L.m = (uint64_t)n + 1;
  L.nblk = (L.m >> 5) + 1;
  L.nsup = (L.m >> kSuperShift) + 1;
  L.nseg = n_seg;
  L.text_words = ((uint64_t)n + 15) / 16 + 4;
  L.tmp = std::max<uint64_t>(prims::radix_temp_bytes(L.m), std::max<uint64_t>(prims::scan_temp_bytes(L.m), prims::scan_temp_bytes(L.nblk)));
  return L;
}

}  // namespace

uint64_t sa_build_device_bytes(uint32_t n, uint32_t n_seg) { return layout_of(n, n_seg).total(); }

void build_rows_device(FmIndex& ix, uint32_t* rounds_out) {
  StageTimer tm("build_index (device)");
  const uint32_t n = ix.n, nseg = (uint32_t)ix.seg_ref.size();
  const Layout L = layout_of(n, nseg);
  if (ix.text.size() != L.text_words || ix.seg_start.size() != L.nseg + 1 || ix.chunk_seg.size() != (size_t)(n >> 5) + 2)
    throw SaBuildError("device index build: the host arrays are not final", false);
  const uint64_t need = L.total();
  size_t free_b = 0, total_b = 0;
  SA_TRY(hipMemGetInfo(&free_b, &total_b));
  if (need > free_b) {
    char msg[256];
    std::snprintf(msg, sizeof msg, "device index build: %llu bytes of device memory needed for %u bases, %llu free",
                  (unsigned long long)need, n, (unsigned long long)free_b);
    throw SaBuildError(msg, true);
  }
  Arena A;
  {
    hipError_t e = hipMalloc((void**)&A.base, need);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      A.base = nullptr;
      char msg[256];
      std::snprintf(msg, sizeof msg, "device index build: cannot allocate the %llu bytes of device memory needed for %u bases (%s)",
                    (unsigned long long)need, n, hipGetErrorString(e));
      throw SaBuildError(msg, true);
    }
    A.size = need;
  }
  uint64_t* keys[2] = {A.take<uint64_t>(L.m), A.take<uint64_t>(L.m)};
  uint32_t* vals[2] = {A.take<uint32_t>(L.n + 1), A.take<uint32_t>(L.n + 1)};
  uint32_t* rank = A.take<uint32_t>(L.n + 1);
  uint32_t* flag = A.take<uint32_t>(L.n + 1);
  uint32_t* d_text = A.take<uint32_t>(L.text_words);
  uint32_t* d_seg_start = A.take<uint32_t>(L.nseg + 1);
  uint32_t* d_chunk_seg = A.take<uint32_t>((L.n >> 5) + 2);
  uint32_t* d_blocks = A.take<uint32_t>(L.nblk * 4);
  uint32_t* d_counts = A.take<uint32_t>(L.nblk * 4);
  uint32_t* d_super = A.take<uint32_t>(L.nsup * 4);
  void* tmp = A.take<char>(L.tmp);
  uint32_t* d_primary = A.take<uint32_t>(1);
  if (A.used > A.size) throw SaBuildError("device index build: buffer layout exceeds its allocation", false);

  hipStream_t stream = nullptr;
  SA_TRY(hipMemcpy(d_text, ix.text.data(), L.text_words * 4, hipMemcpyHostToDevice));
  SA_TRY(hipMemcpy(d_seg_start, ix.seg_start.data(), (L.nseg + 1) * 4, hipMemcpyHostToDevice));
  SA_TRY(hipMemcpy(d_chunk_seg, ix.chunk_seg.data(), ((L.n >> 5) + 2) * 4, hipMemcpyHostToDevice));
  tm.lap("upload");

  uint32_t cur = 0, rounds = 0;  // the sorted pairs are in keys[cur] / vals[cur]
  if (n) {
    const uint32_t grid = blocks_for(n);
    hipLaunchKernelGGL(sa_first_keys_kernel, dim3(grid), dim3(kThreads), 0, stream, d_text, n, keys[0], vals[0]);
    SA_TRY(hipGetLastError());
    bool second = false;
    SA_TRY(prims::radix_sort_pairs_u64(keys[0], keys[1], vals[0], vals[1], n, 2u * kSaFirstBases, tmp, stream, &second));
    cur = second ? 1u : 0u;
    rounds = 1;
    uint64_t h = kSaFirstBases;
    char lap[64];
    for (;;) {
      if (rounds == 1)
        hipLaunchKernelGGL(sa_first_heads_kernel, dim3(grid), dim3(kThreads), 0, stream, keys[cur], vals[cur], n, flag);
      else
        hipLaunchKernelGGL(sa_heads_kernel, dim3(grid), dim3(kThreads), 0, stream, keys[cur], n, flag);
      SA_TRY(hipGetLastError());
      SA_TRY(prims::inclusive_sum_u32(flag, flag, n, tmp, stream));
      uint32_t groups = 0;
      SA_TRY(hipMemcpyAsync(&groups, flag + (n - 1u), 4, hipMemcpyDeviceToHost, stream));
      SA_TRY(hipStreamSynchronize(stream));
      std::snprintf(lap, sizeof lap, "sort round %u (width %llu, %u groups)", rounds, (unsigned long long)h, groups);
      tm.lap(lap);
      if (groups >= n) break;
      if (h >= (uint64_t)n + 1u) {
        char msg[160];
        std::snprintf(msg, sizeof msg, "device index build: %u of %u suffixes still tied after %u rounds (internal error)", n - groups, n,
                      rounds);
        throw SaBuildError(msg, false);
      }
      uint32_t bits = 1;
      while (bits < 32u && (groups >> bits)) ++bits;
      hipLaunchKernelGGL(sa_rank_scatter_kernel, dim3(grid), dim3(kThreads), 0, stream, vals[cur], flag, n, rank);
      SA_TRY(hipGetLastError());
      hipLaunchKernelGGL(sa_next_keys_kernel, dim3(grid), dim3(kThreads), 0, stream, vals[cur], flag, rank, n, h, bits, keys[cur]);
      SA_TRY(hipGetLastError());
      SA_TRY(prims::radix_sort_pairs_u64(keys[cur], keys[cur ^ 1u], vals[cur], vals[cur ^ 1u], n, 2u * bits, tmp, stream, &second));
      if (second) cur ^= 1u;
      h *= 2;
      ++rounds;
    }
  }
  const uint32_t* order = vals[cur];

  // BWT blocks, superblocks, primary
  hipLaunchKernelGGL(sa_bwt_kernel, dim3(blocks_for(L.nblk * 32)), dim3(kThreads), 0, stream, order, d_text, n, (uint32_t)L.nblk, d_blocks,
                     d_counts, d_primary);
  SA_TRY(hipGetLastError());
  for (uint32_t c = 0; c < 4; ++c)
    SA_TRY(prims::exclusive_sum_u32(d_counts + c * L.nblk, d_counts + c * L.nblk, L.nblk, tmp, stream));
  hipLaunchKernelGGL(sa_occ_kernel, dim3(blocks_for(L.nblk)), dim3(kThreads), 0, stream, d_counts, (uint32_t)L.nblk, (uint32_t)L.nsup, ix.C[0],
                     ix.C[1], ix.C[2], ix.C[3], d_blocks, d_super);
  SA_TRY(hipGetLastError());
  SA_TRY(hipStreamSynchronize(stream));
  tm.lap("bwt");

  // 8-byte rows, into a key buffer: both are free once the order stands
  uint64_t* d_rows = keys[0];
  hipLaunchKernelGGL(sa_rows_kernel, dim3(blocks_for(L.m)), dim3(kThreads), 0, stream, order, n, d_seg_start, d_chunk_seg, nseg, d_rows);
  SA_TRY(hipGetLastError());
  SA_TRY(hipStreamSynchronize(stream));
  tm.lap("rows");

  std::vector<OccBlock> blocks(L.nblk);
  std::vector<uint32_t> super(L.nsup * 4);
  std::vector<uint64_t> sa(L.m);
  uint32_t primary = 0;
  SA_TRY(hipMemcpy(blocks.data(), d_blocks, L.nblk * 16, hipMemcpyDeviceToHost));
  SA_TRY(hipMemcpy(super.data(), d_super, L.nsup * 16, hipMemcpyDeviceToHost));
  SA_TRY(hipMemcpy(sa.data(), d_rows, L.m * 8, hipMemcpyDeviceToHost));
  SA_TRY(hipMemcpy(&primary, d_primary, 4, hipMemcpyDeviceToHost));
  tm.lap("download");
  ix.blocks.swap(blocks);
  ix.super.swap(super);
  ix.sa.swap(sa);
  ix.primary = primary;
  if (rounds_out) *rounds_out = rounds;
}

}  // namespace mrg
