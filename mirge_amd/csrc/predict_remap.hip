// Predict mode's second mapping on the device (mrg_predict_trim_reads / mrg_predict_remap_rows, include/mirge_amd.h): the
// reads pass 1 left unaligned as a packed set cut for pass 2, the two listings merged into rows, the rows' sort keys and the
// rows in file order.  gfx950, wave64, no LDS, no atomics: one lane per read (remap_mark_kernel, remap_compact_kernel), per
// output word (remap_trim_kernel) or per row (remap_merge_kernel, the gathers); every output word has one writer and nothing
// depends on lane order.  The stat words are the one exception to "one writer": every lane that finds an input array
// contradicting another stores the same 1 there.  The scan and the two radix sorts between the kernels are prims::, called
// from capi.hip.
#include "predict_remap.hpp"

namespace mrg {

namespace {

constexpr uint32_t kThreads = 256;

inline uint32_t grid_for(uint64_t n) { return (uint32_t)((n + kThreads - 1) / kThreads); }

__global__ __launch_bounds__(kThreads) void remap_mark_kernel(const uint32_t* __restrict__ counts, uint32_t n, uint32_t* __restrict__ flag32) {
  const uint32_t r = blockIdx.x * kThreads + threadIdx.x;  // (n + 1 lanes)
  if (r > n) return;
  if (r == n) {
    flag32[r] = 0;
    return;
  }
  uint32_t any = 0;
#pragma unroll
  for (uint32_t s = 0; s < 4; ++s) any |= counts[(uint64_t)s * n + r];
  flag32[r] = any ? 0u : 1u;
}

__global__ __launch_bounds__(kThreads) void remap_compact_kernel(uint32_t n, const uint32_t* __restrict__ rank, uint32_t* __restrict__ sel) {
  const uint32_t r = blockIdx.x * kThreads + threadIdx.x;
  if (r >= n) return;
  const uint32_t at = rank[r];  // (< rank[n] <= n for a marked read: inside sel [n])
  if (rank[r + 1] != at) sel[at] = r;
}

// word w of a read's 64-bit words shifted down by 2 t5 bits: bases [t5 + 32 w, t5 + 32 w + 32) of the read
__device__ __forceinline__ uint64_t shifted_word(const uint64_t* __restrict__ words, uint32_t W, uint64_t stride, uint32_t r, uint32_t w,
                                                 uint32_t t5) {
  const uint32_t ws = w + (t5 >> 5), sh = 2u * (t5 & 31u);
  if (ws >= W) return 0;
  uint64_t v = words[(uint64_t)ws * stride + r] >> sh;
  if (sh && ws + 1 < W) v |= words[(uint64_t)(ws + 1) * stride + r] << (64u - sh);
  return v;
}

__global__ __launch_bounds__(kThreads) void remap_trim_kernel(RemapReads in, const uint32_t* __restrict__ sel, uint32_t k, uint32_t t5,
                                                              uint32_t t3, uint64_t* __restrict__ out_words, uint8_t* __restrict__ out_lens,
                                                              uint64_t* __restrict__ out_nmask) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;  // (k W lanes: word w of output read j at i = w k + j)
  if (i >= (uint64_t)k * in.W) return;
  const uint32_t w = (uint32_t)(i / k), j = (uint32_t)(i - (uint64_t)w * k);
  const uint32_t r = sel[j];
  uint32_t len = 0;
  uint64_t bits = 0, nbits = 0;
  if (r < in.n) {
    const uint32_t full = min((uint32_t)in.lens[r], 32u * in.W);
    len = full > t5 + t3 ? full - t5 - t3 : 0u;
    const uint32_t nb = len > 32u * w ? min(len - 32u * w, 32u) : 0u;  // bases of the cut read in this word
    if (nb) {
      const uint64_t keep = nb == 32u ? ~0ull : (1ull << (2u * nb)) - 1ull;
      bits = shifted_word(in.words, in.W, in.stride, r, w, t5) & keep;
      if (in.nmask) nbits = shifted_word(in.nmask, in.W, in.stride, r, w, t5) & keep;
    }
  }
  out_words[i] = bits;
  if (in.nmask) out_nmask[i] = nbits;
  if (w == 0) out_lens[j] = (uint8_t)len;
}

// the decimal digits of v (< 10^10) from bit 39 down, four bits each, the rest filled with 15
__device__ __forceinline__ uint64_t digits_key(uint64_t v) {
  uint32_t d = 1;
  for (uint64_t p = 10; d < 10 && v >= p; p *= 10) ++d;
  uint64_t key = d < 10 ? (1ull << (4u * (10u - d))) - 1ull : 0ull;
  for (uint32_t at = 10u - d; at < 10u; ++at) {  // the last digit first
    key |= (v % 10) << (4u * at);
    v /= 10;
  }
  return key;
}

// the read r < n with off[r] <= x < off[r + 1] (n >= 1); false when the offsets do not say so
__device__ __forceinline__ bool owner_of_row(const uint64_t* __restrict__ off, uint32_t n, uint64_t x, uint32_t* owner) {
  uint32_t lo = 0, hi = n;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (off[mid] <= x) lo = mid;
    else hi = mid;
  }
  *owner = lo;
  return off[lo] <= x && x < off[lo + 1];
}

__global__ __launch_bounds__(kThreads) void remap_merge_kernel(RemapMergeArgs a) {
  const uint32_t t = blockIdx.x * kThreads + threadIdx.x;
  const uint32_t total = a.p1.rows + a.p2.rows;  // (< 2^32 - 1: the caller checked)
  if (t == 0) {
    if (a.p1.n && (a.p1.off[0] != 0 || a.p1.off[a.p1.n] != a.p1.rows)) a.stat[kRemapStatBadOffsets] = 1u;
    if (a.p2.n && (a.p2.off[0] != 0 || a.p2.off[a.p2.n] != a.p2.rows)) a.stat[kRemapStatBadOffsets] = 1u;
  }
  // (the grid covers the reads of both listings too: lane t looks at read t's range)
  if (t < a.p1.n && a.p1.off[t] > a.p1.off[t + 1]) a.stat[kRemapStatBadOffsets] = 1u;
  if (t < a.p2.n && a.p2.off[t] > a.p2.off[t + 1]) a.stat[kRemapStatBadOffsets] = 1u;
  if (t >= total) return;
  const bool second = t >= a.p1.rows;
  const RemapListing& p = second ? a.p2 : a.p1;
  const uint32_t x = second ? t - a.p1.rows : t;
  uint32_t read = 0, cluster = 0, offset = 0, mm = 0;
  bool good = p.n != 0 && owner_of_row(p.off, p.n, x, &read);
  if (!good) a.stat[kRemapStatBadOffsets] = 1u;
  if (good && second) {
    read = a.sel[read];
    if (read >= a.n_reads) {
      a.stat[kRemapStatBadRead] = 1u;
      good = false;
    }
  }
  if (good) {
    const int32_t ref = p.ref[x], pos = p.pos[x];
    if (ref < 0 || (uint32_t)ref >= a.n_clusters || pos < 0) {
      a.stat[kRemapStatBadCluster] = 1u;
      good = false;
    } else {
      cluster = (uint32_t)ref;
      offset = (uint32_t)pos;
      mm = p.mm[x];
    }
  }
  if (!good) read = cluster = 0;
  a.rows.read[t] = read;
  a.rows.cluster[t] = cluster;
  a.rows.offset[t] = offset;
  a.rows.mm[t] = (uint8_t)mm;
  a.rows.pass[t] = second ? 1 : 0;
  a.read_key[t] = good ? digits_key(a.numbers[read]) : 0ull;
  a.cluster_key[t] = good ? digits_key((uint64_t)a.kept[cluster] + 1ull) : 0ull;
  a.vals[t] = t;
}

__global__ __launch_bounds__(kThreads) void remap_gather_keys_kernel(const uint64_t* __restrict__ in, const uint32_t* __restrict__ vals,
                                                                     uint32_t rows, uint64_t* __restrict__ out) {
  const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
  if (j >= rows) return;
  const uint32_t v = vals[j];
  out[j] = v < rows ? in[v] : 0ull;
}

__global__ __launch_bounds__(kThreads) void remap_gather_rows_kernel(RemapRows in, const uint32_t* __restrict__ vals, uint32_t rows,
                                                                     RemapRows out) {
  const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
  if (j >= rows) return;
  const uint32_t v = min(vals[j], rows - 1u);  // (a permutation of [0, rows): the clamp only keeps a broken one inside)
  out.read[j] = in.read[v];
  out.cluster[j] = in.cluster[v];
  out.offset[j] = in.offset[v];
  out.mm[j] = in.mm[v];
  out.pass[j] = in.pass[v];
}

}  // namespace

hipError_t remap_mark_launch(const uint32_t* counts, uint32_t n, uint32_t* flag32, hipStream_t stream) {
  hipLaunchKernelGGL(remap_mark_kernel, dim3(grid_for((uint64_t)n + 1)), dim3(kThreads), 0, stream, counts, n, flag32);
  return hipGetLastError();
}

hipError_t remap_compact_launch(uint32_t n, const uint32_t* rank, uint32_t* sel, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(remap_compact_kernel, dim3(grid_for(n)), dim3(kThreads), 0, stream, n, rank, sel);
  return hipGetLastError();
}

hipError_t remap_trim_launch(const RemapReads& in, const uint32_t* sel, uint32_t k, uint32_t t5, uint32_t t3, uint64_t* out_words,
                             uint8_t* out_lens, uint64_t* out_nmask, hipStream_t stream) {
  if (k == 0 || in.W == 0) return hipSuccess;
  hipLaunchKernelGGL(remap_trim_kernel, dim3(grid_for((uint64_t)k * in.W)), dim3(kThreads), 0, stream, in, sel, k, t5, t3, out_words, out_lens,
                     out_nmask);
  return hipGetLastError();
}

hipError_t remap_merge_launch(const RemapMergeArgs& a, hipStream_t stream) {
  uint64_t lanes = (uint64_t)a.p1.rows + a.p2.rows;  // one per row and at least one per read of either listing
  if (lanes < a.p1.n) lanes = a.p1.n;
  if (lanes < a.p2.n) lanes = a.p2.n;
  hipLaunchKernelGGL(remap_merge_kernel, dim3(grid_for(lanes ? lanes : 1)), dim3(kThreads), 0, stream, a);
  return hipGetLastError();
}

hipError_t remap_gather_keys_launch(const uint64_t* in, const uint32_t* vals, uint32_t rows, uint64_t* out, hipStream_t stream) {
  if (rows == 0) return hipSuccess;
  hipLaunchKernelGGL(remap_gather_keys_kernel, dim3(grid_for(rows)), dim3(kThreads), 0, stream, in, vals, rows, out);
  return hipGetLastError();
}

hipError_t remap_gather_rows_launch(const RemapRows& in, const uint32_t* vals, uint32_t rows, const RemapRows& out, hipStream_t stream) {
  if (rows == 0) return hipSuccess;
  hipLaunchKernelGGL(remap_gather_rows_kernel, dim3(grid_for(rows)), dim3(kThreads), 0, stream, in, vals, rows, out);
  return hipGetLastError();
}

}  // namespace mrg
