// `-tcf` on the device (mrg_seq_rank / mrg_collapsed_order, include/mirge_amd.h): the rank of every packed read in Python
// string order, and per sample column the reads with a count ordered by (count, rank) descending -- the line pairs of
// <sample>.trim.collapse.fa.  gfx950, wave64; one lane per read everywhere, no LDS.  The sorts are prims::radix_sort_pairs_u64
// and the compaction prims::exclusive_sum_u32, called from capi.hip between these kernels.
#include "collapsed_order.hpp"

namespace mrg {

namespace {

constexpr uint32_t kThreads = 256;

inline uint32_t grid_for(uint64_t n) { return (uint32_t)((n + kThreads - 1) / kThreads); }

__device__ inline uint32_t wave_max(uint32_t v) {
  for (int d = 32; d; d >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, d, 64));
  return v;
}

__global__ __launch_bounds__(kThreads) void seq_iota_kernel(uint32_t* __restrict__ vals, uint32_t n) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i < n) vals[i] = i;
}

__global__ __launch_bounds__(kThreads) void seq_chunk_keys_kernel(SeqRankParams p, const uint32_t* __restrict__ perm, uint32_t chunk,
                                                                  uint64_t* __restrict__ keys, uint32_t* __restrict__ stat) {
  const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
  if (j >= p.n) return;
  const uint32_t read = perm[j];
  uint64_t key = 0;
  const uint32_t pos0 = kSeqChunkBases * chunk, width = min(kSeqChunkBases, p.max_len - pos0);  // (the caller: pos0 < max_len)
  if (read < p.n) {
    uint32_t len = p.lens[read];
    const uint32_t limit = min(p.max_len, 32u * p.W);
    if (len > limit) {  // nothing beyond the words is read; the call fails on the flag
      atomicOr(&stat[kSeqStatTooLong], 1u);
      len = limit;
    }
    if (pos0 < len) {
      // a window of the 32 bases from pos0 on: the word that holds pos0 (pos0 < len <= 32 W) and the next
      const uint32_t w0 = pos0 >> 5, sh = (pos0 & 31) * 2;
      const uint64_t at = (uint64_t)w0 * p.stride + read;
      const bool more = w0 + 1 < p.W;
      const uint64_t lo = p.reads[at], hi = more ? p.reads[at + p.stride] : 0;
      const uint64_t nlo = p.nmask ? p.nmask[at] : 0, nhi = p.nmask && more ? p.nmask[at + p.stride] : 0;
      const uint64_t code = (lo >> sh) | (sh ? hi << (64 - sh) : 0), isn = (nlo >> sh) | (sh ? nhi << (64 - sh) : 0);
      const uint32_t nb = min(kSeqChunkBases, len - pos0);  // bases at and beyond the length order nothing
#pragma unroll
      for (uint32_t b = 0; b < kSeqChunkBases; ++b) {
        uint64_t c = 0;
        if (b < nb) {
          const uint32_t two = (uint32_t)(code >> (2 * b)) & 3u;
          c = ((isn >> (2 * b)) & 1ull) ? 4 : two == 3 ? 5 : two + 1;
        }
        key |= c << (3 * (kSeqChunkBases - 1 - b));
      }
      key >>= 3 * (kSeqChunkBases - width);  // (b >= width holds zeros: the chunk ends at max_len)
    }
  }
  keys[j] = key;
}

__global__ __launch_bounds__(kThreads) void seq_rank_scatter_kernel(const uint32_t* __restrict__ perm, uint32_t n, uint32_t* __restrict__ rank) {
  const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
  if (j >= n) return;
  const uint32_t read = perm[j];
  if (read < n) rank[read] = j;
}

__global__ __launch_bounds__(kThreads) void collapsed_flags_kernel(const uint32_t* __restrict__ quant, uint32_t n, uint32_t S, uint32_t s,
                                                                   uint32_t* __restrict__ flags, uint32_t* __restrict__ stat) {
  const uint32_t u = blockIdx.x * kThreads + threadIdx.x;  // (n + 1 lanes)
  uint32_t count = 0;
  if (u < n) count = quant[(uint64_t)u * S + s];
  if (u <= n) flags[u] = count ? 1u : 0u;
  const uint32_t top = wave_max(count);
  if ((threadIdx.x & 63) == 0 && top) atomicMax(&stat[kSeqStatMaxCount], top);
}

__global__ __launch_bounds__(kThreads) void collapsed_keys_kernel(const uint32_t* __restrict__ scan, const uint32_t* __restrict__ quant,
                                                                  uint32_t n, uint32_t S, uint32_t s, const uint32_t* __restrict__ rank,
                                                                  uint32_t rank_bits, uint64_t* __restrict__ keys,
                                                                  uint32_t* __restrict__ vals) {
  const uint32_t u = blockIdx.x * kThreads + threadIdx.x;
  if (u >= n) return;
  const uint32_t at = scan[u];
  if (scan[u + 1] == at) return;
  // (at < scan[n] <= n: inside the buffers.  A rank that is no rank of n reads is cut to its bits: a wrong order, no more)
  const uint64_t low = rank_bits ? (uint64_t)rank[u] & ((1ull << rank_bits) - 1) : 0;
  keys[at] = ((uint64_t)quant[(uint64_t)u * S + s] << rank_bits) | low;
  vals[at] = u;
}

__global__ __launch_bounds__(kThreads) void collapsed_reverse_kernel(const uint32_t* __restrict__ vals, uint32_t k, uint32_t* __restrict__ order) {
  const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
  if (j < k) order[j] = vals[k - 1 - j];
}

}  // namespace

hipError_t seq_iota_launch(uint32_t* vals, uint32_t n, hipStream_t stream) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(seq_iota_kernel, dim3(grid_for(n)), dim3(kThreads), 0, stream, vals, n);
  return hipGetLastError();
}

hipError_t seq_chunk_keys_launch(const SeqRankParams& p, const uint32_t* perm, uint32_t chunk, uint64_t* keys, uint32_t* stat,
                                 hipStream_t stream) {
  if (!p.n) return hipSuccess;
  if (chunk && (uint64_t)kSeqChunkBases * chunk >= p.max_len) return hipErrorInvalidValue;  // (chunk 0 runs for max_len 0 too)
  hipLaunchKernelGGL(seq_chunk_keys_kernel, dim3(grid_for(p.n)), dim3(kThreads), 0, stream, p, perm, chunk, keys, stat);
  return hipGetLastError();
}

hipError_t seq_rank_scatter_launch(const uint32_t* perm, uint32_t n, uint32_t* rank, hipStream_t stream) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(seq_rank_scatter_kernel, dim3(grid_for(n)), dim3(kThreads), 0, stream, perm, n, rank);
  return hipGetLastError();
}

hipError_t collapsed_flags_launch(const uint32_t* quant, uint32_t n, uint32_t S, uint32_t s, uint32_t* flags, uint32_t* stat,
                                  hipStream_t stream) {
  hipLaunchKernelGGL(collapsed_flags_kernel, dim3(grid_for((uint64_t)n + 1)), dim3(kThreads), 0, stream, quant, n, S, s, flags, stat);
  return hipGetLastError();
}

hipError_t collapsed_keys_launch(const uint32_t* scan, const uint32_t* quant, uint32_t n, uint32_t S, uint32_t s, const uint32_t* rank,
                                 uint32_t rank_bits, uint64_t* keys, uint32_t* vals, hipStream_t stream) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(collapsed_keys_kernel, dim3(grid_for(n)), dim3(kThreads), 0, stream, scan, quant, n, S, s, rank, rank_bits, keys, vals);
  return hipGetLastError();
}

hipError_t collapsed_reverse_launch(const uint32_t* vals, uint32_t k, uint32_t* order, hipStream_t stream) {
  if (!k) return hipSuccess;
  hipLaunchKernelGGL(collapsed_reverse_kernel, dim3(grid_for(k)), dim3(kThreads), 0, stream, vals, k, order);
  return hipGetLastError();
}

}  // namespace mrg
