// Predict mode's candidate reads on the device (mrg_predict_select / mrg_predict_sample_reads / mrg_predict_gather,
// include/mirge_amd.h): the flags and `mir<k>` numbers of convert2Fasta.py's raw and filtered lists, one sample's rows of a
// list, and a list as a compact packed read set.  gfx950, wave64, no LDS; one lane per read or row, except the flags of wide
// quant rows (S >= kPredictWideS), which 16 neighbouring lanes sum together.  The scans are prims::exclusive_sum_u32, called
// from capi.hip between these kernels.
#include "predict_reads.hpp"

namespace mrg {

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kRowLanes = 16;  // lanes per read of the wide layout

inline uint32_t grid_for(uint64_t n) { return (uint32_t)((n + kThreads - 1) / kThreads); }

__device__ inline void store_flags(const PredictSelectParams& p, uint32_t u, uint64_t sum, uint64_t* __restrict__ total,
                                   uint32_t* __restrict__ raw, uint32_t* __restrict__ sel) {
  uint32_t r = 0, f = 0;
  if (u < p.n) {
    total[u] = sum;
    if (p.pass_id[u] < 0) {
      const uint32_t len = p.lens[u];
      r = sum >= 1 ? 1u : 0u;
      f = (len >= p.min_len && len <= p.max_len && sum >= p.cutoff) ? 1u : 0u;
    }
  }
  raw[u] = r;  // (u <= n: the caller)
  sel[u] = f;
}

__global__ __launch_bounds__(kThreads) void predict_flags_kernel(PredictSelectParams p, uint64_t* __restrict__ total,
                                                                 uint32_t* __restrict__ raw, uint32_t* __restrict__ sel) {
  const uint32_t u = blockIdx.x * kThreads + threadIdx.x;  // (n + 1 lanes)
  if (u > p.n) return;
  uint64_t sum = 0;
  if (u < p.n) {
    const uint32_t* row = p.quant + (uint64_t)u * p.S;
    for (uint32_t c = 0; c < p.S; ++c) sum += row[c];
  }
  store_flags(p, u, sum, total, raw, sel);
}

__global__ __launch_bounds__(kThreads) void predict_flags_wide_kernel(PredictSelectParams p, uint64_t* __restrict__ total,
                                                                      uint32_t* __restrict__ raw, uint32_t* __restrict__ sel) {
  const uint32_t u = blockIdx.x * (kThreads / kRowLanes) + threadIdx.x / kRowLanes;  // (n + 1 rows of 16 lanes)
  const uint32_t lane = threadIdx.x % kRowLanes;
  uint64_t sum = 0;
  if (u < p.n) {
    const uint32_t* row = p.quant + (uint64_t)u * p.S;
    for (uint32_t c = lane; c < p.S; c += kRowLanes) sum += row[c];
  }
  for (int d = kRowLanes / 2; d; d >>= 1) sum += __shfl_xor(sum, d, 64);  // (every lane of the wave is here)
  if (lane == 0 && u <= p.n) store_flags(p, u, sum, total, raw, sel);
}

__global__ __launch_bounds__(kThreads) void predict_numbers_kernel(const uint32_t* __restrict__ raw_scan,
                                                                   const uint32_t* __restrict__ sel_scan, uint32_t n,
                                                                   uint32_t* __restrict__ raw_no, uint32_t* __restrict__ sel_no) {
  const uint32_t u = blockIdx.x * kThreads + threadIdx.x;
  if (u >= n) return;
  const uint32_t r = raw_scan[u], f = sel_scan[u];
  raw_no[u] = raw_scan[u + 1] != r ? r + 1 : 0;
  sel_no[u] = sel_scan[u + 1] != f ? f + 1 : 0;
}

__global__ __launch_bounds__(kThreads) void predict_sample_flags_kernel(const uint32_t* __restrict__ quant,
                                                                        const uint32_t* __restrict__ no, uint32_t n, uint32_t S,
                                                                        uint32_t s, uint64_t threshold, uint32_t* __restrict__ flags) {
  const uint32_t u = blockIdx.x * kThreads + threadIdx.x;  // (n + 1 lanes)
  if (u > n) return;
  uint32_t f = 0;
  if (u < n && no[u]) f = (uint64_t)quant[(uint64_t)u * S + s] >= threshold ? 1u : 0u;
  flags[u] = f;
}

__global__ __launch_bounds__(kThreads) void predict_sample_fill_kernel(const uint32_t* __restrict__ scan,
                                                                       const uint32_t* __restrict__ quant,
                                                                       const uint32_t* __restrict__ no, uint32_t n, uint32_t S,
                                                                       uint32_t s, uint32_t* __restrict__ idx, uint32_t* __restrict__ num,
                                                                       uint32_t* __restrict__ cnt) {
  const uint32_t u = blockIdx.x * kThreads + threadIdx.x;
  if (u >= n) return;
  const uint32_t at = scan[u];
  if (scan[u + 1] == at) return;
  // (at < scan[n], which the caller checked against the buffers)
  idx[at] = u;
  num[at] = no[u];
  cnt[at] = quant[(uint64_t)u * S + s];
}

__global__ __launch_bounds__(kThreads) void predict_gather_kernel(PredictGatherParams p, uint32_t* __restrict__ stat) {
  const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
  if (j >= p.k) return;
  const uint32_t u = p.idx[j];
  bool ok = u < p.n;
  uint32_t len = 0;
  uint64_t count = 0;
  if (!ok) {
    atomicOr(&stat[kPredictStatBadIndex], 1u);
  } else {
    len = p.lens[u];
    if (len > 32u * p.W) {
      atomicOr(&stat[kPredictStatTooLong], 1u);
      ok = false;
    }
  }
  if (ok) {
    const uint32_t* row = p.quant + (uint64_t)u * p.S;
    if (p.sample == kPredictTotalAll) {
      for (uint32_t c = 0; c < p.S; ++c) count += row[c];
    } else {
      count = row[p.sample];
    }
    if (count >> 32) {
      atomicOr(&stat[kPredictStatOverflow], 1u);
      ok = false;
    }
  }
  for (uint32_t w = 0; w < p.W; ++w) {
    const uint64_t from = (uint64_t)w * p.stride + u, to = (uint64_t)w * p.k + j;
    p.out_reads[to] = ok ? p.reads[from] : 0;
    if (p.out_nmask) p.out_nmask[to] = ok && p.nmask ? p.nmask[from] : 0;
  }
  p.out_lens[j] = ok ? (uint8_t)len : 0;
  p.out_counts[j] = ok ? (uint32_t)count : 0;
}

}  // namespace

hipError_t predict_flags_launch(const PredictSelectParams& p, uint64_t* total, uint32_t* raw, uint32_t* sel, hipStream_t stream) {
  const uint64_t rows = (uint64_t)p.n + 1;
  if (p.S >= kPredictWideS) {
    const uint64_t per_block = kThreads / kRowLanes;
    hipLaunchKernelGGL(predict_flags_wide_kernel, dim3((uint32_t)((rows + per_block - 1) / per_block)), dim3(kThreads), 0, stream, p,
                       total, raw, sel);
  } else {
    hipLaunchKernelGGL(predict_flags_kernel, dim3(grid_for(rows)), dim3(kThreads), 0, stream, p, total, raw, sel);
  }
  return hipGetLastError();
}

hipError_t predict_numbers_launch(const uint32_t* raw_scan, const uint32_t* sel_scan, uint32_t n, uint32_t* raw_no, uint32_t* sel_no,
                                  hipStream_t stream) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(predict_numbers_kernel, dim3(grid_for(n)), dim3(kThreads), 0, stream, raw_scan, sel_scan, n, raw_no, sel_no);
  return hipGetLastError();
}

hipError_t predict_sample_flags_launch(const uint32_t* quant, const uint32_t* no, uint32_t n, uint32_t S, uint32_t s, uint64_t threshold,
                                       uint32_t* flags, hipStream_t stream) {
  hipLaunchKernelGGL(predict_sample_flags_kernel, dim3(grid_for((uint64_t)n + 1)), dim3(kThreads), 0, stream, quant, no, n, S, s,
                     threshold, flags);
  return hipGetLastError();
}

hipError_t predict_sample_fill_launch(const uint32_t* scan, const uint32_t* quant, const uint32_t* no, uint32_t n, uint32_t S, uint32_t s,
                                      uint32_t* idx, uint32_t* num, uint32_t* cnt, hipStream_t stream) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(predict_sample_fill_kernel, dim3(grid_for(n)), dim3(kThreads), 0, stream, scan, quant, no, n, S, s, idx, num, cnt);
  return hipGetLastError();
}

hipError_t predict_gather_launch(const PredictGatherParams& p, uint32_t* stat, hipStream_t stream) {
  if (!p.k) return hipSuccess;
  hipLaunchKernelGGL(predict_gather_kernel, dim3(grid_for(p.k)), dim3(kThreads), 0, stream, p, stat);
  return hipGetLastError();
}

}  // namespace mrg
