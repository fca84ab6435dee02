// `-trf` on the device (mrg_trf_sample_groups / mrg_trf_rank, include/mirge_amd.h): from the rows of mrg_trf_classify, the
// packed reads and quant to the row arrays of mrg_trf_rho -- which (row, sample) pairs are items, what each block sums to,
// the reads in Python string order, the printed rows in report order and their layout in the template frame.  gfx950,
// wave64; one lane per pair / row everywhere, no LDS.  The kernels trust what capi.hip has validated (the entry table) and
// check what lives on the device (a row's read, entry and start).
#include "trf_groups.hpp"

#include "trf_tables.hpp"

namespace mrg {

namespace {

constexpr uint32_t kThreads = 256;

inline uint32_t grid_for(uint64_t n) { return (uint32_t)((n + kThreads - 1) / kThreads); }

__device__ inline uint32_t wave_max(uint32_t v) {
  for (int d = 32; d; d >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, d, 64));
  return v;
}

__device__ inline uint64_t keep_mask(uint32_t len, uint32_t w) {  // the bits of word w that lie inside a read of len bases
  const int nb = (int)len - 32 * (int)w;
  return nb >= 32 ? ~0ull : nb <= 0 ? 0ull : (1ull << (2 * nb)) - 1;
}

__global__ __launch_bounds__(kThreads) void trf_items_kernel(TrfGroupParams p, uint32_t* __restrict__ flags, uint64_t* __restrict__ sums,
                                                             uint32_t* __restrict__ printed, int32_t* __restrict__ rep,
                                                             uint32_t* __restrict__ stat) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x, total = (uint64_t)p.S * p.k;
  bool item = false, shown = false, has_n = false;
  uint32_t len = 0;
  if (i < total) {
    const uint32_t s = (uint32_t)(i / p.k), r = (uint32_t)(i % p.k);
    const int32_t* rc = p.rec + (uint64_t)r * kTrfRecInts;
    if ((uint32_t)rc[kTrfRecKind] <= kTrfDele) {
      const uint32_t read = (uint32_t)rc[kTrfRecRead];
      const int32_t entry = rc[kTrfRecEntry], start = rc[kTrfRecStart];
      if (read >= p.n || entry < 0 || (uint32_t)entry >= p.n_entries || start < 0) {
        atomicMin(&stat[kTrfStatBadRow], r);
      } else {
        len = p.lens[read];
        const uint32_t count = p.quant[(uint64_t)read * p.S + s];
        if (count) {
          item = true;
          const int32_t* en = p.entries + (uint64_t)entry * kTrfSampleInts;
          const int32_t tlen = en[kTrfSampleTemplate];
          if (tlen < 0) atomicMin(&stat[kTrfStatNoTemplate], r);
          const uint64_t cell = (uint64_t)s * p.n_names + (uint32_t)en[kTrfSampleName];
          atomicAdd((unsigned long long*)&sums[cell], (unsigned long long)count);
          atomicMin(&rep[cell], entry);
          shown = tlen >= 0 && (int64_t)start + len <= tlen;
          if (shown) {
            atomicAdd(&printed[cell], 1u);
            if (p.nmask)
              for (uint32_t w = 0; w < p.W; ++w) has_n |= (p.nmask[(uint64_t)w * p.stride + read] & keep_mask(len, w)) != 0;
          }
        }
      }
    }
    flags[i] = shown ? 1u : 0u;
  }
  const uint32_t longest = wave_max(len);
  const uint64_t items = __ballot(item), any_n = __ballot(has_n);
  if ((threadIdx.x & 63) == 0) {
    if (longest) atomicMax(&stat[kTrfStatMaxLen], longest);
    if (items) atomicAdd(&stat[kTrfStatItems], (uint32_t)__popcll(items));
    if (any_n) atomicOr(&stat[kTrfStatHasN], 1u);
  }
}

__global__ __launch_bounds__(kThreads) void trf_item_scatter_kernel(const uint32_t* __restrict__ scan, uint64_t total,
                                                                    uint32_t* __restrict__ item) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= total) return;
  const uint32_t at = scan[i];
  if (scan[i + 1] != at) item[at] = (uint32_t)i;
}

__global__ __launch_bounds__(kThreads) void trf_iota_kernel(uint32_t* __restrict__ vals, uint32_t n) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i < n) vals[i] = i;
}

__global__ __launch_bounds__(kThreads) void trf_chunk_keys_kernel(TrfGroupParams p, const uint32_t* __restrict__ vals, uint32_t chunk,
                                                                  uint64_t* __restrict__ keys) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= p.k) return;
  const int32_t* rc = p.rec + (uint64_t)vals[i] * kTrfRecInts;
  const uint32_t read = (uint32_t)rc[kTrfRecRead];
  uint64_t key = 0;
  if ((uint32_t)rc[kTrfRecKind] <= kTrfDele && read < p.n) {
    const uint32_t len = p.lens[read], pos0 = 21 * chunk;
    if (pos0 < len) {
      // a window of the 32 bases from pos0 on: the word that holds pos0 and the next
      const uint32_t w0 = pos0 >> 5, sh = (pos0 & 31) * 2;
      const uint64_t at = (uint64_t)w0 * p.stride + read;
      const bool more = w0 + 1 < p.W;
      const uint64_t lo = p.reads[at], hi = more ? p.reads[at + p.stride] : 0;
      const uint64_t nlo = p.nmask ? p.nmask[at] : 0, nhi = p.nmask && more ? p.nmask[at + p.stride] : 0;
      const uint64_t code = (lo >> sh) | (sh ? hi << (64 - sh) : 0), isn = (nlo >> sh) | (sh ? nhi << (64 - sh) : 0);
      const uint32_t nb = min(21u, len - pos0);
      for (uint32_t b = 0; b < 21; ++b) {
        uint64_t c = 0;
        if (b < nb) {
          const uint32_t two = (uint32_t)(code >> (2 * b)) & 3u;
          c = ((isn >> (2 * b)) & 1ull) ? 4 : two == 3 ? 5 : two + 1;
        }
        key |= c << (3 * (20 - b));
      }
    }
  }
  keys[i] = key;
}

__global__ __launch_bounds__(kThreads) void trf_rank_scatter_kernel(const uint32_t* __restrict__ vals, uint32_t n, uint32_t* __restrict__ rank) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i < n) rank[vals[i]] = i;
}

__global__ __launch_bounds__(kThreads) void trf_order_keys_a_kernel(TrfGroupParams p, const uint32_t* __restrict__ item, uint32_t n_rows,
                                                                    const uint32_t* __restrict__ rank, uint32_t rank_bits,
                                                                    uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
  const uint32_t j = blockIdx.x * kThreads + threadIdx.x;
  if (j >= n_rows) return;
  const uint32_t r = item[j] % p.k;
  const uint32_t start = (uint32_t)p.rec[(uint64_t)r * kTrfRecInts + kTrfRecStart];  // (a printed row: start <= template <= 255)
  keys[j] = ((uint64_t)(255u - min(start, 255u)) << rank_bits) | (uint64_t)(p.k - 1 - rank[r]);
  vals[j] = j;
}

__global__ __launch_bounds__(kThreads) void trf_order_keys_b_kernel(TrfGroupParams p, const uint32_t* __restrict__ item,
                                                                    const uint32_t* __restrict__ vals, uint32_t n_rows,
                                                                    const uint32_t* __restrict__ cell_block, uint64_t* __restrict__ keys) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n_rows) return;
  const uint32_t pair = item[vals[i]], s = pair / p.k, r = pair % p.k;
  const int32_t* rc = p.rec + (uint64_t)r * kTrfRecInts;
  const uint32_t read = (uint32_t)rc[kTrfRecRead];
  const uint32_t name = (uint32_t)p.entries[(uint64_t)rc[kTrfRecEntry] * kTrfSampleInts + kTrfSampleName];
  const uint32_t count = p.quant[(uint64_t)read * p.S + s];
  keys[i] = ((uint64_t)cell_block[(uint64_t)s * p.n_names + name] << 32) | (uint64_t)(~count);
}

// The read shifted by `start` bases into the template frame.  WR (the words of a read) is a template argument and both
// loops are unrolled, so the read stays in registers: word j of the frame takes read word j - start / 32 and the one before.
template <int WR>
__global__ __launch_bounds__(kThreads) void trf_pack_kernel(TrfGroupParams p, const uint32_t* __restrict__ item,
                                                            const uint32_t* __restrict__ vals, uint32_t n_rows,
                                                            const uint64_t* __restrict__ denom, TrfPackOut out) {
  const uint32_t row = blockIdx.x * kThreads + threadIdx.x;
  if (row >= n_rows) return;
  const uint32_t pair = item[vals[row]], s = pair / p.k, r = pair % p.k;
  const int32_t* rc = p.rec + (uint64_t)r * kTrfRecInts;
  const uint32_t read = (uint32_t)rc[kTrfRecRead], start = (uint32_t)rc[kTrfRecStart], len = p.lens[read];
  const uint32_t count = p.quant[(uint64_t)read * p.S + s];
  uint64_t rd[WR], nm[WR];
#pragma unroll
  for (int w = 0; w < WR; ++w) {
    const uint64_t keep = keep_mask(len, (uint32_t)w);
    nm[w] = p.nmask ? p.nmask[(uint64_t)w * p.stride + read] & keep & 0x5555555555555555ull : 0;
    rd[w] = p.reads[(uint64_t)w * p.stride + read] & keep & ~(nm[w] | (nm[w] << 1));
  }
  const int ws = (int)(start >> 5);
  const uint32_t bs = (start & 31) * 2;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if ((uint32_t)j < out.words) {
      uint64_t lo = 0, hi = 0, nlo = 0, nhi = 0;
#pragma unroll
      for (int w = 0; w < WR; ++w) {
        if (w == j - ws) {
          lo = rd[w];
          nlo = nm[w];
        }
        if (w == j - ws - 1) {
          hi = rd[w];
          nhi = nm[w];
        }
      }
      const uint64_t at = (uint64_t)j * out.row_stride + row;
      out.codes[at] = (lo << bs) | (bs ? hi >> (64 - bs) : 0);
      if (out.nmask) out.nmask[at] = (nlo << bs) | (bs ? nhi >> (64 - bs) : 0);
    }
  }
  out.span[row] = (uint16_t)((start + 1) | ((start + len) << 8));
  out.rpm[row] = trf_rp100k_text(count, denom[s]);
  out.row[3ull * row] = r;
  out.row[3ull * row + 1] = count;
  out.row[3ull * row + 2] = (uint32_t)rc[kTrfRecType];
}

__device__ inline uint32_t group_of(const uint32_t* __restrict__ off, uint32_t n_groups, uint32_t row) {  // off[g] <= row < off[g + 1]
  uint32_t lo = 0, hi = n_groups;
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (off[mid] <= row) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kThreads) void trf_rank_keys_kernel(const uint32_t* __restrict__ off, uint32_t n_groups,
                                                                 const float* __restrict__ rho, uint32_t n_rows, uint64_t* __restrict__ keys,
                                                                 uint32_t* __restrict__ vals) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n_rows) return;
  keys[i] = ((uint64_t)group_of(off, n_groups, i) << 32) | (uint64_t)(~__float_as_uint(rho[i]));
  vals[i] = i;
}

__global__ __launch_bounds__(kThreads) void trf_rank_local_kernel(const uint32_t* __restrict__ off, const uint64_t* __restrict__ keys,
                                                                  const uint32_t* __restrict__ vals, uint32_t n_rows, uint32_t* __restrict__ rank) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i < n_rows) rank[i] = vals[i] - off[(uint32_t)(keys[i] >> 32)];
}

}  // namespace

hipError_t trf_items_launch(const TrfGroupParams& p, uint32_t* flags, uint64_t* sums, uint32_t* printed, int32_t* rep, uint32_t* stat,
                            hipStream_t stream) {
  const uint64_t total = (uint64_t)p.S * p.k;
  if (!total) return hipSuccess;
  hipLaunchKernelGGL(trf_items_kernel, dim3(grid_for(total)), dim3(kThreads), 0, stream, p, flags, sums, printed, rep, stat);
  return hipGetLastError();
}

hipError_t trf_item_scatter_launch(const uint32_t* scan, uint64_t total, uint32_t* item, hipStream_t stream) {
  if (!total) return hipSuccess;
  hipLaunchKernelGGL(trf_item_scatter_kernel, dim3(grid_for(total)), dim3(kThreads), 0, stream, scan, total, item);
  return hipGetLastError();
}

hipError_t trf_iota_launch(uint32_t* vals, uint32_t n, hipStream_t stream) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(trf_iota_kernel, dim3(grid_for(n)), dim3(kThreads), 0, stream, vals, n);
  return hipGetLastError();
}

hipError_t trf_chunk_keys_launch(const TrfGroupParams& p, const uint32_t* vals, uint32_t chunk, uint64_t* keys, hipStream_t stream) {
  if (!p.k) return hipSuccess;
  hipLaunchKernelGGL(trf_chunk_keys_kernel, dim3(grid_for(p.k)), dim3(kThreads), 0, stream, p, vals, chunk, keys);
  return hipGetLastError();
}

hipError_t trf_rank_scatter_launch(const uint32_t* vals, uint32_t n, uint32_t* rank, hipStream_t stream) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(trf_rank_scatter_kernel, dim3(grid_for(n)), dim3(kThreads), 0, stream, vals, n, rank);
  return hipGetLastError();
}

hipError_t trf_order_keys_a_launch(const TrfGroupParams& p, const uint32_t* item, uint32_t n_rows, const uint32_t* rank, uint32_t rank_bits,
                                   uint64_t* keys, uint32_t* vals, hipStream_t stream) {
  if (!n_rows) return hipSuccess;
  hipLaunchKernelGGL(trf_order_keys_a_kernel, dim3(grid_for(n_rows)), dim3(kThreads), 0, stream, p, item, n_rows, rank, rank_bits, keys,
                     vals);
  return hipGetLastError();
}

hipError_t trf_order_keys_b_launch(const TrfGroupParams& p, const uint32_t* item, const uint32_t* vals, uint32_t n_rows,
                                   const uint32_t* cell_block, uint64_t* keys, hipStream_t stream) {
  if (!n_rows) return hipSuccess;
  hipLaunchKernelGGL(trf_order_keys_b_kernel, dim3(grid_for(n_rows)), dim3(kThreads), 0, stream, p, item, vals, n_rows, cell_block, keys);
  return hipGetLastError();
}

hipError_t trf_pack_launch(const TrfGroupParams& p, const uint32_t* item, const uint32_t* vals, uint32_t n_rows, const uint64_t* denom,
                           const TrfPackOut& out, hipStream_t stream) {
  if (!n_rows) return hipSuccess;
  const dim3 grid(grid_for(n_rows)), block(kThreads);
  switch (p.W) {
    case 1: hipLaunchKernelGGL(trf_pack_kernel<1>, grid, block, 0, stream, p, item, vals, n_rows, denom, out); break;
    case 2: hipLaunchKernelGGL(trf_pack_kernel<2>, grid, block, 0, stream, p, item, vals, n_rows, denom, out); break;
    case 4: hipLaunchKernelGGL(trf_pack_kernel<4>, grid, block, 0, stream, p, item, vals, n_rows, denom, out); break;
    case 8: hipLaunchKernelGGL(trf_pack_kernel<8>, grid, block, 0, stream, p, item, vals, n_rows, denom, out); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t trf_rank_keys_launch(const uint32_t* off, uint32_t n_groups, const float* rho, uint32_t n_rows, uint64_t* keys, uint32_t* vals,
                                hipStream_t stream) {
  if (!n_rows) return hipSuccess;
  hipLaunchKernelGGL(trf_rank_keys_kernel, dim3(grid_for(n_rows)), dim3(kThreads), 0, stream, off, n_groups, rho, n_rows, keys, vals);
  return hipGetLastError();
}

hipError_t trf_rank_local_launch(const uint32_t* off, const uint64_t* keys, const uint32_t* vals, uint32_t n_rows, uint32_t* rank,
                                 hipStream_t stream) {
  if (!n_rows) return hipSuccess;
  hipLaunchKernelGGL(trf_rank_local_kernel, dim3(grid_for(n_rows)), dim3(kThreads), 0, stream, off, keys, vals, n_rows, rank);
  return hipGetLastError();
}

}  // namespace mrg
