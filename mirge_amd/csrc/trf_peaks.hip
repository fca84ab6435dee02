// Density peaks (Rodriguez-Laio) of the per-sample tRF reports, `-trf` (W2C = utils/writeDataToCSV.py): the
// O(n^2) parts of local_density (W2C:470-499), min_distance (W2C:509-533) and the border-density loop
// (W2C:951-961) for every (sample, tRNA) group of a run, one launch each.  Row layout: include/mirge_amd.h.
// No distance is stored: getDistance (W2C:417-449) is recomputed from the two rows whenever a pass needs it,
//   |first_i - first_j| + |last_i - last_j| + popcount(((x | x >> 1) | (n_i ^ n_j)) & 0x55.. & overlap)
// per word, x = codes_i ^ codes_j (an N carries code 0: N = N, N != base).
// One lane per row, kTrfTile rows of one group per workgroup; the group's j-rows go through LDS a tile at a time
// and every lane reads the same j (an LDS broadcast).  The host orders the blocks with the most work first.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "trf_peaks.hpp"

// rho is a left-to-right double sum of rounded products (Python's `rho[i] += f * R`): no FMA.
#pragma clang fp contract(off)

namespace mrg {

namespace {

constexpr uint32_t TILE = kTrfTile;
constexpr uint32_t W_MAX = 8;  // 255-nt templates
constexpr uint64_t M55 = 0x5555555555555555ull;

struct Row {
  uint64_t c[W_MAX], n[W_MAX];
  int32_t first, last;
};

template <bool HAS_N>
__device__ __forceinline__ void load_row(Row& r, const TrfLaunch& L, uint64_t row) {
#pragma unroll
  for (uint32_t w = 0; w < W_MAX; ++w) {
    r.c[w] = w < L.W ? L.codes[w * L.n_all + row] : 0ull;
    r.n[w] = (HAS_N && w < L.W) ? L.nmask[w * L.n_all + row] : 0ull;
  }
  r.first = (int32_t)(L.span[row] & 0xffu);
  r.last = (int32_t)(L.span[row] >> 8);
}

// The j-rows of one tile, SoA in LDS so that a staging store of the block is contiguous.
template <bool HAS_N>
struct Stage {
  uint64_t c[W_MAX * TILE];
  uint64_t n[HAS_N ? W_MAX * TILE : 1];
  uint16_t span[TILE];

  __device__ __forceinline__ void put(uint32_t t, const TrfLaunch& L, uint64_t row) {
#pragma unroll
    for (uint32_t w = 0; w < W_MAX; ++w) {
      if (w < L.W) {
        c[w * TILE + t] = L.codes[w * L.n_all + row];
        if (HAS_N) n[w * TILE + t] = L.nmask[w * L.n_all + row];
      }
    }
    span[t] = L.span[row];
  }
};

// getDistance of row `a` and staged row t: returns the shift part in *sh and, if it is <= bound, the whole distance
// (else the shift part: the substitutions cannot bring it down).
template <bool HAS_N>
__device__ __forceinline__ int32_t pair_dist(const Row& a, const Stage<HAS_N>& s, uint32_t t, uint32_t W, int32_t bound) {
  const int32_t fj = (int32_t)(s.span[t] & 0xffu), lj = (int32_t)(s.span[t] >> 8);
  int32_t d = abs(a.first - fj) + abs(a.last - lj);
  if (d > bound) return d;
  const int32_t lo = max(a.first, fj) - 1, hi = min(a.last, lj) - 1;  // 0-based, inclusive
#pragma unroll
  for (uint32_t w = 0; w < W_MAX; ++w) {
    const int32_t b = 32 * (int32_t)w;
    if (w < W && hi >= b && lo <= b + 31 && lo <= hi) {
      const int32_t s0 = max(lo - b, 0), e0 = min(hi - b, 31);
      const uint64_t m = (e0 == 31 ? ~0ull : ((1ull << (2 * e0 + 2)) - 1ull)) & (~0ull << (2 * s0));
      const uint64_t x = a.c[w] ^ s.c[w * TILE + t];
      uint64_t y = x | (x >> 1);
      if (HAS_N) y |= a.n[w] ^ s.n[w * TILE + t];
      d += __popcll(y & m & M55);
    }
  }
  return d;
}

// ---------------------------------------------------------------- local_density (W2C:470-499)
template <bool HAS_N>
__global__ __launch_bounds__(TILE) void trf_rho_kernel(const TrfLaunch L, const double* __restrict__ ktab,
                                                       uint32_t n_ktab, float* __restrict__ rho,
                                                       uint32_t* __restrict__ max_dis) {
  __shared__ Stage<HAS_N> s;
  __shared__ double s_rpm[TILE], s_k[kTrfKtabMax];
  __shared__ uint32_t s_max;
  const uint2 b = L.blocks[blockIdx.x];
  const uint64_t base = L.off[b.x];
  const uint32_t n = L.off[b.x + 1] - (uint32_t)base, tid = threadIdx.x, i = b.y + tid;
  const bool act = i < n;
  for (uint32_t t = tid; t < n_ktab; t += TILE) s_k[t] = ktab[t];
  if (tid == 0) s_max = 0;
  Row a;
  if (act) load_row<HAS_N>(a, L, base + i);
  double acc = 0.0;
  int32_t mx = 0;
  for (uint32_t jt = 0; jt < n; jt += TILE) {
    const uint32_t cnt = min(TILE, n - jt);
    __syncthreads();
    if (tid < cnt) {
      s.put(tid, L, base + jt + tid);
      s_rpm[tid] = L.rpm[base + jt + tid];
    }
    __syncthreads();
    for (uint32_t t = 0; act && t < cnt; ++t) {
      if (jt + t == i) continue;
      const int32_t d = pair_dist<HAS_N>(a, s, t, L.W, INT32_MAX);
      mx = max(mx, d);
      // rho_i += K[d] * RPM_j in the reference's j order; K[d] == 0 past the table adds +0.0 (skipped)
      if ((uint32_t)d < n_ktab) {
        const double term = s_k[d] * s_rpm[t];
        acc = acc + term;
      }
    }
  }
  if (act) {
    rho[base + i] = (float)(acc + L.rpm[base + i]);
    atomicMax(&s_max, (uint32_t)mx);
  }
  __syncthreads();
  if (tid == 0 && s_max) atomicMax(&max_dis[b.x], s_max);
}

// ---------------------------------------------------------------- min_distance (W2C:509-533)
// Lane p takes the row at rank position p; its candidates are the rows at positions q < p, scanned in rank order
// with `<=`, so of equally near rows the one ranked last wins.
template <bool HAS_N>
__global__ __launch_bounds__(TILE) void trf_delta_kernel(const TrfLaunch L, const uint32_t* __restrict__ rank,
                                                         const uint32_t* __restrict__ max_dis, int32_t* __restrict__ delta,
                                                         int32_t* __restrict__ nneigh) {
  __shared__ Stage<HAS_N> s;
  __shared__ uint32_t s_row[TILE];
  const uint2 b = L.blocks[blockIdx.x];
  const uint64_t base = L.off[b.x];
  const uint32_t n = L.off[b.x + 1] - (uint32_t)base, tid = threadIdx.x, p = b.y + tid;
  const uint32_t i = p < n ? rank[base + p] : 0u;
  const bool act = p < n && i < n;  // (a rank entry out of its group is ignored, not followed)
  Row a;
  if (act) load_row<HAS_N>(a, L, base + i);
  int32_t best = (int32_t)max_dis[b.x], nn = -1;
  const uint32_t q_end = min(n, b.y + TILE);
  for (uint32_t qt = 0; qt < q_end; qt += TILE) {
    const uint32_t cnt = min(TILE, q_end - qt);
    __syncthreads();
    if (tid < cnt) {
      const uint32_t r = rank[base + qt + tid];
      s_row[tid] = r < n ? r : 0u;
      s.put(tid, L, base + s_row[tid]);
    }
    __syncthreads();
    const uint32_t lim = act && p > qt ? min(cnt, p - qt) : 0u;
    for (uint32_t t = 0; t < lim; ++t) {
      const int32_t d = pair_dist<HAS_N>(a, s, t, L.W, best);
      if (d <= best) {
        best = d;
        nn = (int32_t)s_row[t];
      }
    }
  }
  if (act) {
    delta[base + i] = p == 0 ? -1 : best;
    nneigh[base + i] = p == 0 ? -1 : nn;
  }
}

// ---------------------------------------------------------------- border density (W2C:951-961)
// Each lane takes the pairs of its row (both orders of a pair give the same value), then one atomic max on the float
// bits (the values are >= 0) into the slot of its label; label -1 is Python's bord_rho[-1] = bord_rho[NCLUST].
template <bool HAS_N>
__global__ __launch_bounds__(TILE) void trf_border_kernel(const TrfLaunch L, const float* __restrict__ rho,
                                                          const int32_t* __restrict__ label,
                                                          const uint32_t* __restrict__ bord_off, float* __restrict__ bord) {
  __shared__ Stage<HAS_N> s;
  __shared__ float s_rho[TILE];
  __shared__ int32_t s_cl[TILE];
  const uint2 b = L.blocks[blockIdx.x];
  const uint64_t base = L.off[b.x];
  const uint32_t n = L.off[b.x + 1] - (uint32_t)base, tid = threadIdx.x, i = b.y + tid;
  const uint32_t n_slots = bord_off[b.x + 1] - bord_off[b.x];  // NCLUST + 1
  const bool act = i < n;
  Row a;
  const float rho_i = act ? rho[base + i] : 0.f;
  const int32_t cl_i = act ? label[base + i] : 0;
  if (act) load_row<HAS_N>(a, L, base + i);
  float m = -1.f;
  for (uint32_t jt = 0; jt < n; jt += TILE) {
    const uint32_t cnt = min(TILE, n - jt);
    __syncthreads();
    if (tid < cnt) {
      s.put(tid, L, base + jt + tid);
      s_rho[tid] = rho[base + jt + tid];
      s_cl[tid] = label[base + jt + tid];
    }
    __syncthreads();
    for (uint32_t t = 0; act && t < cnt; ++t) {
      if (s_cl[t] != cl_i && pair_dist<HAS_N>(a, s, t, L.W, 3) <= 3) {  // (s_cl[t] != cl_i also skips j == i)
        const float v = (rho_i + s_rho[t]) / 2.0f;
        m = v > m ? v : m;
      }
    }
  }
  const int32_t slot = cl_i < 0 ? cl_i + (int32_t)n_slots : cl_i;
  if (act && m >= 0.f && slot >= 0 && (uint32_t)slot < n_slots)
    atomicMax(reinterpret_cast<unsigned int*>(bord + bord_off[b.x] + slot), __float_as_uint(m));
}

template <typename K1, typename K0, typename... A>
hipError_t launch(const TrfLaunch& L, K1 with_n, K0 without_n, hipStream_t stream, A... args) {
  if (!L.n_blocks) return hipSuccess;
  if (L.nmask)
    hipLaunchKernelGGL(with_n, dim3(L.n_blocks), dim3(TILE), 0, stream, L, args...);
  else
    hipLaunchKernelGGL(without_n, dim3(L.n_blocks), dim3(TILE), 0, stream, L, args...);
  return hipGetLastError();
}

}  // namespace

hipError_t trf_rho_launch(const TrfLaunch& L, const double* ktab, uint32_t n_ktab, float* rho, uint32_t* max_dis,
                          hipStream_t stream) {
  return launch(L, trf_rho_kernel<true>, trf_rho_kernel<false>, stream, ktab, n_ktab, rho, max_dis);
}

hipError_t trf_delta_launch(const TrfLaunch& L, const uint32_t* rank, const uint32_t* max_dis, int32_t* delta,
                            int32_t* nneigh, hipStream_t stream) {
  return launch(L, trf_delta_kernel<true>, trf_delta_kernel<false>, stream, rank, max_dis, delta, nneigh);
}

hipError_t trf_border_launch(const TrfLaunch& L, const float* rho, const int32_t* label, const uint32_t* bord_off,
                             float* bord, hipStream_t stream) {
  return launch(L, trf_border_kernel<true>, trf_border_kernel<false>, stream, rho, label, bord_off, bord);
}

}  // namespace mrg
