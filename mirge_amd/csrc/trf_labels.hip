// `-trf` on the device (mrg_trf_assign / mrg_trf_halo, include/mirge_amd.h): from rho, the rank, delta and nneigh of the
// density peaks to the cluster centres, every row's label and its core / halo flag -- peaks_results' label pass and the halo
// half of cluster_text (mirge_amd/trf_samples.py) on the arrays.  gfx950, wave64; one lane per row (or group), no LDS.
// Everything is integer work or an exact float32 comparison, and every sum goes through an integer atomic: nothing depends
// on the order of the lanes.  The labels are the roots of the nneigh forest, found by pointer doubling in a number of rounds
// the host fixes: no loop here ends on a value read from device memory, and every index is range-checked before it is followed.
#include "trf_labels.hpp"

namespace mrg {

namespace {

constexpr uint32_t kThreads = 256;
constexpr uint64_t M55 = 0x5555555555555555ull;

inline uint32_t grid_for(uint64_t n) { return (uint32_t)((n + kThreads - 1) / kThreads); }

// The group of a row: the last g with off[g] <= row (32 halvings cover 2^32 groups).
__device__ inline uint32_t group_of(const uint32_t* __restrict__ off, uint32_t n_groups, uint32_t row) {
  uint32_t lo = 0, hi = n_groups;
  for (int s = 0; s < 32; ++s) {
    if (hi - lo > 1) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (off[mid] <= row) lo = mid; else hi = mid;
    }
  }
  return lo;
}

// The top row of a group (group-local), or kTrfNoRow when the rank entry is no row of the group.
__device__ inline uint32_t top_of(const TrfAssignIn& in, uint32_t g) {
  const uint32_t a = in.off[g], size = in.off[g + 1] - a;
  const uint32_t top = in.rank[a];
  return top < size ? top : kTrfNoRow;
}

__global__ __launch_bounds__(kThreads) void trf_assign_stats_kernel(const TrfAssignIn in, uint32_t* __restrict__ grp,
                                                                    uint32_t* __restrict__ gdelta, uint32_t* __restrict__ grho,
                                                                    uint32_t* __restrict__ err) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= in.n_rows) return;
  const uint32_t g = group_of(in.off, in.n_groups, i);
  grp[i] = g;
  const uint32_t top = top_of(in, g);
  if (top == kTrfNoRow) {
    atomicOr(err, kTrfErrTop);
    return;
  }
  if (i - in.off[g] != top) atomicMax(&gdelta[g], (uint32_t)max(in.delta[i], 0));
  atomicMax(&grho[g], __float_as_uint(fmaxf(in.rho[i], 0.f)));  // (rho >= 0: the bit pattern is monotone)
}

__device__ inline bool is_center(const TrfAssignIn& in, uint32_t g, uint32_t i, const uint32_t* __restrict__ gdelta) {
  const uint32_t top = top_of(in, g);
  const int32_t d = (i - in.off[g] == top) ? (int32_t)min(gdelta[g], 0x7FFFFFFFu) : in.delta[i];
  return in.rho[i] >= kTrfRhoMin && d >= kTrfDeltaMin;
}

__global__ __launch_bounds__(kThreads) void trf_assign_flags_kernel(const TrfAssignIn in, const uint32_t* __restrict__ grp,
                                                                    const uint32_t* __restrict__ gdelta, uint32_t* __restrict__ flags) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i > in.n_rows) return;
  flags[i] = (i < in.n_rows && is_center(in, grp[i], i, gdelta)) ? 1u : 0u;
}

__global__ __launch_bounds__(kThreads) void trf_assign_fallback_kernel(const TrfAssignIn in, const uint32_t* __restrict__ grp,
                                                                       const uint32_t* __restrict__ scan,
                                                                       const uint32_t* __restrict__ gdelta,
                                                                       const uint32_t* __restrict__ grho, uint32_t* __restrict__ fb) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= in.n_rows) return;
  const uint32_t g = grp[i];
  if (scan[in.off[g + 1]] != scan[in.off[g]]) return;  // the group has a centre
  if (gdelta[g] > (uint32_t)kTrfDeltaMin || __uint_as_float(grho[g]) < kTrfRhoMin) return;  // W2C:895
  if (__float_as_uint(fmaxf(in.rho[i], 0.f)) == grho[g]) atomicMin(&fb[g], i - in.off[g]);
}

__global__ __launch_bounds__(kThreads) void trf_assign_nclust_kernel(const TrfAssignIn in, const uint32_t* __restrict__ scan,
                                                                     const uint32_t* __restrict__ fb, uint32_t* __restrict__ ncl) {
  const uint32_t g = blockIdx.x * kThreads + threadIdx.x;
  if (g > in.n_groups) return;
  uint32_t n = 0;
  if (g < in.n_groups) {
    n = scan[in.off[g + 1]] - scan[in.off[g]];
    if (n == 0 && fb[g] != kTrfNoRow) n = 1;
  }
  ncl[g] = n;
}

__global__ __launch_bounds__(kThreads) void trf_assign_init_kernel(const TrfAssignIn in, const uint32_t* __restrict__ grp,
                                                                   const uint32_t* __restrict__ scan, const uint32_t* __restrict__ fb,
                                                                   const uint32_t* __restrict__ cen_off, int32_t* __restrict__ lab,
                                                                   uint32_t* __restrict__ nxt, uint32_t* __restrict__ centers,
                                                                   uint32_t* __restrict__ err) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= in.n_rows) return;
  const uint32_t g = grp[i], a = in.off[g], size = in.off[g + 1] - a, local = i - a;
  const uint32_t n_flag = scan[a + size] - scan[a];
  int32_t label = 0;
  uint32_t next = i;
  if (n_flag ? scan[i + 1] != scan[i] : fb[g] == local) {
    label = n_flag ? (int32_t)(scan[i] - scan[a]) + 1 : 1;   // numbered in row order
    const uint32_t slot = cen_off[g] + (uint32_t)label - 1;
    if (slot < cen_off[g + 1]) centers[slot] = local;
  } else if (local == top_of(in, g)) {
    label = -1;                                              // a top row that is no centre: its tree has no cluster
  } else {
    const int32_t nn = in.nneigh[i];
    if (nn < 0 || (uint32_t)nn >= size || (uint32_t)nn == local) {
      atomicOr(err, kTrfErrNeighbour);
      label = -1;                                            // (closed, so that no round follows it)
    } else {
      next = a + (uint32_t)nn;
    }
  }
  lab[i] = label;
  nxt[i] = next;
}

// Between a row and its nxt lie only rows that were open at the start (no centre, no top), so the first closed row on the
// way carries the label of the first centre of the row's own chain.  After round r every row within 2^r steps of a centre or
// a top is closed; the open ones point 2^r steps up.
__global__ __launch_bounds__(kThreads) void trf_assign_round_kernel(const TrfAssignIn in, const uint32_t* __restrict__ grp,
                                                                    const int32_t* __restrict__ lab_in, const uint32_t* __restrict__ nxt_in,
                                                                    int32_t* __restrict__ lab_out, uint32_t* __restrict__ nxt_out) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= in.n_rows) return;
  int32_t label = lab_in[i];
  uint32_t next = nxt_in[i];
  if (label == 0) {
    const uint32_t g = grp[i], a = in.off[g], b = in.off[g + 1];
    if (next >= a && next < b) {          // (always, by construction: checked all the same before it is followed)
      const int32_t up = lab_in[next];
      if (up != 0) {
        label = up;
      } else {
        const uint32_t far = nxt_in[next];
        if (far >= a && far < b) next = far;
      }
    }
  }
  lab_out[i] = label;
  nxt_out[i] = next;
}

__global__ __launch_bounds__(kThreads) void trf_assign_finish_kernel(uint32_t n_rows, const int32_t* __restrict__ lab,
                                                                     int32_t* __restrict__ label, uint32_t* __restrict__ err) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= n_rows) return;
  const int32_t v = lab[i];
  label[i] = v;
  if (v == 0) atomicOr(err, kTrfErrUnresolved);
}

// getDistance (W2C:434-440) of two rows, as pair_dist of trf_peaks.hip, from global memory.
__device__ inline int32_t row_dist(const TrfHaloIn& in, uint32_t x, uint32_t y) {
  const uint32_t sx = in.span[x], sy = in.span[y];
  const int32_t fx = (int32_t)(sx & 0xffu), lx = (int32_t)(sx >> 8), fy = (int32_t)(sy & 0xffu), ly = (int32_t)(sy >> 8);
  int32_t d = abs(fx - fy) + abs(lx - ly);
  const int32_t lo = max(fx, fy) - 1, hi = min(lx, ly) - 1;  // 0-based, inclusive
  for (uint32_t w = 0; w < in.W; ++w) {
    const int32_t b = 32 * (int32_t)w;
    if (hi >= b && lo <= b + 31 && lo <= hi) {
      const int32_t s0 = max(lo - b, 0), e0 = min(hi - b, 31);
      const uint64_t m = (e0 == 31 ? ~0ull : ((1ull << (2 * e0 + 2)) - 1ull)) & (~0ull << (2 * s0));
      const uint64_t c = in.codes[w * in.stride + x] ^ in.codes[w * in.stride + y];
      uint64_t v = c | (c >> 1);
      if (in.nmask) v |= in.nmask[w * in.stride + x] ^ in.nmask[w * in.stride + y];
      d += __popcll(v & m & M55);
    }
  }
  return d;
}

__global__ __launch_bounds__(kThreads) void trf_halo_kernel(const TrfHaloIn in, uint32_t slot_bits, uint8_t* __restrict__ core,
                                                            unsigned long long* __restrict__ tally, uint64_t* __restrict__ keys,
                                                            uint32_t* __restrict__ vals, uint32_t* __restrict__ err) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= in.n_rows) return;
  const uint32_t g = group_of(in.off, in.n_groups, i), a = in.off[g], size = in.off[g + 1] - a;
  const uint32_t c0 = in.cen_off[g], nc = in.cen_off[g + 1] - c0;
  const int32_t label = in.label[i];
  uint32_t slot = nc;
  bool is_core = false;
  if (label >= 1 && (uint32_t)label <= nc) {
    slot = (uint32_t)label - 1;
    const uint32_t center = in.centers[c0 + slot];
    if (center >= size) {
      atomicOr(err, 1u);
    } else {
      is_core = row_dist(in, i, a + center) <= kTrfDeltaMin;
      if (nc > 1) {
        const uint32_t b0 = in.bord_off[g];
        if (in.bord_off[g + 1] - b0 != nc + 1)
          atomicOr(err, 1u);
        else if (in.rho[i] < in.bord[b0 + (uint32_t)label])
          is_core = false;
      }
      const unsigned long long count = in.counts[(uint64_t)i * in.count_stride];
      unsigned long long* t = tally + 4ull * (c0 + slot);
      atomicAdd(&t[0], 1ull);
      if (is_core) atomicAdd(&t[1], 1ull);
      atomicAdd(&t[is_core ? 2 : 3], count);
    }
  } else if (label != -1) {
    atomicOr(err, 1u);
  }
  core[i] = is_core ? 1 : 0;
  keys[i] = ((uint64_t)g << slot_bits) | (uint64_t)slot;
  vals[i] = i;
}

}  // namespace

#define TRF_LABELS_LAUNCH(kernel, count, ...)                                                            \
  do {                                                                                                   \
    if (!(count)) return hipSuccess;                                                                     \
    hipLaunchKernelGGL(kernel, dim3(grid_for(count)), dim3(kThreads), 0, stream, __VA_ARGS__);           \
    return hipGetLastError();                                                                            \
  } while (0)

hipError_t trf_assign_stats_launch(const TrfAssignIn& in, uint32_t* grp, uint32_t* gdelta, uint32_t* grho, uint32_t* err, hipStream_t stream) {
  TRF_LABELS_LAUNCH(trf_assign_stats_kernel, in.n_rows, in, grp, gdelta, grho, err);
}

hipError_t trf_assign_flags_launch(const TrfAssignIn& in, const uint32_t* grp, const uint32_t* gdelta, uint32_t* flags, hipStream_t stream) {
  TRF_LABELS_LAUNCH(trf_assign_flags_kernel, (uint64_t)in.n_rows + 1, in, grp, gdelta, flags);
}

hipError_t trf_assign_fallback_launch(const TrfAssignIn& in, const uint32_t* grp, const uint32_t* scan, const uint32_t* gdelta,
                                      const uint32_t* grho, uint32_t* fb, hipStream_t stream) {
  TRF_LABELS_LAUNCH(trf_assign_fallback_kernel, in.n_rows, in, grp, scan, gdelta, grho, fb);
}

hipError_t trf_assign_nclust_launch(const TrfAssignIn& in, const uint32_t* scan, const uint32_t* fb, uint32_t* ncl, hipStream_t stream) {
  TRF_LABELS_LAUNCH(trf_assign_nclust_kernel, (uint64_t)in.n_groups + 1, in, scan, fb, ncl);
}

hipError_t trf_assign_init_launch(const TrfAssignIn& in, const uint32_t* grp, const uint32_t* scan, const uint32_t* fb,
                                  const uint32_t* cen_off, int32_t* lab, uint32_t* nxt, uint32_t* centers, uint32_t* err,
                                  hipStream_t stream) {
  TRF_LABELS_LAUNCH(trf_assign_init_kernel, in.n_rows, in, grp, scan, fb, cen_off, lab, nxt, centers, err);
}

hipError_t trf_assign_round_launch(const TrfAssignIn& in, const uint32_t* grp, const int32_t* lab_in, const uint32_t* nxt_in,
                                   int32_t* lab_out, uint32_t* nxt_out, hipStream_t stream) {
  TRF_LABELS_LAUNCH(trf_assign_round_kernel, in.n_rows, in, grp, lab_in, nxt_in, lab_out, nxt_out);
}

hipError_t trf_assign_finish_launch(uint32_t n_rows, const int32_t* lab, int32_t* label, uint32_t* err, hipStream_t stream) {
  TRF_LABELS_LAUNCH(trf_assign_finish_kernel, n_rows, n_rows, lab, label, err);
}

hipError_t trf_halo_launch(const TrfHaloIn& in, uint32_t slot_bits, uint8_t* core, unsigned long long* tally, uint64_t* keys,
                           uint32_t* vals, uint32_t* err, hipStream_t stream) {
  TRF_LABELS_LAUNCH(trf_halo_kernel, in.n_rows, in, slot_bits, core, tally, keys, vals, err);
}

}  // namespace mrg
