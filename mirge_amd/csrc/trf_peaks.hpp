// Launchers of csrc/trf_peaks.hip (the density-peak clustering of `-trf`); the C-ABI entry points
// mrg_trf_rho / mrg_trf_delta / mrg_trf_border (capi.hip) build the block lists and call these.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

namespace mrg {

constexpr uint32_t kTrfTile = 256;     // rows per workgroup (one lane each) and j-rows per LDS tile
constexpr uint32_t kTrfKtabMax = 256;  // entries of the gaussian table K[d] the rho pass keeps in LDS

struct TrfLaunch {
  const uint32_t* off;     // device, n_groups + 1 row offsets
  const uint2* blocks;     // device, (group, first row or rank position of the tile), most work first
  uint32_t n_blocks;
  uint64_t n_all;          // rows of all groups (the SoA stride)
  uint32_t W;              // words per row: ceil(longest template / 32), 1..8
  const uint64_t* codes;   // [W][n_all]
  const uint64_t* nmask;   // [W][n_all] or nullptr
  const uint16_t* span;    // first | last << 8
  const double* rpm;       // rho pass only
};

hipError_t trf_rho_launch(const TrfLaunch& L, const double* ktab, uint32_t n_ktab, float* rho, uint32_t* max_dis,
                          hipStream_t stream);
hipError_t trf_delta_launch(const TrfLaunch& L, const uint32_t* rank, const uint32_t* max_dis, int32_t* delta,
                            int32_t* nneigh, hipStream_t stream);
hipError_t trf_border_launch(const TrfLaunch& L, const float* rho, const int32_t* label, const uint32_t* bord_off,
                             float* bord, hipStream_t stream);

}  // namespace mrg
