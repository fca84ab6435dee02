// Suffix array, BWT blocks and suffix-array rows of an FM index on the device (gfx950): the device route of
// build_index (fm_index.hpp, RowBuilder).  Internal header (capi.hip).
#pragma once
#include <cstdint>
#include <stdexcept>
#include <string>

#include "fm_index.hpp"

namespace mrg {

// What went wrong on the device route: a HIP call failed, or the working set does not fit the free device memory.
struct SaBuildError : std::runtime_error {
  bool no_memory;
  SaBuildError(const std::string& what, bool nomem) : std::runtime_error(what), no_memory(nomem) {}
};

// Device bytes build_rows_device allocates for a text of n bases (about 33 per base).
uint64_t sa_build_device_bytes(uint32_t n, uint32_t n_seg);

// Bases of the first-round key: the order of the first 30 bases of every suffix comes from one sort of the packed text.
constexpr uint32_t kSaFirstBases = 30;

// Fills ix.blocks, ix.super, ix.primary and ix.sa, every word what build_index's host code computes, on the CURRENT
// device from ix.n, ix.C, ix.text, ix.seg_start and ix.chunk_seg.  *rounds (may be null): sort rounds used, the
// first-round sort included; never more than ceil(log2((n + 1) / kSaFirstBases)) + 1.  Throws SaBuildError; nothing of
// ix is touched before the device work is complete.
void build_rows_device(FmIndex& ix, uint32_t* rounds);

}  // namespace mrg
