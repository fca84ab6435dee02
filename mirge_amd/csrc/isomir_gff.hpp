// `-gff`: the isomiR classification of the reads claimed by the exact-miRNA and the isomiR pass (csrc/isomir_gff.hip,
// mrg_isomir_classify) and the writer of the per-sample GFF files (isomir_gff_write.cpp, mrg_write_isomir_gff).
// Internal header: the record layout both sides and mirge_amd/isomir.py share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mrg {

// Per miRNA library entry (host table of mirge_amd.isomir.entry_table), int32 [M][5].
constexpr uint32_t kIsoDescInts = 5;
constexpr int kIsoDescOff = 0;     // first word of the entry's precursor in the text tables
constexpr int kIsoDescLen = 1;     // bases of the precursor
constexpr int kIsoDescM0 = 2;      // first occurrence of the mature sequence in it
constexpr int kIsoDescMat = 3;     // bases of the mature sequence
constexpr int kIsoDescStatus = 4;  // 0 = ok, 1 = mature not in the precursor (the read is dropped), 2 = unresolvable

// Per output row, int32 [k][8].
constexpr uint32_t kIsoRecInts = 8;
constexpr int kIsoRecStart = 0;  // pre_start = r0 + 1
constexpr int kIsoRecEnd = 1;    // pre_end = r1
constexpr int kIsoRec5p = 2;     // iso_5p value m0 - r0 (0 = no such variant)
constexpr int kIsoRec3p = 3;     // iso_3p or iso_add value r1 - m1 (0 = neither)
constexpr int kIsoRecFlags = 4;  // kind | snp << 8 | add << 16
constexpr int kIsoRecEnds = 5;   // leading | trailing << 16 read bases outside the precursor (the CIGAR's I columns)
constexpr int kIsoRecEntry = 6;  // the library entry (ref_id of the read)
// kind
constexpr uint32_t kIsoDropped = 0, kIsoRef = 1, kIsoIsomir = 2, kIsoUnresolvable = 3, kIsoBadEntry = 4;
// snp: 0 = none, 1 = iso_snp, 2 = _seed, 3 = _central_offset, 4 = _central, 5 = central_supp

struct IsoClassifyParams {
  const uint64_t* reads;  // [W][stride]
  const uint64_t* nmask;  // or nullptr
  const uint8_t* lens;
  const int32_t* ref_id;
  const int32_t* pos;
  uint64_t stride;
  uint32_t W;
  const uint32_t* idx;    // row -> read
  uint32_t rows;          // rows to classify (min(selected, capacity))
  uint32_t n_canon;       // rows below this one come from the exact-miRNA pass
  const int32_t* desc;    // device copy of the entry table
  uint32_t n_entries;
  const uint64_t* text;   // precursor bases, 2 bits each, every precursor from a word boundary
  const uint64_t* nplane; // bit 2i set: base i is no ACGT (code 0 = N, code 1 = a character no read holds)
  uint32_t text_words;
  int32_t* rec;           // [rows][kIsoRecInts]
  uint32_t* mask;         // [rows][2 * mask_words] (the uint64 [rows][mask_words] of the C-ABI, low half first)
  uint32_t mask_words;    // ceil(32 W / 64)
};

// flags[i] = pass_id[i] == canon_pass, flags[n + i] = pass_id[i] == isomir_pass, flags[2n] = 0
hipError_t iso_flags_launch(const int8_t* pass_id, uint64_t n, int32_t canon_pass, int32_t isomir_pass, uint32_t* flags,
                            hipStream_t stream);
// idx[off[j]] = j mod n for every set flag j whose slot is below cap (off = exclusive sums of the flags)
hipError_t iso_scatter_launch(const int8_t* pass_id, uint64_t n, int32_t canon_pass, int32_t isomir_pass, const uint32_t* off,
                              uint64_t cap, uint32_t* idx, hipStream_t stream);
hipError_t iso_classify_launch(const IsoClassifyParams& p, hipStream_t stream);

// Throws std::runtime_error (I/O) or std::invalid_argument (a record that does not fit its read).
void write_isomir_gff(const char* const* paths, const char* const* coldata, uint32_t S, const char* source, const uint64_t* reads,
                      uint32_t W, uint64_t stride, const uint8_t* lens, const uint64_t* nmask, uint64_t n, const uint32_t* quant,
                      const uint32_t* idx, const int32_t* rec, const uint64_t* mask, uint64_t k, const char* const* entry_names,
                      const char* const* pre_names, uint64_t n_entries, uint64_t* rows);

}  // namespace mrg
