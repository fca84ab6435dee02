// `-ai`: the alignment of every miRNA read to the canonical sequence of its (merged) miRNA (csrc/a2i_align.hip,
// mrg_a2i_align) and the writer of a2IEditing.detail.txt (a2i_detail_write.cpp, mrg_write_a2i_detail).
// Internal header: the record layout both sides and mirge_amd/a2i.py share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mrg {

// Per selected read, int32 [k][4] (16 bytes).
constexpr uint32_t kA2iRecInts = 4;
constexpr int kA2iRecFlags = 0;   // status | verdict << 8 | substring << 9 | m << 16
constexpr int kA2iRecDiag = 1;    // d = target position - read position of the ungapped frame
constexpr int kA2iRecMask = 2;    // bit k: k < la - 5, target[k] == from_base, read[k - d] == to_base
constexpr int kA2iRecTarget = 3;  // target id (-1 = none)
// status
constexpr uint32_t kA2iSimple = 0, kA2iEnds = 1, kA2iGapped = 2, kA2iNoScore = 3, kA2iUnsupported = 4;
constexpr uint32_t kA2iTied = 5;  // a row of status 1 that mrg_a2i_settle settled: d, verdict, substring and mask as for 0

struct A2iAlignParams {
  const uint64_t* reads;  // [W][stride]; only word 0 is read (a read beyond 32 nt is unsupported)
  const uint64_t* nmask;  // or nullptr
  const uint8_t* lens;
  const int8_t* pass_id;
  const int32_t* ref_id;
  const uint32_t* idx;    // row -> read
  uint32_t rows;          // rows to align (min(selected, capacity))
  int32_t canon_pass;
  const int32_t* canon_target;   // entry -> target id, device copies
  uint32_t n_canon;
  const int32_t* isomir_target;
  uint32_t n_isomir;
  const uint64_t* target_words;  // one word per target, 2 bits per base
  const uint8_t* target_lens;    // 0 = the target cannot be aligned here (no sequence, beyond 32 nt, not ACGT)
  uint32_t n_targets;
  uint32_t from_base, to_base;   // codes 0..3
  int32_t* rec;                  // [rows][kA2iRecInts]
};

// flags[i] = pass_id[i] is one of the two passes (and keep[i] != 0 where keep is given), flags[n] = 0
hipError_t a2i_flags_launch(const int8_t* pass_id, const uint8_t* keep, uint64_t n, int32_t canon_pass, int32_t isomir_pass,
                            uint32_t* flags, hipStream_t stream);
// idx[off[i]] = i for every selected read whose slot is below cap (off = exclusive sums of the flags)
hipError_t a2i_scatter_launch(const int8_t* pass_id, const uint8_t* keep, uint64_t n, int32_t canon_pass, int32_t isomir_pass,
                              const uint32_t* off, uint64_t cap, uint32_t* idx, hipStream_t stream);
hipError_t a2i_align_launch(const A2iAlignParams& p, hipStream_t stream);

struct A2iSettleParams {
  const uint64_t* reads;         // as A2iAlignParams
  const uint64_t* nmask;
  const uint8_t* lens;
  uint64_t n_reads;
  const uint32_t* idx;           // row -> read
  int32_t* rec;                  // [k][kA2iRecInts], rewritten in place where a row is settled
  const uint32_t* sel;           // the rows of status 1
  uint32_t n_sel;
  const uint64_t* target_words;
  const uint8_t* target_lens;
  uint32_t n_targets;
  uint32_t from_base, to_base;
  uint32_t* settled;             // += rows settled
};

// flags[i] = row i of rec has status 1, flags[k] = 0
hipError_t a2i_tied_select_launch(const int32_t* rec, uint64_t k, uint32_t* flags, hipStream_t stream);
// sel[off[i]] = i for every row of status 1 (off = exclusive sums of the flags)
hipError_t a2i_tied_scatter_launch(const int32_t* rec, uint64_t k, const uint32_t* off, uint32_t* sel, hipStream_t stream);
hipError_t a2i_settle_launch(const A2iSettleParams& p, hipStream_t stream);

struct A2iDetailArgs {
  const char* path;
  const uint64_t* reads;
  uint32_t W;
  uint64_t stride;
  const uint8_t* lens;
  const uint64_t* nmask;
  uint64_t n;
  uint64_t n_blocks;
  const uint64_t* block_off;        // [n_blocks + 1] into the rows
  const int32_t* block_group;       // [n_blocks]
  const int32_t* block_frame;       // [n_blocks][2]: dashes in front of / behind the target
  const char* const* block_text;    // [n_blocks] or nullptr; a non-null entry is written as it is
  const char* const* group_names;   // [n_groups]
  const char* const* group_targets; // [n_groups]
  uint64_t n_groups;
  const uint32_t* row_read;
  const uint32_t* row_count;
  const uint8_t* row_flags;         // bit 0 = judge_align verdict, bit 1 = retained by the genome filter
  const int32_t* row_d;
};
// Throws std::runtime_error (I/O) or std::invalid_argument (a row that does not fit its block's frame).
void write_a2i_detail(const A2iDetailArgs& a, uint64_t* lines);

}  // namespace mrg
