// Predict mode's candidate reads (reference utils/convert2Fasta.py over unmapped.csv) from the arrays `annotate` leaves on
// the device: which unmapped reads enter the raw and the filtered list and their `mir<k>` numbers (mrg_predict_select), one
// sample's rows of either list (mrg_predict_sample_reads), a list as a compact packed read set (mrg_predict_gather) --
// csrc/predict_reads.hip, strung together in capi.hip -- and the host writers of the FASTA files and the read names
// (predict_reads_write.cpp, mrg_write_predict_fasta / mrg_predict_read_names).  Internal header.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mrg {

// quant rows of at least this many sample columns are summed by 16 neighbouring lanes each (coalesced), narrower ones by
// one lane per read
constexpr uint32_t kPredictWideS = 16;
constexpr uint32_t kPredictTotalAll = 0xFFFFFFFFu;  // mrg_predict_gather: `sample` that asks for the row totals

// stat words of mrg_predict_gather
constexpr int kPredictStatBadIndex = 0;  // an index that is no read
constexpr int kPredictStatTooLong = 1;   // a read longer than its words hold
constexpr int kPredictStatOverflow = 2;  // a row total of 2^32 or more asked for as uint32
constexpr uint32_t kPredictStatWords = 4;

struct PredictSelectParams {
  const int8_t* pass_id;
  const uint8_t* lens;
  const uint32_t* quant;  // [n][S]
  uint32_t n, S, min_len, max_len;
  uint64_t cutoff;
};

// total[u] = the sum of quant[u][*]; for an unmapped read (pass_id < 0) raw[u] = total >= 1 and
// sel[u] = min_len <= lens[u] <= max_len && total >= cutoff, else 0; raw[n] = sel[n] = 0
hipError_t predict_flags_launch(const PredictSelectParams& p, uint64_t* total, uint32_t* raw, uint32_t* sel, hipStream_t stream);
// scan = the exclusive sums of flags, [n + 1]: no[u] = scan[u] + 1 where scan[u + 1] > scan[u], else 0
hipError_t predict_numbers_launch(const uint32_t* raw_scan, const uint32_t* sel_scan, uint32_t n, uint32_t* raw_no, uint32_t* sel_no,
                                  hipStream_t stream);
// flags[u] = no[u] != 0 && quant[u][s] >= threshold for u < n, flags[n] = 0
hipError_t predict_sample_flags_launch(const uint32_t* quant, const uint32_t* no, uint32_t n, uint32_t S, uint32_t s, uint64_t threshold,
                                       uint32_t* flags, hipStream_t stream);
// flagged read u: row scan[u] of (idx, num, cnt) = (u, no[u], quant[u][s])
hipError_t predict_sample_fill_launch(const uint32_t* scan, const uint32_t* quant, const uint32_t* no, uint32_t n, uint32_t S, uint32_t s,
                                      uint32_t* idx, uint32_t* num, uint32_t* cnt, hipStream_t stream);

struct PredictGatherParams {
  const uint64_t* reads;  // [W][stride]
  const uint64_t* nmask;  // or nullptr
  const uint8_t* lens;
  const uint32_t* quant;  // [n][S]
  const uint32_t* idx;    // [k]
  uint64_t stride;
  uint32_t n, W, S, sample, k;
  uint64_t* out_reads;  // [W][k]
  uint64_t* out_nmask;  // or nullptr
  uint8_t* out_lens;
  uint32_t* out_counts;
};
// row j < k: read idx[j]'s words, mask, length and its count in `sample` (kPredictTotalAll: its total).  A row whose index
// is no read, whose length its words do not hold or whose total needs more than 32 bits is zero and sets its stat word.
hipError_t predict_gather_launch(const PredictGatherParams& p, uint32_t* stat, hipStream_t stream);

struct PredictFastaArgs {
  const char* path;
  const uint64_t* reads;  // [W][stride]
  uint32_t W;
  uint64_t stride;
  const uint8_t* lens;
  const uint64_t* nmask;  // or nullptr
  uint64_t n;
  const uint32_t* idx;  // [k]
  const uint32_t* num;  // [k]
  const void* counts;   // [k], uint32 or uint64
  uint32_t count_bytes;  // 4 or 8
  uint64_t k;
  const char* const* extra_seqs;  // [n_extra]: the reads beyond 255 nt, in file order
  const uint64_t* extra_nums;
  const uint64_t* extra_counts;
  uint64_t n_extra;
};
// Returns the rows written.  Throws std::invalid_argument (an index that is no read, a number of 0, numbers that do not
// increase: nothing is written) or std::runtime_error (I/O: the file may be left truncated).
uint64_t write_predict_fasta(const PredictFastaArgs& a);
// "mir<num>_<count>" of every row, one after the other without a separator: offsets[j] .. offsets[j + 1] of blob.  Returns
// the bytes of all the names; blob is filled only when cap holds them.
uint64_t predict_read_names(const uint32_t* num, const void* counts, uint32_t count_bytes, uint64_t k, char* blob, uint64_t cap,
                            uint64_t* offsets);

}  // namespace mrg
