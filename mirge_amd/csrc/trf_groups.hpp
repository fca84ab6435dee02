// `-trf`: the per-sample (sample, tRNA) blocks of tRFs.samples.tmp/ from the rows of mrg_trf_classify (csrc/trf_groups.hip,
// strung together by mrg_trf_sample_groups / mrg_trf_rank in capi.hip) and the writer of <sample>.potential_tRFs.report and
// .potential_tRFs.summary.report (trf_samples_write.cpp, mrg_write_trf_sample_reports).  Internal header: the layouts both
// sides and mirge_amd/trf.py (sample_tables) share, and the one rule for the RP100K value the density peaks see.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mrg {

// Per library entry (host table of mirge_amd.trf.sample_tables, over the entries of trf.entry_tables), int32 [E][4].
constexpr uint32_t kTrfSampleInts = 4;
constexpr int kTrfSampleName = 0;      // rank of the entry's name among the distinct names, Python string order
constexpr int kTrfSampleTemplate = 1;  // bases of the block's template (-1: the lookup raises)
constexpr int kTrfSampleFlags = 2;     // bit 0: "pre_" in name (summary key), bit 1: "pre" in name (template, its label)
constexpr uint32_t kTrfMaxTemplate = 255;
constexpr uint32_t kTrfNone = 0xFFFFFFFFu;

// stat words of the item pass
constexpr int kTrfStatNoTemplate = 0;  // min tsv row of an item whose entry has no template (kTrfNone: none)
constexpr int kTrfStatBadRow = 1;      // min tsv row with a read, entry or start out of range
constexpr int kTrfStatMaxLen = 2;      // longest read of a selected row
constexpr int kTrfStatHasN = 3;        // a printed row holds an N
constexpr int kTrfStatItems = 4;       // items
constexpr uint32_t kTrfStatWords = 8;

// The exact RP100K of an item, the double the Python route carries.
__host__ __device__ inline double trf_rp100k(uint64_t count, uint64_t denom) {
  return denom ? 100000.0 * (double)count / (double)denom : 0.0;
}

// float("%.3f" % round(x, 3)) for x = trf_rp100k(count, denom) in integers: x = m * 2^e exactly, k = m * 1000 * 2^e rounded
// to the nearest integer, ties to even, from the shifted-out remainder; the value is the double quotient k / 1000.0.
// (m * 1000 < 2^63.  A value with e >= 0 is an integer and is its own 3-decimal text.)
__host__ __device__ inline double trf_rp100k_text(uint64_t count, uint64_t denom) {
  const double x = trf_rp100k(count, denom);
  union {
    double d;
    uint64_t u;
  } bits;
  bits.d = x;
  const uint32_t field = (uint32_t)((bits.u >> 52) & 0x7FF);
  const uint64_t frac = bits.u & ((1ull << 52) - 1);
  if (field == 0x7FF || (field == 0 && frac == 0)) return x;
  const uint64_t m = field ? (frac | (1ull << 52)) : frac;
  const int e = (field ? (int)field : 1) - 1075;
  if (e >= 0) return x;
  const uint32_t sh = (uint32_t)(-e);
  if (sh >= 64) return 0.0;
  const uint64_t prod = m * 1000ull;
  uint64_t k = prod >> sh;
  const uint64_t rem = prod & ((1ull << sh) - 1), half = 1ull << (sh - 1);
  if (rem > half || (rem == half && (k & 1))) ++k;
  return (double)k / 1000.0;
}

struct TrfGroupParams {
  const uint64_t* reads;  // [W][stride]
  const uint64_t* nmask;  // or nullptr
  const uint8_t* lens;
  uint64_t stride, n;
  uint32_t W;
  const uint32_t* quant;  // [n][S]
  uint32_t S;
  const int32_t* rec;     // [k][kTrfRecInts], in the order of the tsv
  uint32_t k;
  const int32_t* entries; // [E][kTrfSampleInts]
  uint32_t n_entries, n_names;
};

// Item pass over the pairs i = s * k + r: flags[i] = the pair is a printed row; every item adds its count to sums[s][name],
// lowers rep[s][name] to its entry and counts in printed[s][name] when it is printed; stat as above.  flags[S * k] = 0.
hipError_t trf_items_launch(const TrfGroupParams& p, uint32_t* flags, uint64_t* sums, uint32_t* printed, int32_t* rep, uint32_t* stat,
                            hipStream_t stream);
// item[j] = the pair of printed row j (scan = the exclusive sums of flags, [S * k + 1])
hipError_t trf_item_scatter_launch(const uint32_t* scan, uint64_t total, uint32_t* item, hipStream_t stream);

hipError_t trf_iota_launch(uint32_t* vals, uint32_t n, hipStream_t stream);
// keys[i] = bases [21 c, 21 c + 21) of the read of row vals[i], 3 bits each, first base highest: end of read 0, A 1, C 2,
// G 3, N 4, T 5 (Python string order, a proper prefix first); 0 for a row that is not selected
hipError_t trf_chunk_keys_launch(const TrfGroupParams& p, const uint32_t* vals, uint32_t chunk, uint64_t* keys, hipStream_t stream);
// rank[vals[i]] = i
hipError_t trf_rank_scatter_launch(const uint32_t* vals, uint32_t n, uint32_t* rank, hipStream_t stream);
// printed row j: keys[j] = (255 - start) << rank_bits | (k - 1 - rank of its read), vals[j] = j
hipError_t trf_order_keys_a_launch(const TrfGroupParams& p, const uint32_t* item, uint32_t n_rows, const uint32_t* rank, uint32_t rank_bits,
                                   uint64_t* keys, uint32_t* vals, hipStream_t stream);
// keys[i] = block position of printed row vals[i] << 32 | ~count
hipError_t trf_order_keys_b_launch(const TrfGroupParams& p, const uint32_t* item, const uint32_t* vals, uint32_t n_rows,
                                   const uint32_t* cell_block, uint64_t* keys, hipStream_t stream);

struct TrfPackOut {
  uint32_t words;       // of the template frame, 1..8
  uint64_t row_stride;  // of codes / nmask
  uint64_t* codes;
  uint64_t* nmask;      // or nullptr: no printed row holds an N
  uint16_t* span;
  double* rpm;
  uint32_t* row;        // [n_rows][3]: tsv row, count, type
};
// one lane per printed row, in their final order (vals)
hipError_t trf_pack_launch(const TrfGroupParams& p, const uint32_t* item, const uint32_t* vals, uint32_t n_rows, const uint64_t* denom,
                           const TrfPackOut& out, hipStream_t stream);

// mrg_trf_rank: keys[i] = group of row i << 32 | ~bits of rho[i], vals[i] = i; then rank[p] = vals[p] - off[group]
hipError_t trf_rank_keys_launch(const uint32_t* off, uint32_t n_groups, const float* rho, uint32_t n_rows, uint64_t* keys, uint32_t* vals,
                                hipStream_t stream);
hipError_t trf_rank_local_launch(const uint32_t* off, const uint64_t* keys, const uint32_t* vals, uint32_t n_rows, uint32_t* rank,
                                 hipStream_t stream);

struct TrfSampleWriteArgs {
  const char* const* paths;          // [2 S]: report, summary report of each sample
  uint32_t S;
  const uint64_t* denom;             // [S]
  const uint64_t* reads;
  uint32_t W;
  uint64_t stride;
  const uint8_t* lens;
  const uint64_t* nmask;
  uint64_t n;
  const uint32_t* quant;             // [n][S]
  const int32_t* rec;                // [k][12], in the order of the tsv
  uint64_t k;
  const int32_t* entries;            // [E][4]
  const char* const* entry_names;    // [E]
  const char* const* templates;      // [E]
  const char* const* aa_types;       // [E]
  uint64_t n_entries;
  uint32_t n_names;
  const int32_t* blocks;             // [B][6]: sample, representative entry, first and number of printed rows, group, 0
  const uint64_t* block_sums;        // [B]
  uint64_t n_blocks;
  const uint32_t* rows;              // [R][3]: tsv row, count, type
  uint64_t n_rows;
};
// Throws std::runtime_error (I/O) or std::invalid_argument (inconsistent tables).
void write_trf_sample_reports(const TrfSampleWriteArgs& a);

}  // namespace mrg
