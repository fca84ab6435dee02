// Predict mode's second mapping on the device (predict_remap.hip, strung together by mrg_predict_trim_reads and
// mrg_predict_remap_rows in capi.hip): the per-read and per-row work between the two bowtie passes of the reference's
// miRge2.0.py:566-601 and its `sort -k6,6 -k1,1` -- picking the reads pass 1 left unaligned, cutting them for pass 2,
// merging the two listings into rows and ordering the rows as the sorted table has them.  Internal header; everything is
// asynchronous on `stream`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mrg {

// stat words of mrg_predict_remap_rows (zeroed by the caller): set to 1 by the kernels when an input array contradicts another
constexpr uint32_t kRemapStatBadOffsets = 0;  // a listing's offsets do not ascend from 0 to its rows
constexpr uint32_t kRemapStatBadCluster = 1;  // a row's entry is no retained cluster, or its offset is negative
constexpr uint32_t kRemapStatBadRead = 2;     // a pass-2 read's index is no read
constexpr uint32_t kRemapStatWords = 4;

// A name's number as a sort key: its decimal digits from bit 39 down, four bits each, the rest filled with 15 -- the byte
// order of `<digits>_` among names whose numbers differ (`_` sorts after every digit, so `10_` comes before `1_`).
constexpr uint32_t kRemapKeyBits = 40;  // ten digits: numbers up to 2^32

// flag32[r] = 1 iff read r has no alignment in any of the four strata of counts [4][n] (mrg_list_valid_count's layout);
// flag32[n] = 0 closes the scan's input.  n + 1 lanes.
hipError_t remap_mark_launch(const uint32_t* counts, uint32_t n, uint32_t* flag32, hipStream_t stream);

// sel[rank[r]] = r for every marked read (rank: the exclusive sum of flag32, [n + 1]).
hipError_t remap_compact_launch(uint32_t n, const uint32_t* rank, uint32_t* sel, hipStream_t stream);

struct RemapReads {
  const uint64_t* words;  // [W][stride]
  uint32_t W;
  uint64_t stride;
  const uint8_t* lens;    // [n]
  const uint64_t* nmask;  // [W][stride] or null
  uint32_t n;
};

// The reads sel[0 .. k) as a packed set of their own, [W][k], with t5 bases cut at the 5' end and t3 at the 3' end (bowtie's
// -5 / -3): out_lens[j] = max(0, len - t5 - t3), the words and the N mask shifted down by 2 t5 bits across the 64-bit word
// boundaries, every bit at and beyond the new length zero.  One lane per output word.
hipError_t remap_trim_launch(const RemapReads& in, const uint32_t* sel, uint32_t k, uint32_t t5, uint32_t t3, uint64_t* out_words,
                             uint8_t* out_lens, uint64_t* out_nmask, hipStream_t stream);

// One listing of mrg_list_valid_fill against the cluster library: read r owns rows [off[r], off[r + 1]).
struct RemapListing {
  const uint64_t* off;  // [n + 1]
  uint32_t n;
  const int32_t* ref;   // [rows] the cluster library's entry
  const int32_t* pos;   // [rows]
  const uint8_t* mm;    // [rows]
  uint32_t rows;
};

struct RemapRows {
  uint32_t* read;
  uint32_t* cluster;
  uint32_t* offset;
  uint8_t* mm;
  uint8_t* pass;  // 0 = pass 1, 1 = pass 2
};

struct RemapMergeArgs {
  RemapListing p1, p2;
  const uint32_t* sel;      // [p2.n] the read of every pass-2 read
  uint32_t n_reads;         // = p1.n
  const uint32_t* numbers;  // [n_reads] the n of `mir<n>_<count>`
  uint32_t n_clusters;
  const uint32_t* kept;     // [n_clusters] the cluster's number is kept[j] + 1
  RemapRows rows;           // [p1.rows + p2.rows] in listing order: pass 1, then pass 2
  uint64_t* read_key;
  uint64_t* cluster_key;
  uint32_t* vals;           // vals[t] = t
  uint32_t* stat;
};

// One lane per row of the two listings: its read (the owner of its row range), cluster, offset, mismatches and pass, and the
// two sort keys.  A row whose arrays contradict each other sets a stat word and becomes a row of read 0, cluster 0.  The grid
// holds at least one lane per read of either listing too: lane t checks that read t's offsets ascend.
hipError_t remap_merge_launch(const RemapMergeArgs& a, hipStream_t stream);

// out[j] = in[vals[j]] (the cluster keys between the two sorts).
hipError_t remap_gather_keys_launch(const uint64_t* in, const uint32_t* vals, uint32_t rows, uint64_t* out, hipStream_t stream);

// out row j = in row vals[j]: the rows in file order.
hipError_t remap_gather_rows_launch(const RemapRows& in, const uint32_t* vals, uint32_t rows, const RemapRows& out, hipStream_t stream);

}  // namespace mrg
