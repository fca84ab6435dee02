// Predict mode's location clusters on the device (predict_cluster.hip): the alignment rows of the genome listing are
// sorted by coordinate and merged where they overlap -- what the reference does with samtools and a Python loop
// (utils/cluster_basedon_location.py).  Internal header of capi.hip; everything is asynchronous on `stream`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mrg {

// Key of an alignment row, over `pos_bits + 1 + entry bits` bits:
//   kClusterOrder  entry | strand | position     the (entry, strand) lists of the cluster rule, each in position order
//   kSamOrder      entry | position | strand     a coordinate-sorted SAM file, + before - at one position
constexpr int32_t kClusterOrder = 0, kSamOrder = 1;

// Per-row arrays of one clustering run, carved out of one caller-owned buffer of cluster_work_bytes(rows) bytes.
struct ClusterWork {
  uint32_t* end;     // 1-based inclusive end of the row's alignment
  uint32_t* runmax;  // inclusive maximum of `end` over the row's (entry, strand) list so far
  uint32_t* chead;   // 1 = the row opens a cluster
  uint32_t* cinc;    // inclusive sum of chead: the row's cluster is cinc - 1
  uint8_t* lhead;    // 1 = the row opens an (entry, strand) list
  uint64_t* n_valid; // rows on kept entries (they sort in front of the others)
};
size_t cluster_work_bytes(uint64_t rows);
ClusterWork cluster_work(void* buf, uint64_t rows);

struct ClusterKeysArgs {
  const uint64_t* offsets;  // [n_reads + 1] rows of this part per read
  uint64_t n_reads;
  const int32_t* ref;       // this part's rows
  const int32_t* pos;
  const uint8_t* strand;
  uint32_t rows, entry_base, row_base, n_entries, pos_bits;
  int32_t order;
  const uint8_t* entry_keep;  // [n_entries] or null: rows of an entry with 0 get the entry number n_entries
  uint64_t* keys;             // written at row_base + k
  uint32_t* vals;             // = row_base + k
  uint32_t* owner;            // = the row's read
};
hipError_t cluster_keys_launch(const ClusterKeysArgs& a, hipStream_t stream);

// ends, list heads, the members' reads; then (after the caller's segmented max-scan of `end` into `runmax`) the
// cluster heads under the overlap threshold t
hipError_t cluster_rows_launch(const uint64_t* keys, const uint32_t* vals, uint32_t rows, const uint32_t* owner, const uint8_t* lens,
                               uint32_t n_entries, uint32_t pos_bits, const ClusterWork& w, uint32_t* member, hipStream_t stream);
hipError_t cluster_heads_launch(const uint64_t* keys, uint32_t rows, uint32_t n_entries, uint32_t pos_bits, int32_t t, const ClusterWork& w,
                                hipStream_t stream);

struct ClusterTable {
  uint32_t n_clusters;
  uint32_t n_valid;
  uint32_t* entry;
  uint8_t* strand;
  uint32_t* start;       // 1-based
  uint32_t* end;         // 1-based inclusive
  uint32_t* member_off;  // [n_clusters + 1] into the sorted rows
  uint32_t* len;         // [n_clusters + 1], the last 0: end - start + 1
};
hipError_t cluster_bounds_launch(const uint64_t* keys, uint32_t pos_bits, const ClusterWork& w, const ClusterTable& c, hipStream_t stream);

struct ClusterAssembleArgs {
  const uint64_t* keys;
  uint32_t pos_bits;
  const uint32_t* member;   // the sorted rows' reads
  const uint64_t* reads;    // packed reads [words][n_reads]
  uint32_t words;
  const uint64_t* nmask;    // or null
  const uint8_t* lens;
  uint64_t n_reads;
  const uint32_t* counts;   // per read
  const uint64_t* seq_off;  // [n_clusters + 1]
  char* seq;
  unsigned long long* sum;  // [n_clusters], zeroed
};
hipError_t cluster_assemble_launch(const ClusterAssembleArgs& a, const ClusterWork& w, const ClusterTable& c, hipStream_t stream);

// the sorted rows as columns (for the sorted SAM): read, entry, 0-based offset, strand, mismatches
hipError_t cluster_gather_launch(const uint64_t* keys, const uint32_t* vals, uint32_t rows, uint32_t pos_bits, int32_t order,
                                 const uint32_t* owner, const uint8_t* mm, uint32_t* out_read, int32_t* out_entry, int32_t* out_pos,
                                 uint8_t* out_strand, uint8_t* out_mm, hipStream_t stream);

}  // namespace mrg
