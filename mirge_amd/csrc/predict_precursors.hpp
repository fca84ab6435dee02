// Predict mode's precursor candidates on the device (predict_precursors.hip, strung together by mrg_predict_precursors and
// mrg_predict_precursor_bases in capi.hip): what get_precursors.py of the reference cuts out of the genome for every line
// of `_features.tsv` -- two windows around the stable part of the cluster, 70 nt upstream and 20 downstream, and 20 and 70,
// reverse-complemented on the minus strand and transcribed -- from the groups mrg_predict_feature_neighbors ordered and the
// packed text of the resident genome libraries.  The rule: tests/predict_precursors_model.py.  Internal header; everything
// is asynchronous on `stream`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

namespace mrg {

// stat words (zeroed by the caller): set to 1 by the lanes that would read through arrays contradicting each other
constexpr uint32_t kPrecStatBadGroup = 0;    // `order` names no group, or one without a stable column (valid == 0)
constexpr uint32_t kPrecStatBadCluster = 1;  // a group of no retained cluster
constexpr uint32_t kPrecStatBadEntry = 2;    // a cluster on no entry
constexpr uint32_t kPrecStatBadWindow = 3;   // a window that ends at or before the chromosome's first base
constexpr uint32_t kPrecStatBadRecord = 4;   // record offsets that do not ascend by hi - lo, or a record outside its entry
constexpr uint32_t kPrecStatWords = 8;

constexpr int64_t kPrecLong = 70, kPrecShort = 20;  // get_precursors.py: selectRangeList = [(20, 70)]
constexpr int64_t kPrecMinStable = 7;               // the feature writer's rule for a line of `_features.tsv`
constexpr uint32_t kPrecMaxParts = 32;

struct PrecGroups {
  uint32_t n_order;
  const uint32_t* order;  // the groups in file order
  uint32_t n_groups;
  const uint32_t* group_cluster;
  const int32_t* frame;  // [n_groups][4]: H, T, head, tail
  const uint8_t* valid;  // null in the bases step
};

struct PrecClusters {
  uint32_t n;
  const uint32_t* entry;
  const uint8_t* strand;
  const uint32_t* start;
  const uint32_t* end;
  uint32_t n_entries;
  const uint32_t* entry_len;
};

// one resident genome library: global entries [entry_base, entry_base + n_ref)
struct PrecPart {
  const uint32_t* text;       // two bits a base, sixteen bases a word
  const uint32_t* seg_start;  // [n_seg + 1] text offsets of the N-free segments
  const uint32_t* seg_off;    // [n_seg] the segment's offset in its entry
  const uint32_t* first_seg;  // [n_ref + 1] segments of local entry e: [first_seg[e], first_seg[e + 1])
  uint32_t entry_base, n_ref;
};
struct PrecGenome {
  uint32_t n_parts;
  PrecPart part[kPrecMaxParts];
};

struct PrecRecords {
  uint32_t n;  // two per written group
  const uint32_t* group;
  const uint32_t* lo;
  const uint32_t* hi;     // bases [lo, hi) of the cluster's entry, 0-based
  const uint64_t* off;    // [n + 1]
};

// One lane per position j of `order`: written[j] and flag32[j] = 1 iff the feature file holds the group's line,
// win[4 j ..] = lo, hi of precusor_1 and of precusor_2, clipped to [0, entry_len].  flag32[n_order] = 0.
hipError_t prec_windows_launch(const PrecGroups& g, const PrecClusters& cl, uint8_t* written, uint32_t* flag32, uint32_t* win, uint32_t* stat,
                               hipStream_t stream);
// rank = the exclusive sum of flag32 [n_order + 1].  The written position j fills records 2 rank[j] and 2 rank[j] + 1:
// rec_group, rec_lo, rec_hi and len32 = hi - lo; the last lane closes len32[2 W] = 0.
hipError_t prec_compact_launch(const PrecGroups& g, const uint32_t* rank, const uint32_t* win, uint32_t* rec_group, uint32_t* rec_lo,
                               uint32_t* rec_hi, uint32_t* len32, hipStream_t stream);
// One lane per record: the checks of kPrecStatBadRecord / BadGroup / BadCluster / BadEntry over arrays handed in.
hipError_t prec_check_launch(const PrecRecords& r, const PrecGroups& g, const PrecClusters& cl, uint64_t seq_len, uint32_t* stat, hipStream_t stream);
// One lane per output byte (the arrays passed prec_check_launch).
hipError_t prec_bases_launch(const PrecRecords& r, const PrecGroups& g, const PrecClusters& cl, const PrecGenome& genome, uint64_t seq_len,
                             char* seq, hipStream_t stream);

// mrg_write_precursors (predict_precursors_write.cpp): `_features_precusor.fa` from host arrays.  Throws
// std::invalid_argument (arrays that contradict each other: no file is opened) or std::runtime_error.
struct FmIndex;
struct PrecWriteArgs {
  const char* path;
  const std::vector<const FmIndex*>* parts;  // the genome: the entries' lengths
  const FmIndex* clusters;                   // the cluster library: entry j's name is retained cluster j's
  uint64_t n_clusters;
  const uint32_t* cl_entry;
  uint64_t n_groups;
  const uint32_t* group_cluster;
  uint64_t n_rec;
  const uint32_t* rec_group;
  const uint32_t *rec_lo, *rec_hi;
  const uint64_t* rec_off;  // [n_rec + 1]
  const char* seq;
  uint64_t seq_len;
};
// written[0] = records, written[1] = bytes of the file
void write_precursors(const PrecWriteArgs& a, uint64_t* written);

}  // namespace mrg
