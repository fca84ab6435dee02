// Predict mode's cluster feature table on the device (predict_features.hip, strung together by mrg_predict_feature_groups,
// _align, _tally and _neighbors in capi.hip): what generate_featureFiles.py and readCluster.py of the reference compute per
// cluster of `<sample>_vs_representative_seq_modified_selected_sorted.tsv`, from the rows mrg_predict_remap_rows leaves --
// the groups of rows and their filter, every row's read aligned to its cluster, the count-weighted column tallies of every
// group's frame with the head / tail positions and the nine feature columns, and the neighbours of every group on its
// chromosome.  Internal header; everything is asynchronous on `stream`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

namespace mrg {

// stat words (zeroed by the caller): set to 1 by the lanes that would read through arrays contradicting each other
constexpr uint32_t kFeatStatBadRow = 0;      // a row names no read or no retained cluster
constexpr uint32_t kFeatStatBadCluster = 1;  // a cluster on no entry, or end - start + 1 is not its sequence length, or its offsets descend
constexpr uint32_t kFeatStatBadGroups = 2;   // group offsets that do not ascend inside the rows, or a group of no cluster
constexpr uint32_t kFeatStatPassed = 3;      // (a counter: the groups that pass the filter)
constexpr uint32_t kFeatStatSorted = 4;      // (the groups the neighbour step ordered)
constexpr uint32_t kFeatStatWords = 8;

// the filter of generate_featureFiles.py
constexpr uint64_t kFeatMinCount = 10;
constexpr uint32_t kFeatMinMembers = 3, kFeatTerminal = 20;

// row status of feat_align_launch; from kFeatRowHost on the row is left to the host and marks its group
constexpr uint8_t kFeatRowSimple = 0;       // one ungapped diagonal, one best cell
constexpr uint8_t kFeatRowTied = 1;         // several best cells, settled as pairwise2 lists them
constexpr uint8_t kFeatRowSkipped = 2;      // its group did not pass the filter: not aligned
constexpr uint8_t kFeatRowHost = 3;
constexpr uint8_t kFeatRowUnsupported = 3;  // read or cluster longer than 32 nt, or a cluster letter other than A/C/G/T
constexpr uint8_t kFeatRowN = 4;            // an N in the read
constexpr uint8_t kFeatRowGapped = 5;       // a gapped path reaches the best ungapped score
constexpr uint8_t kFeatRowUnsettled = 6;    // a tie the settle rule leaves open
constexpr uint8_t kFeatRowNoScore = 7;      // no matching base at all

constexpr uint32_t kFeatNine = 9, kFeatNineWords = 45;  // per feature column: A, T, C, G, dash
constexpr uint32_t kFeatNoRank = 0xffffffffu;           // the chromosome rank of a group that takes no part in the neighbour step

// neighbour flags
constexpr uint8_t kFeatNoUp = 1, kFeatNoDown = 2;
constexpr uint8_t kFeatStateShift = 2;  // bits 2..3: 0 = Null, 1 = Good, 2 = Bad

struct FeatRows {
  uint32_t n_rows;
  const uint32_t* read;
  const uint32_t* cluster;
};

struct FeatReads {
  const uint64_t* words;  // [W][stride]; only word 0 is read (a read beyond 32 nt goes to the host)
  const uint8_t* lens;
  const uint64_t* nmask;  // [W][stride] or null
  const uint32_t* counts;
  uint32_t n;
};

// the retained clusters: cluster j of the rows
struct FeatClusters {
  uint32_t n;
  const uint32_t* entry;
  const uint8_t* strand;
  const uint32_t* start;
  const uint32_t* end;
  const uint32_t* kept;       // the cluster's number is kept[j] + 1
  const uint64_t* seq_off;    // [n + 1]
  const char* orig;           // [orig_len]
  uint64_t orig_len;
};

// flag32[t] = 1 iff row t starts a run of equal cluster (t < n_rows), flag32[n_rows] = 0.  n_rows + 1 lanes.
hipError_t feat_mark_launch(const FeatRows& rows, uint32_t n_reads, uint32_t n_clusters, uint32_t* flag32, uint32_t* stat, hipStream_t stream);

// rank = the exclusive sum of flag32 [n_rows + 1]: row_group[t] = rank[t + 1] - 1; the first row of group g writes
// group_off[g] and group_cluster[g], the last row of all closes group_off.  group_off: [n_rows + 1].
hipError_t feat_starts_launch(const FeatRows& rows, const uint32_t* rank, uint32_t* row_group, uint32_t* group_off, uint32_t* group_cluster,
                              hipStream_t stream);

// One wave per group: its 64-bit count sum, and pass = sum >= 10, members >= 3, start > 20, end < entry_len - 20.
hipError_t feat_filter_launch(uint32_t n_groups, const uint32_t* group_off, const uint32_t* group_cluster, const FeatRows& rows,
                              const FeatReads& reads, const FeatClusters& cl, uint32_t n_entries, const uint32_t* entry_len,
                              uint64_t* group_sum, uint8_t* group_pass, uint32_t* stat, hipStream_t stream);

// cl_word[j] = the cluster's bases, two bits each (A C G T = 0 1 2 3); cl_len[j] = its length, 255 when it is longer than
// 32 or holds another letter.  One lane per cluster.
hipError_t feat_pack_launch(const FeatClusters& cl, uint64_t* cl_word, uint8_t* cl_len, uint32_t* stat, hipStream_t stream);

struct FeatAlignArgs {
  FeatRows rows;
  const uint32_t* row_group;
  uint32_t n_groups;
  const uint8_t* group_pass;
  FeatReads reads;
  uint32_t n_clusters;
  const uint64_t* cl_word;
  const uint8_t* cl_len;
  uint8_t* row_status;
  int32_t* row_diag;      // read base 0 under cluster position d
  uint8_t* row_ident;     // equal columns over the whole overlap
  uint8_t* group_host;    // [n_groups], zeroed by the caller: 1 = a row of the group is left to the host
};

// 32 lanes per row (a2i_align_kernel's layout, with a2i_settle_kernel's second walk for the rows whose best score ends in
// several cells).
hipError_t feat_align_launch(const FeatAlignArgs& a, hipStream_t stream);

struct FeatTallyArgs {
  uint32_t n_groups;
  const uint32_t* group_off;
  const uint32_t* group_cluster;
  const uint8_t* group_pass;
  const uint8_t* group_host;
  FeatRows rows;
  const int32_t* row_diag;
  const uint8_t* row_ident;
  FeatReads reads;
  uint32_t n_clusters;
  const uint8_t* cl_len;
  uint8_t* valid;      // [n_groups] 1 = tallied here and a stable column exists
  int32_t* frame;      // [n_groups][4]: H, T, head, tail (tail negative)
  uint64_t* exact;     // [n_groups] the summed counts of the members whose identity is their length
  uint64_t* nine;      // [n_groups][45]
};

// One wave per group that passed and is not host-marked; the others get valid = 0 and zeros.
hipError_t feat_tally_launch(const FeatTallyArgs& a, hipStream_t stream);

struct FeatNeighborArgs {
  uint32_t n_groups;
  const uint32_t* group_cluster;
  const uint8_t* valid;
  const int32_t* frame;
  FeatClusters cl;
  uint32_t n_entries;
  const uint32_t* entry_rank;  // the position of the entry's name among the sorted names
};

// key_c / key_se / key_r [n_groups]: the three sort keys of every group (cluster-number digits, start << 32 | end, chromosome
// rank or kFeatNoRank), vals[g] = g.
hipError_t feat_keys_launch(const FeatNeighborArgs& a, uint64_t* key_c, uint64_t* key_se, uint64_t* key_r, uint32_t* vals, uint32_t* stat,
                            hipStream_t stream);
// out[j] = in[vals[j]]
hipError_t feat_gather_keys_launch(const uint64_t* in, const uint32_t* vals, uint32_t n, uint64_t* out, hipStream_t stream);

// sorted_rank / order [n_groups]: the groups ordered by (rank, start, end, cluster number).  One lane per position: the
// group's index t on its chromosome, its two distances, the None flags and the state, stored under the GROUP's index;
// stat[kFeatStatSorted] = the groups with a rank.
hipError_t feat_neighbors_launch(const FeatNeighborArgs& a, const uint64_t* sorted_rank, const uint32_t* order, uint32_t* nb_t, int64_t* nb_up,
                                 int64_t* nb_down, uint8_t* nb_flags, uint32_t* stat, hipStream_t stream);

// mrg_write_predict_features (predict_features_write.cpp): `_features.tsv` and `_cluster.txt` from host arrays.  Throws
// std::invalid_argument (arrays that contradict each other, a template that leaves its chromosome: no file is opened) or
// std::runtime_error.
struct FmIndex;
struct FeatWriteArgs {
  const char *features_path, *cluster_path;
  bool mapped;                                   // the table's base name begins `mapped_`: `-1\tNull` in front, else `Null\tNull`
  const std::vector<const FmIndex*>* parts;      // the genome: entry names, lengths and the template bases
  const FmIndex* clusters;                       // the cluster library: entry j's name is retained cluster j's
  uint64_t n_clusters;
  const uint32_t* cl_entry;
  const uint8_t* cl_strand;
  const uint32_t *cl_start, *cl_end;
  const uint64_t* kept_seq_off;
  const char* kept_orig;
  const uint64_t* reads;  // [W][stride]
  uint32_t W;
  uint64_t stride;
  const uint8_t* lens;
  const uint64_t* nmask;  // or null
  const uint32_t* counts;
  uint64_t n_reads;
  uint64_t n_rows;
  const uint32_t* row_read;
  const int32_t* row_diag;
  uint64_t n_groups;
  const uint32_t* group_off;      // [n_groups + 1]
  const uint32_t* group_cluster;
  const int32_t* frame;           // [n_groups][4]: H, T, head, tail
  const uint64_t* exact;
  const uint64_t* nine;           // [n_groups][45]
  const uint32_t* nb_t;
  const int64_t *nb_up, *nb_down;
  const uint8_t* nb_flags;
  const char* const* group_text;  // null, or per group null / its frame as text: the cluster's padded row and every member's, '\n' between
  uint64_t n_order;
  const uint32_t* order;          // the groups to write, in file order
};
// written[0] = blocks of `_cluster.txt`, written[1] = lines of `_features.tsv` below the header
void write_predict_features(const FeatWriteArgs& a, uint64_t* written);

}  // namespace mrg
