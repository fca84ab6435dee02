// `-trf`: cluster centres, labels and halos of the density peaks on the device (csrc/trf_labels.hip, strung together by
// mrg_trf_assign / mrg_trf_halo in capi.hip), and the writer of <sample>.potential_tRFs.clusters.detail and
// <sample>.tRFs.report.tsv (trf_clusters_write.cpp, mrg_write_trf_cluster_reports).  Internal header.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

namespace mrg {

constexpr uint32_t kTrfNoRow = 0xFFFFFFFFu;
constexpr float kTrfRhoMin = 5.0f;     // W2C:877
constexpr int32_t kTrfDeltaMin = 8;

// error bits of the assign pass (one word on the device)
constexpr uint32_t kTrfErrTop = 1;         // a group's first rank entry lies outside the group
constexpr uint32_t kTrfErrNeighbour = 2;   // a row's nneigh lies outside its group
constexpr uint32_t kTrfErrUnresolved = 4;  // a row reached no root in the fixed number of rounds (a cycle)

// The rows of all groups, as mrg_trf_rank / mrg_trf_delta left them.
struct TrfAssignIn {
  const uint32_t* off;  // device, n_groups + 1
  uint32_t n_groups, n_rows;
  const float* rho;
  const uint32_t* rank;
  const int32_t* delta;
  const int32_t* nneigh;
};

// grp[i] = the group of row i; per group gdelta = max(0, delta of every row but the top), grho = the largest bits of rho
// (both zeroed by the caller); err |= kTrfErrTop
hipError_t trf_assign_stats_launch(const TrfAssignIn& in, uint32_t* grp, uint32_t* gdelta, uint32_t* grho, uint32_t* err, hipStream_t stream);
// flags[i] = row i is a centre (rho >= 5, delta >= 8, the top's delta = gdelta); flags[n_rows] = 0
hipError_t trf_assign_flags_launch(const TrfAssignIn& in, const uint32_t* grp, const uint32_t* gdelta, uint32_t* flags, hipStream_t stream);
// groups without centre, gdelta <= 8 and max rho >= 5: fb[g] = min row (group-local) of maximal rho (fb preset to kTrfNoRow)
hipError_t trf_assign_fallback_launch(const TrfAssignIn& in, const uint32_t* grp, const uint32_t* scan, const uint32_t* gdelta,
                                      const uint32_t* grho, uint32_t* fb, hipStream_t stream);
// ncl[g] = NCLUST of group g; ncl[n_groups] = 0
hipError_t trf_assign_nclust_launch(const TrfAssignIn& in, const uint32_t* scan, const uint32_t* fb, uint32_t* ncl, hipStream_t stream);
// the forest: lab[i] = the label of a centre (1..NCLUST) or of a top row that is none (-1), else 0 = open, with nxt[i] = its
// nneigh as a row of all groups; centers[cen_off[g] + c - 1] = the group-local row of cluster c; err |= kTrfErrNeighbour
hipError_t trf_assign_init_launch(const TrfAssignIn& in, const uint32_t* grp, const uint32_t* scan, const uint32_t* fb,
                                  const uint32_t* cen_off, int32_t* lab, uint32_t* nxt, uint32_t* centers, uint32_t* err,
                                  hipStream_t stream);
// one round of pointer doubling, from (lab_in, nxt_in) to (lab_out, nxt_out)
hipError_t trf_assign_round_launch(const TrfAssignIn& in, const uint32_t* grp, const int32_t* lab_in, const uint32_t* nxt_in,
                                   int32_t* lab_out, uint32_t* nxt_out, hipStream_t stream);
// label[i] = lab[i]; err |= kTrfErrUnresolved where a row is still open
hipError_t trf_assign_finish_launch(uint32_t n_rows, const int32_t* lab, int32_t* label, uint32_t* err, hipStream_t stream);

struct TrfHaloIn {
  const uint32_t* off;       // device, n_groups + 1
  uint32_t n_groups, n_rows;
  uint64_t stride;           // of codes / nmask
  uint32_t W;
  const uint64_t* codes;
  const uint64_t* nmask;     // or nullptr
  const uint16_t* span;
  const float* rho;
  const int32_t* label;
  const uint32_t* counts;    // read count of row i at counts[i * count_stride]
  uint32_t count_stride;
  const uint32_t* cen_off;   // device, n_groups + 1
  const uint32_t* centers;   // device, group-local rows
  const uint32_t* bord_off;  // device, n_groups + 1
  const float* bord;
};
// core[i], tally[cluster][4] += (members, cores, read count in the core, read count in the halo) (zeroed by the caller),
// keys[i] = group << slot_bits | (label - 1, or NCLUST for label -1), vals[i] = i; err = 1 where a label or a centre is out of range
hipError_t trf_halo_launch(const TrfHaloIn& in, uint32_t slot_bits, uint8_t* core, unsigned long long* tally, uint64_t* keys,
                           uint32_t* vals, uint32_t* err, hipStream_t stream);

struct TrfClusterWriteArgs {
  const char* const* paths;  // [2 S]: clusters.detail, tRFs.report.tsv of each sample
  uint32_t S;
  const uint64_t* codes;     // [W][stride]
  const uint64_t* nmask;     // or nullptr
  uint32_t max_len;
  uint64_t stride;
  const uint16_t* span;
  const double* rpm;
  const uint32_t* rows;      // [n][3]: tsv row, count, type
  uint64_t n_rows;
  const uint32_t* off;       // [G + 1]
  uint32_t G;
  const int32_t* group_sample;            // [G], ascending
  const int32_t* group_len;               // [G] bases of the group's own template
  const char* const* group_names;         // [G] the name the group is paired with
  const char* const* group_keys;          // [G] the tRNA it is reported under
  const char* const* group_mature;        // [G] trnaStruDic[name]["seq"], or NULL
  const char* const* group_trailer;       // [G] pretrnaNameSeqDic[name], or NULL
  const int32_t* labels;
  const uint8_t* core;
  const uint32_t* order;
  const uint32_t* nclust;    // [G]
  const uint32_t* cen_off;   // [G + 1]
  const uint32_t* centers;
  const uint64_t* tallies;   // [cen_off[G]][4]
  int64_t* status;           // [2]: 0 = written, 1 = KeyError, 2 = IndexError of the record route; the group
};
// Throws std::runtime_error (I/O) or std::invalid_argument (inconsistent tables).
void write_trf_cluster_reports(const TrfClusterWriteArgs& a);

// Python 3's repr(float)
std::string py3_float_repr(double v);

}  // namespace mrg
