// `-trf`: typing, selection and cluster assignment of the reads claimed by the mature-tRNA and the pre-tRNA trailer pass
// (csrc/trf_tables.hip, mrg_trf_classify) and the writer of the four tRF tables (trf_tables_write.cpp,
// mrg_write_trf_tables).  Internal header: the layouts both sides and mirge_amd/trf.py share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mrg {

// Per library entry (host table of mirge_amd.trf.entry_tables; the mature_trna entries first, then the pre_trna ones),
// int32 [E][8].
constexpr uint32_t kTrfDescInts = 8;
constexpr int kTrfDescTemplate = 0;   // bases of the template add_dash_new pads to (-1: the lookup raises)
constexpr int kTrfDescTypeLen = 1;    // len(trnaStruDic[name]["seq"]) (trfTypes; unused for a "pre_" name)
constexpr int kTrfDescAnticodon = 2;  // anticodonStart - 1
constexpr int kTrfDescFlags = 3;      // bit 0: "pre_" in name (tRF-1), bit 1: trfTypes raises for this entry
constexpr int kTrfDescRank = 4;       // rank of dup.get(name, name) among all such names, Python string order
constexpr int kTrfDescRep = 5;        // the entry of the same library whose name that is, or -1
constexpr int kTrfDescFirst = 6;      // first predefined tRF of tRNAtrfDic[name]
constexpr int kTrfDescCount = 7;      // how many (0: assign_cluster says "Dele")

// Per predefined tRF, int32 [T][6].
constexpr uint32_t kTrfClusterInts = 6;
constexpr int kTrfClusterFirst = 0;   // coordinate(dashed)[0] (1-based first non-dash position)
constexpr int kTrfClusterLast = 1;    // coordinate(dashed)[1]
constexpr int kTrfClusterLen = 2;     // len(dashed)
constexpr int kTrfClusterWord = 3;    // first word of the dashed string in the text tables
constexpr int kTrfClusterRank = 4;    // rank of the cluster name (ties in distance)
constexpr int kTrfClusterMerged = 5;  // index into trfMergedList, -1: trfMergedNameDic has no such name

// Per kept alignment, int32 [h][4]: entry, start (0-based), end = start + len - 1 - tail, type.
constexpr uint32_t kTrfHitInts = 4;
constexpr uint32_t kTrfType1 = 0, kTrfTypeWhole = 1, kTrfType5Half = 2, kTrfType5 = 3, kTrfType3Half = 4, kTrfType3 = 5, kTrfTypeI = 6,
                   kTrfTypeUnresolvable = 7, kTrfTypeRange = 8;

// Per selected read, int32 [k][12].
constexpr uint32_t kTrfRecInts = 12;
constexpr int kTrfRecRead = 0;      // the read
constexpr int kTrfRecEntry = 1;     // the selected tRNA's entry (-1: none)
constexpr int kTrfRecStart = 2;     // its start, end and type
constexpr int kTrfRecEnd = 3;
constexpr int kTrfRecType = 4;
constexpr int kTrfRecCluster = 5;   // the nearest predefined tRF (-1: none)
constexpr int kTrfRecDistance = 6;  // its get_distance2 (100 for "Dele")
constexpr int kTrfRecKind = 7;
constexpr int kTrfRecHit0 = 8;      // the read's kept alignments: rows [hit0, hit0 + hits) of the hit table, ascending entry
constexpr int kTrfRecHits = 9;
constexpr int kTrfRecTail = 10;     // trailing T's stripped before the listing (0 for the mature pass)
// kind
constexpr uint32_t kTrfAssigned = 0, kTrfUndef = 1, kTrfDele = 2, kTrfUnresolvable = 3, kTrfRange = 4, kTrfNoCandidate = 5;

// flags / scatter of the two passes: iso_flags_launch / iso_scatter_launch (isomir_gff.hpp) with the tRNA passes.

// rows [0, k) = the reads idx[]; row r < n_mature goes to set A ([W][n_mature], whole length), the others to set B
// ([W][k - n_mature], their T tail cut off; length 0 when strip_poly_t's precondition fails).  Bits behind the length are 0.
struct TrfGatherParams {
  const uint64_t* reads;  // [W][stride]
  const uint64_t* nmask;  // or nullptr
  const uint8_t* lens;
  uint64_t stride;
  uint32_t W;
  const uint32_t* idx;
  uint32_t k, n_mature;
  uint64_t *words_a, *nmask_a, *words_b, *nmask_b;  // (nmask_* nullptr with nmask)
  uint8_t* sub_len;   // [k] the listed length
  uint8_t* tail;      // [k]
};
hipError_t trf_gather_launch(const TrfGatherParams& p, hipStream_t stream);

// keys[off[r] + j] = (row0 + r) << (entry_bits + pos_bits) | (entry0 + ref) << pos_bits | pos for the listing of one set
hipError_t trf_keys_launch(const uint64_t* off, const int32_t* ref, const int32_t* pos, uint32_t n_rows, uint32_t row0, uint32_t entry0,
                           uint32_t entry_bits, uint32_t pos_bits, uint64_t out0, uint64_t* keys, hipStream_t stream);
// head[i] = keys[i] starts an (owner, entry) run; head[n] = 0
hipError_t trf_heads_launch(const uint64_t* keys, uint32_t n, uint32_t pos_bits, uint32_t* head, hipStream_t stream);

struct TrfTypeParams {
  const uint64_t* keys;   // sorted
  const uint32_t* slot;   // exclusive sums of the head flags, [n_keys + 1]
  uint32_t n_keys, entry_bits, pos_bits;
  const uint8_t* lens;    // of the reads, [stride]
  const uint32_t* idx;    // row -> read
  const uint8_t* tail;    // [k]
  uint32_t k;
  const int32_t* desc;
  uint32_t n_entries;
  int32_t* hits;          // [kept][4]
  uint32_t* hit0;         // [k] first kept alignment of a row
  uint32_t* hit1;         // [k] one past its last (both zeroed before the launch)
};
hipError_t trf_type_launch(const TrfTypeParams& p, hipStream_t stream);

struct TrfAssignParams {
  const uint64_t* reads;  // [W][stride]
  const uint64_t* nmask;
  const uint8_t* lens;
  uint64_t stride;
  uint32_t W;
  const uint32_t* idx;
  const uint8_t* sub_len;
  const uint8_t* tail;
  uint32_t k, n_mature;
  const int32_t* hits;
  const uint32_t *hit0, *hit1;
  const int32_t* desc;
  uint32_t n_entries;
  const int32_t* clusters;
  uint32_t n_clusters;
  const uint64_t* text;   // the dashed strings, 2 bits per base, each from a word boundary
  const uint64_t* plane;  // bit 2i: base i is no ACGT (code 0 = N, 1 = another character), bit 2i + 1: it is a dash
  int32_t* rec;           // [k][kTrfRecInts]
};
hipError_t trf_assign_launch(const TrfAssignParams& p, hipStream_t stream);

struct TrfWriteArgs {
  const char* const* paths;          // tsv, discarded summary, counts, RP100K
  const char* const* samples;
  uint32_t S;
  const uint64_t* denom;             // [S] maturetrnaReads + pretrnaReads
  const uint64_t* reads;
  uint32_t W;
  uint64_t stride;
  const uint8_t* lens;
  const uint64_t* nmask;
  uint64_t n;
  const uint32_t* quant;             // [n][S]
  const int32_t* rec;                // [k][12], in the order of the tsv
  uint64_t k;
  const int32_t* hits;               // [h][4]
  uint64_t h;
  const int32_t* desc;               // [E][8]
  const char* const* entry_names;    // [E]
  const char* const* aa_types;       // [E] aaType, nullptr: trnaAAanticodonDic has no such name
  const char* const* anticodons;     // [E]
  uint64_t n_entries;
  const int32_t* clusters;           // [T][6]
  uint64_t n_clusters;
  const char* const* merged_names;   // [G] trfMergedList
  uint64_t n_merged;
};
// Throws std::runtime_error (I/O) or std::invalid_argument (a row the Python route would have raised for).
void write_trf_tables(const TrfWriteArgs& a, uint64_t* rows);

}  // namespace mrg
