// Predict mode's report (reference utils/write_novel_report.py without its drawing): the pair correction, the arm re-type,
// the entries and the coverage profiles on the device (predict_report.hip, behind mrg_predict_report_* in capi.hip) and the
// host side around them (predict_report_write.cpp: the reader of the novel list, the screened table and the cluster file,
// and the writers of `_corrected.tsv`, `_novel_miRNAs_report.csv` and `_novel_miRNAs_report_profiles.tsv`).  The rule:
// tests/predict_report_model.py.  Internal header.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

namespace mrg {

constexpr uint32_t kReportMaxPrec = 256;   // a corrected precursor or structure staged in LDS (the screen stage's own limit)
constexpr uint32_t kReportMaxSeq = 255;    // a clusterSeq, stableClusterSeq or read the kernels take
constexpr uint32_t kReportTile = 64;       // read rows staged through LDS at a time
constexpr int64_t kReportMaxPad = 65535;   // a longer run of dashes on one side of a row goes to the host
constexpr int64_t kReportNone = INT64_MIN, kReportBad = INT64_MIN + 1;   // a distance cell: `None`, or no whole number
constexpr uint32_t kReportNoGroup = 0xffffffffu;

// a line's flags, as the reader sets them
enum : uint8_t { kRepListed = 1, kRepPairYes = 2, kRepPrecNone = 4, kRepArmShift = 3, kRepMinus = 32 };
enum : uint8_t { kRepArm5 = 0, kRepArm3 = 1, kRepLoop = 2, kRepArmOther = 3 };
// a line's state, as the correction leaves it: the new arm code sits in bits 4 and 5
enum : uint8_t { kRepTouched = 1, kRepRetyped = 2, kRepHost = 4, kRepNone = 8, kRepStateArmShift = 4 };
// where the reference raises (err [n] per line, chunk_err [n] per chunk)
enum : uint8_t {
  kRepErrUp = 1,        // a qualifying line whose upstreamDistance is no whole number
  kRepErrDown = 2,      // ... whose upstreamDistance exceeds 44 and whose downstreamDistance is None (int('None'))
  kRepErrLast = 3,      // the last line offers to a line that does not exist
  kRepErrListedNone = 4,// a listed name whose precursor is None
  kRepErrUnlisted = 5,  // neither member of a pair is listed, and the chosen mature is not loop
  kRepErrAbsent = 6,    // a stable sequence that the precursor does not hold
  kRepErrBlock = 7,     // no (or a malformed) block in the cluster file
  kRepErrOffsets = 8,   // offsets that do not ascend inside their text (the caller's arrays, not the files)
};
enum : uint8_t { kRepRagged = 1, kRepEntryHost = 2, kRepEntryBad = 4 };   // an entry's flag

struct ReportLines {   // the table's lines on the device
  uint32_t n;
  const uint8_t* flags;    // [n]
  const uint32_t* rank;    // [n] rank in the deduplicated novel list, or 0xffffffff
  const int64_t* up;       // [n]
  const int64_t* down;     // [n]
  const int64_t* pos;      // [n][2] start and end from clusterName
  const int32_t* adj;      // [n][4] head dashes, tail dashes, headUnstableLength, tailUnstableLength
  const int64_t* reads;    // [n] readCountSum
  const uint32_t* gid3;    // [n][3] the interned (precursor of line j-1 / j / j+1, chr, strand)
  const uint64_t* t_off;   // [4 n + 1] precursor, structure, clusterSeq, stableClusterSeq of every line
  const char* text;
  uint64_t text_len;
};
struct ReportLineOut {
  uint32_t* src;           // [n]
  uint8_t* state;          // [n]
  uint8_t* err;            // [n]
  int64_t* pos_adj;        // [n][2]
  int32_t* stable_idx;     // [n] (-1 absent)
  uint32_t* gid;           // [n]
};
struct ReportRows {   // the cluster file's blocks
  const uint8_t* blk;      // [n] 0 missing, 1 read, 2 malformed
  const uint64_t* r_off;   // [n + 1]
  uint64_t n_rows;
  const int64_t* start;    // [n_rows]
  const int64_t* end;
  const int64_t* count;
  const uint64_t* s_off;   // [n_rows + 1]
  const char* text;
  uint64_t text_len;
};
struct ReportEntryScratch {   // pieces of the call's scratch
  uint32_t *key0, *key1, *val0, *val1, *ckey0, *ckey1, *cval0, *cval1, *cm, *emit, *num, *rows32, *len32;
  int32_t* cp;
  void *sort_tmp, *scan_tmp;
};
struct ReportEntryOut {
  uint32_t* ent_m;         // [n]
  int32_t* ent_p;          // [n] (-1 none)
  uint8_t* chunk_err;      // [n]
  uint32_t* chunk_line;    // [n] the chunk's mature line (for the message)
  uint64_t* row_off;       // [n + 1]
  uint64_t* prof_off;      // [n + 1]
  uint32_t* n_entries;     // [1]
};
struct ReportProfileOut {
  int32_t* lead;           // [rows]
  int32_t* trail;          // [rows]
  uint64_t* prof;          // [sum of L]
  uint64_t* total;         // [n_entries]
  uint8_t* flag;           // [n_entries]
};

hipError_t report_correct_launch(const ReportLines& in, const ReportLineOut& out, hipStream_t stream);
hipError_t report_entries_launch(const ReportLines& in, const ReportLineOut& lines, const uint8_t* blk, const uint64_t* r_off,
                                 const ReportEntryScratch& sc, const ReportEntryOut& out, hipStream_t stream);
hipError_t report_profile_launch(const ReportLines& in, const ReportLineOut& lines, const ReportRows& rows, uint32_t n_entries,
                                 const uint32_t* ent_m, const int32_t* ent_p, const uint64_t* row_off, const uint64_t* prof_off,
                                 const ReportProfileOut& out, hipStream_t stream);

// predict_report_write.cpp (host, no GPU).  Throw std::invalid_argument (files that contradict themselves) or std::runtime_error.
struct ReportTable {
  uint64_t n = 0, n_listed = 0, n_rows = 0;
  std::string header_raw;
  std::vector<std::string> header_cells;
  std::vector<std::string> raw;                      // [n] the lines as read
  std::vector<std::vector<std::string>> cells;       // [n] stripped and split
  size_t i_name = 0, i_seq = 0, i_str = 0, i_arm = 0, i_reads = 0, i_stable = 0;
  std::vector<std::string> prob;                     // [n_listed] the probability text by rank
  std::vector<uint8_t> flags, blk;
  std::vector<uint32_t> rank, gid3;
  std::vector<int64_t> up, down, pos, reads, row_start, row_end, row_count;
  std::vector<int32_t> adj;
  std::vector<uint64_t> t_off, r_off, row_soff;
  std::string text, row_text;
};
void read_report_inputs(const char* novel_path, const char* table_path, const char* cluster_path, ReportTable* out);
struct ReportWriteArgs {
  const uint32_t* src;
  const uint8_t* state;
  const int64_t* pos_adj;
  uint64_t n_entries;
  const uint32_t* ent_m;
  const int32_t* ent_p;
  const uint64_t* row_off;
  const int32_t* lead;
  const int32_t* trail;
  const uint64_t* prof_off;
  const uint64_t* prof;
  const uint64_t* total;
  const uint8_t* flag;
  const char* corrected_path;
  const char* report_path;
  const char* profiles_path;
};
void write_report(const ReportTable& t, const ReportWriteArgs& a);

}  // namespace mrg
