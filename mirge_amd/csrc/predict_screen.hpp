// Predict mode's screening of the folded precursor candidates on the device (predict_screen.hip, strung together by the
// mrg_predict_screen_* entry points in capi.hip): what screen_precusor_candidates of the reference works out around its
// two folds -- which records of the `.str` are a line's candidates and which miRNAs go with them, the slice
// getPrunedPrecusor cuts, the numbers featuresInPrecusor / percentageOfPairedInMiRNA / bindingsInMiRNA return for the folded
// slice, and selcteOptimalPrecusor's choice.  The rule: tests/predict_screen_model.py.  Internal header; everything is
// asynchronous on `stream`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

namespace mrg {

// stat words (zeroed by the caller): set to 1 by the lanes that find what the word names
constexpr uint32_t kScreenStatBadLine = 0;     // a Good line without the neighbour its distances name (cand_n = 0 there)
constexpr uint32_t kScreenStatBadGroup = 1;    // a line of no group
constexpr uint32_t kScreenStatBadOffsets = 2;  // offsets that do not ascend from 0 to the blob's length
constexpr uint32_t kScreenStatBadCand = 3;     // a candidate of no record or no miRNA
constexpr uint32_t kScreenStatRefused = 4;     // a structure that does not balance, a hairpin loop under 3, or a miRNA the
                                               // reference would index the structure beyond its end with
constexpr uint32_t kScreenStatWords = 8;

constexpr uint32_t kScreenNoIndex = 0xffffffffu;  // an unused candidate slot (cand_rec) or no second miRNA (cand_mir)
constexpr uint32_t kScreenMaxLen = 256;           // characters of a candidate the kernels hold in LDS
constexpr uint32_t kScreenMaxMir = 255;           // characters of a miRNA
constexpr int kScreenMaxElements = 10;            // stems or hairpins from which the last-character quirk can act
constexpr int64_t kScreenNoNeighbour = 10000, kScreenClosest = 9, kScreenFarthest = 44;

// a candidate's status (prune) / the state word of its feature row
constexpr uint8_t kScreenNone = 0;      // pairing_partner gave None / the all-None row
constexpr uint8_t kScreenOk = 1;
constexpr uint8_t kScreenHost = 2;      // beyond the kernels' limits: the caller works it out
constexpr uint8_t kScreenUnused = 3;    // an unused slot
constexpr uint8_t kScreenRefused = 4;   // see kScreenStatRefused

// the arm types, as numbers
constexpr int kArmLoop = 0, kArm5 = 1, kArm3 = 2, kArmUnmatched = 3;

// a feature row: kScreenFeatWords int32
enum ScreenFeat {
  kSfState = 0, kSfHairpins, kSfBindings, kSfInterior, kSfArm1, kSfApical, kSfOver1, kSfDist1, kSfArm2, kSfOver2, kSfDist2, kSfStemLen,
  kSfUgu, kSfBound, kSfMirLen, kSfStems, kScreenFeatWords
};

struct ScreenBlob {   // n strings: bytes [off[i], off[i + 1]) of text (and of text2 where given)
  uint32_t n;
  const uint64_t* off;
  const char* text;
  const char* text2;
  uint64_t len;
};

// One lane per line: cand_n [n_lines] = 2 or 4 (0: kScreenStatBadLine), cand_rec [4 n_lines] = the record (2 line' or
// 2 line' + 1) or kScreenNoIndex, cand_mir [8 n_lines] = the one or two lines whose miRNA goes with the candidate.
hipError_t screen_candidates_launch(uint32_t n_lines, const uint32_t* line_group, uint32_t n_groups, const uint8_t* nb_flags,
                                    const int64_t* nb_up, const int64_t* nb_down, uint8_t* cand_n, uint32_t* cand_rec, uint32_t* cand_mir,
                                    uint32_t* stat, hipStream_t stream);
// One lane per offset: kScreenStatBadOffsets.
hipError_t screen_check_offsets_launch(const ScreenBlob& b, uint32_t* stat, hipStream_t stream);
// One lane per candidate: kScreenStatBadCand.  cand_rec (null: not looked at): an unused slot is skipped; status (null: not
// looked at): a candidate that is not kScreenOk is skipped.
hipError_t screen_check_cands_launch(uint32_t n_cand, const uint32_t* cand_rec, const uint8_t* status, const uint32_t* cand_mir, uint32_t n_rec,
                                     uint32_t n_mir, uint32_t* stat, hipStream_t stream);
// One wave per candidate: status, the slice [lo, hi) of its record and len32 = hi - lo (0 unless kScreenOk); len32[n_cand] = 0.
hipError_t screen_prune_launch(uint32_t n_cand, const uint32_t* cand_rec, const uint32_t* cand_mir, const ScreenBlob& rec, const ScreenBlob& mir,
                               int32_t pruned_length, uint8_t* status, uint32_t* lo, uint32_t* hi, uint32_t* len32, uint32_t* stat,
                               hipStream_t stream);
// One wave per candidate: the bytes of its slice to pruned + pruned_off[c].
hipError_t screen_copy_launch(uint32_t n_cand, const uint32_t* cand_rec, const ScreenBlob& rec, const uint8_t* status, const uint32_t* lo,
                              const uint32_t* hi, const uint64_t* pruned_off, char* pruned, hipStream_t stream);
// One wave per candidate with status kScreenOk: its feature row; the others get kScreenNone rows.
hipError_t screen_features_launch(uint32_t n_cand, const uint8_t* status, const uint32_t* cand_mir, const ScreenBlob& pruned, const ScreenBlob& mir,
                                  int32_t* feat, uint32_t* stat, hipStream_t stream);
// One lane per line: best [n_lines] = the chosen candidate (0..3) or -1.
hipError_t screen_select_launch(uint32_t n_lines, const uint8_t* cand_n, const uint32_t* cand_rec, uint32_t n_rec, const double* rec_mfe,
                                const int32_t* feat, int32_t threshold, int32_t* best, uint32_t* stat, hipStream_t stream);

// predict_screen_write.cpp (host, no GPU).  Throw std::invalid_argument (input that contradicts itself: no file is
// written) or std::runtime_error.
struct StrRecords {
  std::vector<uint64_t> off;  // [n + 1] into seq and structure
  std::string seq, structure;
  std::vector<double> mfe;
};
// the records of an RNAfold output; expected = the FASTA's record count
void read_str_file(const char* path, uint64_t expected, StrRecords* out);
// `>c<k>` records for the n strings of a blob whose keep[k] != 0; returns the records written
uint64_t write_pruned_fasta(const char* path, uint64_t n, const uint64_t* off, const char* seq, const uint8_t* keep);
struct ScreenWriteArgs {
  const char* features_path;
  const char* out_path;
  uint64_t n_lines;
  const int32_t* best;      // [n_lines]
  const int32_t* feat;      // [4 n_lines][kScreenFeatWords]
  const uint64_t* p_off;    // [4 n_lines + 1] into p_seq / p_str
  const char* p_seq;
  const char* p_str;
  const double* p_mfe;      // [4 n_lines]
};
// returns the lines written below the header
uint64_t write_screened_features(const ScreenWriteArgs& a);

}  // namespace mrg
