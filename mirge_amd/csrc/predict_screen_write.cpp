// The host side of predict mode's screening (reference utils/screen_precusor_candidates.py; the rule:
// tests/predict_screen_model.py), no GPU: the reader of RNAfold's output, the FASTA of the pruned candidates the second
// fold is fed, and `<table>_features_updated_stableClusterSeq_15.tsv` from the arrays of mrg_predict_screen_features and
// mrg_predict_screen_select.  Everything is checked before an output file is opened.  The table's lines are formatted by
// worker threads in blocks and written in order: the bytes depend on neither the thread count nor the block length.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "host_write.hpp"
#include "predict_screen.hpp"

namespace mrg {

namespace {

// what Python's str.strip() and str.split() take for white space in ASCII text
inline bool is_space(char c) { return c == ' ' || (c >= '\t' && c <= '\r') || (c >= '\x1c' && c <= '\x1f'); }

struct Span {
  const char* p;
  size_t n;
};
inline Span strip(Span s) {
  while (s.n && is_space(s.p[0])) ++s.p, --s.n;
  while (s.n && is_space(s.p[s.n - 1])) --s.n;
  return s;
}
// the lines of a text as readlines() gives them (the last one may lack its newline)
std::vector<Span> lines_of(const std::string& text) {
  std::vector<Span> out;
  size_t at = 0;
  while (at < text.size()) {
    const void* nl = std::memchr(text.data() + at, '\n', text.size() - at);
    const size_t end = nl ? (size_t)(static_cast<const char*>(nl) - text.data()) + 1 : text.size();
    out.push_back(Span{text.data() + at, end - at});
    at = end;
  }
  return out;
}
std::vector<Span> split(Span s) {
  std::vector<Span> out;
  size_t i = 0;
  while (i < s.n) {
    while (i < s.n && is_space(s.p[i])) ++i;
    size_t j = i;
    while (j < s.n && !is_space(s.p[j])) ++j;
    if (j > i) out.push_back(Span{s.p + i, j - i});
    i = j;
  }
  return out;
}
// Python's float() of a stripped token; false where it raises
bool to_double(Span s, double* v) {
  s = strip(s);
  if (s.n == 0 || s.n > 64) return false;
  for (size_t i = 0; i < s.n; ++i)
    if (s.p[i] == 'x' || s.p[i] == 'X' || s.p[i] == 'p' || s.p[i] == 'P') return false;  // (strtod reads hexadecimal floats)
  char buf[65];
  std::memcpy(buf, s.p, s.n);
  buf[s.n] = 0;
  char* end = nullptr;
  *v = std::strtod(buf, &end);
  return end == buf + s.n;
}
// the reference's two-branch parse of `(-12.30)` / `( -2.30)`: 0.0 where it fails
double energy_of(const std::vector<Span>& f) {
  double v = 0.0;
  if (f.size() < 2) return 0.0;
  if (f[1].n >= 3) return to_double(Span{f[1].p + 1, f[1].n - 2}, &v) ? v : 0.0;
  if (f.size() < 3) return 0.0;
  // f[2][:-1]: an empty token cannot occur
  return to_double(Span{f[2].p, f[2].n - 1}, &v) ? v : 0.0;
}

const char* const kArmNames[4] = {"loop", "arm5", "arm3", "unmatchedRegion"};
const char kHeaderTail[] =
    "pruned_precusor_seq\tpruned_precusor_str\tarmType\tdistanceToloop\tpercentage_PairedInMiRNA\thairpin_count\tbinding_count\t"
    "interiorLoopCount\tapicalLoop_size\tstem_length\tmFE\tcount_bindings_in_miRNA\tUGU_UGUG_motif\tpair_state\n";

void format_line(const ScreenWriteArgs& a, Span line, uint64_t i, std::string& out) {
  const Span s = strip(line);
  out.append(s.p, s.n);
  out.push_back('\t');
  if (a.best[i] < 0) {
    for (int k = 0; k < 14; ++k) out += k ? "\tNone" : "None";
    out.push_back('\n');
    return;
  }
  const uint64_t c = 4 * i + (uint64_t)a.best[i];
  const int32_t* f = a.feat + c * kScreenFeatWords;
  out.append(a.p_seq + a.p_off[c], (size_t)(a.p_off[c + 1] - a.p_off[c]));
  out.push_back('\t');
  out.append(a.p_str + a.p_off[c], (size_t)(a.p_off[c + 1] - a.p_off[c]));
  // armTypeOverlenDic[armType][1]: the second miRNA's entry replaces the first's under the same arm
  const int dist = f[kSfArm2] == f[kSfArm1] ? f[kSfDist2] : f[kSfDist1];
  const double percent = f[kSfMirLen] > 0 ? (double)f[kSfBound] / (double)f[kSfMirLen] : 0.0;
  char buf[256];
  std::snprintf(buf, sizeof buf, "\t%s\t%d\t%.2f\t%d\t%d\t%d\t%d\t%d\t%.2f\t%d\t%s\t%s\n", kArmNames[f[kSfArm1]], dist, percent, f[kSfHairpins],
                f[kSfBindings], f[kSfInterior], f[kSfApical], f[kSfStemLen], a.p_mfe[c], f[kSfBound], f[kSfUgu] ? "Yes" : "No",
                f[kSfArm2] >= 0 ? "Yes" : "No");
  out += buf;
}

}  // namespace

void read_str_file(const char* path, uint64_t expected, StrRecords* out) {
  std::string text;
  {
    File in(path, "rb");
    text = in.read_all();
  }
  const std::vector<Span> lines = lines_of(text);
  const uint64_t n = (lines.size() + 2) / 3;
  if (n != expected || lines.size() % 3)
    throw std::invalid_argument(std::string(path) + ": " + std::to_string(n) + " folded records (" + std::to_string(lines.size()) +
                                " lines) for the " + std::to_string(expected) + " sequences of the FASTA");
  out->off.assign(1, 0);
  out->seq.clear();
  out->structure.clear();
  out->mfe.clear();
  for (uint64_t r = 0; r < n; ++r) {
    const Span seq = strip(lines[3 * r + 1]);
    const std::vector<Span> f = split(lines[3 * r + 2]);
    if (f.empty() ? seq.n != 0 : f[0].n != seq.n)
      throw std::invalid_argument(std::string(path) + ": record " + std::to_string(r) + ": the structure's length is not the sequence's");
    out->seq.append(seq.p, seq.n);
    if (!f.empty()) out->structure.append(f[0].p, f[0].n);
    out->off.push_back(out->seq.size());
    out->mfe.push_back(energy_of(f));
  }
}

uint64_t write_pruned_fasta(const char* path, uint64_t n, const uint64_t* off, const char* seq, const uint8_t* keep) {
  for (uint64_t k = 0; k < n; ++k)
    if (off[k] > off[k + 1]) throw std::invalid_argument("offsets that do not ascend at string " + std::to_string(k));
  File fa(path, "wb");
  std::string text;
  uint64_t written = 0;
  for (uint64_t k = 0; k < n; ++k) {
    if (!keep[k]) continue;
    text += ">c" + std::to_string(k) + "\n";
    text.append(seq + off[k], (size_t)(off[k + 1] - off[k]));
    text.push_back('\n');
    ++written;
    if (text.size() > (1u << 20)) {
      fa.write(text);
      text.clear();
    }
  }
  fa.write(text);
  fa.close();
  return written;
}

uint64_t write_screened_features(const ScreenWriteArgs& a) {
  std::string text;
  {
    File in(a.features_path, "rb");
    text = in.read_all();
  }
  const std::vector<Span> lines = lines_of(text);
  const uint64_t have = lines.empty() ? 0 : lines.size() - 1;
  if (have != a.n_lines)
    throw std::invalid_argument(std::string(a.features_path) + ": " + std::to_string(have) + " lines below the header, arrays for " +
                                std::to_string(a.n_lines));
  if (a.p_off[0] != 0) throw std::invalid_argument("the pruned offsets do not start at 0");
  for (uint64_t c = 0; c < 4 * a.n_lines; ++c)
    if (a.p_off[c] > a.p_off[c + 1]) throw std::invalid_argument("the pruned offsets do not ascend at candidate " + std::to_string(c));
  for (uint64_t i = 0; i < a.n_lines; ++i) {
    if (a.best[i] < 0) continue;
    const int32_t* f = a.feat + (4 * i + (uint64_t)a.best[i]) * kScreenFeatWords;
    if (a.best[i] > 3 || f[kSfState] != kScreenOk || f[kSfArm1] < 0 || f[kSfArm1] > 3)
      throw std::invalid_argument("line " + std::to_string(i) + ": the chosen candidate has no feature row");
  }
  File out(a.out_path, "wb");
  if (!lines.empty()) {
    const Span h = strip(lines[0]);
    out.write(std::string(h.p, h.n) + "\t" + kHeaderTail);
  }
  const uint64_t run = env_count("MIRGE_AMD_SCREEN_BLOCK_LINES", 4096);  // lines per worker and round (tests lower it)
  const uint64_t n_runs = (a.n_lines + run - 1) / run;
  const unsigned n_threads = writer_threads(n_runs);
  std::vector<std::string> block(n_threads);
  in_batches(n_runs, n_threads,
             [&](unsigned t, uint64_t r) {
               block[t].clear();
               for (uint64_t i = r * run; i < std::min(a.n_lines, (r + 1) * run); ++i) format_line(a, lines[i + 1], i, block[t]);
             },
             [&](uint64_t, unsigned live) {
               for (unsigned t = 0; t < live; ++t) out.write(block[t]);
             });
  out.close();
  return a.n_lines;
}

}  // namespace mrg
