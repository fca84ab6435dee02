// The host side of predict mode's report (reference utils/write_novel_report.py; the rule: tests/predict_report_model.py), no
// GPU: the reader of the novel list, the screened table and the cluster file, which validates headers and cluster names and
// interns what the device compares as numbers, and the writers of `_corrected.tsv`, `_novel_miRNAs_report.csv` (both byte
// for byte the reference's) and `_novel_miRNAs_report_profiles.tsv` from the device's arrays.  Lines end at '\n' alone.
// Where this is stricter than the reference: a table line with fewer cells than the header names, a repeated clusterName in
// the table, a cluster name that is not `<sample>:<cluster>:<chr>:<start>_<end><+|->` and a count cell that is no whole
// number are refused when read, not when (and if) the reference would reach them.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "host_write.hpp"
#include "predict_report.hpp"

namespace mrg {

namespace {

// what Python's str.strip() takes for white space in ASCII text
inline bool is_space(char c) { return c == ' ' || (c >= '\t' && c <= '\r') || (c >= '\x1c' && c <= '\x1f'); }

std::string stripped(const char* p, size_t n) {
  while (n && is_space(p[0])) ++p, --n;
  while (n && is_space(p[n - 1])) --n;
  return std::string(p, n);
}
std::string stripped(const std::string& s) { return stripped(s.data(), s.size()); }
std::vector<std::string> split(const std::string& s, char sep) {
  std::vector<std::string> out;
  size_t at = 0;
  for (;;) {
    const size_t e = s.find(sep, at);
    if (e == std::string::npos) break;
    out.emplace_back(s, at, e - at);
    at = e + 1;
  }
  out.emplace_back(s, at);
  return out;
}
// the lines of a text as readlines() gives them: the '\n' stays
std::vector<std::string> raw_lines(const std::string& text) {
  std::vector<std::string> out;
  size_t at = 0;
  while (at < text.size()) {
    const void* nl = std::memchr(text.data() + at, '\n', text.size() - at);
    const size_t end = nl ? (size_t)(static_cast<const char*>(nl) - text.data()) + 1 : text.size();
    out.emplace_back(text, at, end - at);
    at = end;
  }
  return out;
}
std::string read_file(const char* path) {
  File in(path, "rb");
  return in.read_all();
}
size_t index_of(const std::vector<std::string>& cells, const char* name, const char* where) {
  for (size_t i = 0; i < cells.size(); ++i)
    if (cells[i] == name) return i;
  throw std::invalid_argument(std::string(where) + ": no column " + name);
}
// Python's int() of a cell: white space around an optional sign and digits
bool whole_number(const std::string& cell, int64_t* v) {
  const std::string t = stripped(cell);
  size_t k = (t.size() && (t[0] == '+' || t[0] == '-')) ? 1 : 0;
  if (t.size() <= k || t.size() - k > 18) return false;
  int64_t x = 0;
  for (size_t j = k; j < t.size(); ++j) {
    if (t[j] < '0' || t[j] > '9') return false;
    x = x * 10 + (t[j] - '0');
  }
  *v = t[0] == '-' ? -x : x;
  return true;
}
int64_t head_dashes(const std::string& s) {
  size_t k = 0;
  while (k < s.size() && s[k] == '-') ++k;
  return (int64_t)k;
}
int64_t tail_dashes(const std::string& s) {
  size_t k = 0;
  while (k < s.size() && s[s.size() - 1 - k] == '-') ++k;
  return (int64_t)k;
}
std::string joined(const std::vector<std::string>& cells, char sep) {
  std::string out;
  for (size_t i = 0; i < cells.size(); ++i) {
    if (i) out.push_back(sep);
    out += cells[i];
  }
  return out;
}
std::string to_rna(const std::string& s) {
  std::string out(s);
  for (char& c : out)
    if (c == 'T') c = 'U';
  return out;
}
struct Name {   // `<sample>:<cluster>:<chr>:<start>_<end><strand>`
  std::string chr;
  int64_t start = 0, end = 0;
  char strand = '+';
};
bool parse_name(const std::string& name, Name* out) {
  const std::vector<std::string> parts = split(name, ':');
  if (parts.size() != 4 || parts[3].size() < 4) return false;
  out->strand = parts[3].back();
  if (out->strand != '+' && out->strand != '-') return false;
  const std::vector<std::string> span = split(parts[3].substr(0, parts[3].size() - 1), '_');
  if (span.size() != 2 || !whole_number(span[0], &out->start) || !whole_number(span[1], &out->end)) return false;
  out->chr = parts[2];
  return true;
}
std::string line_no(uint64_t i) { return "line " + std::to_string(i + 2) + " of the table"; }

}  // namespace

void read_report_inputs(const char* novel_path, const char* table_path, const char* cluster_path, ReportTable* out) {
  ReportTable& t = *out;
  // ---- the novel list: the first line of every name counts
  std::unordered_map<std::string, uint32_t> rank_of;
  {
    const std::vector<std::string> lines = raw_lines(read_file(novel_path));
    if (lines.empty()) throw std::invalid_argument(std::string(novel_path) + ": no header line");
    const std::vector<std::string> head = split(stripped(lines[0]), ',');
    const size_t i_prob = index_of(head, "probability", novel_path), i_name = index_of(head, "clusterName", novel_path);
    for (size_t li = 1; li < lines.size(); ++li) {
      const std::vector<std::string> c = split(stripped(lines[li]), ',');
      if (c.size() <= std::max(i_prob, i_name))
        throw std::invalid_argument("line " + std::to_string(li + 1) + " of the novel list: fewer cells than the header names");
      if (rank_of.emplace(c[i_name], (uint32_t)t.prob.size()).second) t.prob.push_back(c[i_prob]);
    }
    t.n_listed = t.prob.size();
  }
  // ---- the screened table
  std::vector<std::string> lines = raw_lines(read_file(table_path));
  if (lines.empty()) throw std::invalid_argument(std::string(table_path) + ": no header line");
  t.header_raw = lines[0];
  t.header_cells = split(stripped(lines[0]), '\t');
  const std::vector<std::string>& h = t.header_cells;
  t.i_name = index_of(h, "clusterName", table_path);
  t.i_seq = index_of(h, "pruned_precusor_seq", table_path);
  t.i_str = index_of(h, "pruned_precusor_str", table_path);
  t.i_arm = index_of(h, "armType", table_path);
  t.i_reads = index_of(h, "readCountSum", table_path);
  t.i_stable = index_of(h, "stableClusterSeq", table_path);
  const size_t i_up = index_of(h, "upstreamDistance", table_path), i_down = index_of(h, "downstreamDistance", table_path),
               i_pair = index_of(h, "pair_state", table_path), i_cs = index_of(h, "clusterSeq", table_path),
               i_aligned = index_of(h, "alignedClusterSeq", table_path), i_hul = index_of(h, "headUnstableLength", table_path),
               i_tul = index_of(h, "tailUnstableLength", table_path);
  index_of(h, "seqCount", table_path);
  size_t need = 0;
  for (size_t i : {t.i_name, t.i_seq, t.i_str, t.i_arm, t.i_reads, t.i_stable, i_up, i_down, i_pair, i_cs, i_aligned, i_hul, i_tul}) need = std::max(need, i + 1);
  const uint64_t n = t.n = lines.size() - 1;
  if (n >= (1ull << 28)) throw std::invalid_argument(std::string(table_path) + ": 2^28 lines or more");
  t.raw.assign(std::make_move_iterator(lines.begin() + 1), std::make_move_iterator(lines.end()));
  t.cells.resize(n);
  t.flags.assign(n, 0);
  t.rank.assign(n, 0xffffffffu);
  t.up.assign(n, kReportNone);
  t.down.assign(n, kReportNone);
  t.pos.assign(2 * n, 0);
  t.reads.assign(n, 0);
  t.adj.assign(4 * n, 0);
  t.gid3.assign(3 * n, kReportNoGroup);
  t.t_off.assign(4 * n + 1, 0);
  std::vector<Name> names(n);
  std::unordered_map<std::string, uint32_t> line_of;
  uint64_t found = 0;
  for (uint64_t j = 0; j < n; ++j) {
    std::vector<std::string>& c = t.cells[j];
    c = split(stripped(t.raw[j]), '\t');
    if (c.size() < need) throw std::invalid_argument(line_no(j) + ": fewer cells than the header names");
    if (!parse_name(c[t.i_name], &names[j]))
      throw std::invalid_argument(line_no(j) + ": clusterName is not <sample>:<cluster>:<chr>:<start>_<end><+|->");
    if (!line_of.emplace(c[t.i_name], (uint32_t)j).second) throw std::invalid_argument(line_no(j) + ": clusterName is repeated");
    uint8_t f = 0;
    const auto r = rank_of.find(c[t.i_name]);
    if (r != rank_of.end()) {
      f |= kRepListed;
      t.rank[j] = r->second;
      ++found;
    }
    if (c[i_pair] == "Yes") f |= kRepPairYes;
    if (c[t.i_seq] == "None") f |= kRepPrecNone;
    const std::string& arm = c[t.i_arm];
    f |= (uint8_t)((arm == "arm5" ? kRepArm5 : arm == "arm3" ? kRepArm3 : arm == "loop" ? kRepLoop : kRepArmOther) << kRepArmShift);
    if (names[j].strand == '-') f |= kRepMinus;
    t.flags[j] = f;
    if (c[i_up] != "None" && !whole_number(c[i_up], &t.up[j])) t.up[j] = kReportBad;
    if (c[i_down] != "None" && !whole_number(c[i_down], &t.down[j])) t.down[j] = kReportBad;
    t.pos[2 * j] = names[j].start;
    t.pos[2 * j + 1] = names[j].end;
    int64_t hul = 0, tul = 0;
    if (!whole_number(c[i_hul], &hul) || !whole_number(c[i_tul], &tul) || !whole_number(c[t.i_reads], &t.reads[j]))
      throw std::invalid_argument(line_no(j) + ": headUnstableLength, tailUnstableLength or readCountSum is no whole number");
    if (std::max(std::abs(hul), std::abs(tul)) > 0x3fffffff) throw std::invalid_argument(line_no(j) + ": an unstable length beyond 2^30");
    t.adj[4 * j] = (int32_t)head_dashes(c[i_aligned]);
    t.adj[4 * j + 1] = (int32_t)tail_dashes(c[i_aligned]);
    t.adj[4 * j + 2] = (int32_t)hul;
    t.adj[4 * j + 3] = (int32_t)tul;
    const size_t cols[4] = {t.i_seq, t.i_str, i_cs, t.i_stable};
    for (size_t k = 0; k < 4; ++k) {
      t.text += c[cols[k]];
      t.t_off[4 * j + k + 1] = t.text.size();
    }
  }
  if (found != t.n_listed) {
    for (const auto& kv : rank_of)
      if (!line_of.count(kv.first)) throw std::invalid_argument("the novel list names " + kv.first + ", which the table does not hold");
  }
  // the groups a line can end in: (the precursor of line j - 1, j or j + 1, the line's chr and strand), interned
  {
    std::unordered_map<std::string, uint32_t> ids;
    for (uint64_t j = 0; j < n; ++j)
      for (int d = -1; d <= 1; ++d) {
        if ((d < 0 && j == 0) || (d > 0 && j + 1 == n)) continue;
        const std::string key = t.cells[j + d][t.i_seq] + "\t" + names[j].chr + "\t" + names[j].strand;
        t.gid3[3 * j + (size_t)(d + 1)] = ids.emplace(key, (uint32_t)ids.size()).first->second;
      }
  }
  // ---- the cluster file: the blocks of the table's names; a name's last block counts
  struct Row {
    int64_t start, end, count;
    std::string seq;
  };
  std::vector<std::vector<Row>> rows(n);
  t.blk.assign(n, 0);
  {
    const std::vector<std::string> cl = raw_lines(read_file(cluster_path));
    std::vector<size_t> labels;
    for (size_t i = 0; i < cl.size(); ++i)
      if (cl[i].find("Cluster Name:") != std::string::npos) labels.push_back(i);
    for (size_t k = 0; k < labels.size(); ++k) {
      const size_t lo = labels[k], hi = k + 1 < labels.size() ? labels[k + 1] : cl.size();
      const std::vector<std::string> words = split(stripped(cl[lo]), ' ');
      if (words.size() < 3) continue;
      const auto it = line_of.find(words[2]);
      if (it == line_of.end()) continue;
      const uint32_t j = it->second;
      rows[j].clear();
      t.blk[j] = 2;
      if (hi - lo < 5) continue;
      const std::string dashed = stripped(cl[lo + 4]);
      const bool minus = names[j].strand == '-';
      const int64_t d_start = names[j].start - (minus ? tail_dashes(dashed) : head_dashes(dashed));
      const int64_t d_end = names[j].end + (minus ? head_dashes(dashed) : tail_dashes(dashed));
      bool ok = true;
      for (size_t i = lo + 5; i < hi && ok; ++i) {
        const std::string member = split(cl[i], '\t')[0];
        const std::vector<std::string> c = split(stripped(cl[i]), '\t');
        Row r;
        ok = c.size() >= 2 && whole_number(c[1], &r.count) && r.count >= 0;
        if (!ok) break;
        r.start = d_start + (minus ? tail_dashes(member) : head_dashes(member));
        r.end = d_end - (minus ? head_dashes(member) : tail_dashes(member));
        for (char ch : member)
          if (ch != '-') r.seq.push_back(ch == 'T' ? 'U' : ch);
        rows[j].push_back(std::move(r));
      }
      if (ok) t.blk[j] = 1;
      else rows[j].clear();
    }
  }
  t.r_off.assign(n + 1, 0);
  t.row_soff.assign(1, 0);
  for (uint64_t j = 0; j < n; ++j) {
    for (const Row& r : rows[j]) {
      t.row_start.push_back(r.start);
      t.row_end.push_back(r.end);
      t.row_count.push_back(r.count);
      t.row_text += r.seq;
      t.row_soff.push_back(t.row_text.size());
    }
    t.r_off[j + 1] = t.row_start.size();
  }
  t.n_rows = t.row_start.size();
}

void write_report(const ReportTable& t, const ReportWriteArgs& a) {
  const uint64_t n = t.n, E = a.n_entries;
  if (n && (!a.src || !a.state || !a.pos_adj)) throw std::invalid_argument("null line arrays");
  if (E && (!a.ent_m || !a.ent_p || !a.row_off || !a.prof_off || !a.total || !a.flag)) throw std::invalid_argument("null entry arrays");
  for (uint64_t j = 0; j < n; ++j)
    if (a.src[j] >= n || (a.src[j] > j ? a.src[j] - j : j - a.src[j]) > 1) throw std::invalid_argument(line_no(j) + ": src names no neighbour");
  for (uint64_t e = 0; e < E; ++e) {
    const uint32_t m = a.ent_m[e];
    const int32_t p = a.ent_p[e];
    if (m >= n || p >= (int64_t)n || p < -1) throw std::invalid_argument("entry " + std::to_string(e + 1) + " names no line");
    if (!(t.flags[m] & kRepListed)) throw std::invalid_argument("entry " + std::to_string(e + 1) + ": its mature line is not in the novel list");
    uint64_t rows = t.r_off[m + 1] - t.r_off[m];
    if (p >= 0) rows += t.r_off[p + 1] - t.r_off[p];
    const uint64_t L = t.cells[a.src[m]][t.i_seq].size();
    if (a.row_off[e + 1] - a.row_off[e] != rows || a.prof_off[e + 1] - a.prof_off[e] != L || a.row_off[e] > a.row_off[e + 1] ||
        a.prof_off[e] > a.prof_off[e + 1])
      throw std::invalid_argument("entry " + std::to_string(e + 1) + ": its rows or its profile are not the sizes of its clusters and its precursor");
    if ((rows && (!a.lead || !a.trail)) || (L && !a.prof)) throw std::invalid_argument("null row or profile arrays");
  }
  if (E && (a.row_off[0] != 0 || a.prof_off[0] != 0)) throw std::invalid_argument("offsets that do not start at 0");
  const uint64_t run = env_count("MIRGE_AMD_REPORT_BLOCK_LINES", 2048);   // lines or entries per worker and round (tests lower it)

  // ---- `_corrected.tsv`: a line the correction did not touch and the re-type did not change is written as it was read
  const bool head_touched = n && (t.flags[0] & kRepListed) && (t.flags[0] & kRepPairYes) && t.up[0] != kReportNone && t.up[0] != kReportBad &&
                            t.up[0] <= 44;
  File corrected(a.corrected_path, "wb");
  File report(a.report_path, "wb");
  File profiles(a.profiles_path, "wb");
  corrected.write(head_touched ? joined(t.header_cells, '\t') + "\n" : t.header_raw);
  {
    const uint64_t n_runs = (n + run - 1) / run;
    const unsigned threads = writer_threads(n_runs);
    std::vector<std::string> block(threads);
    in_batches(n_runs, threads,
               [&](unsigned w, uint64_t r) {
                 std::string& b = block[w];
                 b.clear();
                 for (uint64_t j = r * run; j < std::min(n, (r + 1) * run); ++j) {
                   const uint8_t st = a.state[j];
                   if (!(st & (kRepTouched | kRepRetyped))) {
                     b += t.raw[j];
                     continue;
                   }
                   const std::vector<std::string>& c = t.cells[j];
                   const std::vector<std::string>& s = t.cells[a.src[j]];
                   for (size_t i = 0; i < c.size(); ++i) {
                     if (i) b.push_back('\t');
                     if (i == t.i_seq) b += s[t.i_seq];
                     else if (i == t.i_str) b += s[t.i_str];
                     else if (i == t.i_arm && (st & kRepRetyped)) b += "loop";
                     else b += c[i];
                   }
                   b.push_back('\n');
                 }
               },
               [&](uint64_t, unsigned live) {
                 for (unsigned w = 0; w < live; ++w) corrected.write(block[w]);
               });
  }
  corrected.close();

  // ---- the report and the profiles, one entry a line / a block
  report.write(
      "Novel miRNA name,Probability,Chr,Start Pos,End Pos,Strand,Mature miRNA sequence,Arm type,Passenger miRNA sequence,Mature miRNA read "
      "Count,Passenger miRNA read Count,Precursor miRNA sequence,Precursor miRNA structure\n");
  {
    const uint64_t n_runs = (E + run - 1) / run;
    const unsigned threads = writer_threads(n_runs);
    std::vector<std::string> rep(threads), prof(threads);
    in_batches(n_runs, threads,
               [&](unsigned w, uint64_t r) {
                 std::string &b = rep[w], &q = prof[w];
                 b.clear();
                 q.clear();
                 for (uint64_t e = r * run; e < std::min(E, (r + 1) * run); ++e) {
                   const uint32_t m = a.ent_m[e];
                   const int32_t p = a.ent_p[e];
                   const std::vector<std::string>& c = t.cells[m];
                   const std::vector<std::string>& s = t.cells[a.src[m]];
                   const std::vector<std::string> name = split(c[t.i_name], ':');
                   const std::string num = "novel_miRNA_" + std::to_string(e + 1);
                   b += num + "," + t.prob[t.rank[m]] + "," + name[2] + ",";
                   append_int(b, a.pos_adj[2 * (uint64_t)m]);
                   b.push_back(',');
                   append_int(b, a.pos_adj[2 * (uint64_t)m + 1]);
                   b.push_back(',');
                   b.push_back((t.flags[m] & kRepMinus) ? '-' : '+');
                   b += "," + to_rna(c[t.i_stable]) + "," + ((a.state[m] & kRepRetyped) ? std::string("loop") : c[t.i_arm]) + ",";
                   b += (p >= 0 ? to_rna(t.cells[p][t.i_stable]) : std::string("None")) + "," + c[t.i_reads] + ",";
                   b += (p >= 0 ? t.cells[p][t.i_reads] : std::string("None")) + "," + s[t.i_seq] + "," + s[t.i_str] + "\n";
                   // the profile block
                   const uint64_t L = s[t.i_seq].size(), r0 = a.row_off[e], rows = a.row_off[e + 1] - r0;
                   q += ">" + num + "\t";
                   append_int(q, (long long)L);
                   q.push_back('\t');
                   q += std::to_string(a.total[e]);
                   q.push_back('\t');
                   append_int(q, (long long)rows);
                   q += (a.flag[e] & kRepRagged) ? "\t1\n" : "\t0\n";
                   q += s[t.i_seq] + "\n" + s[t.i_str] + "\n";
                   for (uint64_t x = 0; x < L; ++x) {
                     if (x) q.push_back('\t');
                     q += std::to_string(a.prof[a.prof_off[e] + x]);
                   }
                   q.push_back('\n');
                   uint64_t k = 0;
                   for (const int64_t line : {(int64_t)m, (int64_t)p}) {
                     if (line < 0) continue;
                     for (uint64_t row = t.r_off[line]; row < t.r_off[line + 1]; ++row, ++k) {
                       q.append((size_t)std::max(a.lead[r0 + k], 0), '-');
                       q.append(t.row_text, t.row_soff[row], t.row_soff[row + 1] - t.row_soff[row]);
                       q.append((size_t)std::max(a.trail[r0 + k], 0), '-');
                       q.push_back('\t');
                       append_int(q, t.row_count[row]);
                       q.push_back('\n');
                     }
                   }
                 }
               },
               [&](uint64_t, unsigned live) {
                 for (unsigned w = 0; w < live; ++w) {
                   report.write(rep[w]);
                   profiles.write(prof[w]);
                 }
               });
  }
  report.close();
  profiles.close();
}

}  // namespace mrg
