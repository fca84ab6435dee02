// `<table>_features.tsv` and `<table>_cluster.txt` of predict mode (reference utils/generate_featureFiles.py and
// classes/readCluster.py; the rule: tests/predict_features_model.py) from host arrays, no GPU: the rows and groups of
// mrg_predict_feature_groups, the diagonals of _align, the frames and nine columns of _tally and the neighbours of
// _neighbors.  A group's frame is built as text -- from (diagonal, read) per member, or taken from the text the caller
// hands in for a group the host worked out (a gapped member has inner dashes) -- and everything is printed from there on
// one path: per column the cluster base's and the majority base's share for `_cluster.txt`, the re-padded frame, the genome
// template and the 63 values of the nine columns for `_features.tsv`.  Floats print as Python 2's str prints them
// (py2_float); the reference's literal 0 prints as `0`.
// Everything is checked before a file is opened.  Blocks of groups are formatted by worker threads and written in order:
// the bytes depend on neither the thread count nor the block length.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "fm_index.hpp"
#include "host_write.hpp"
#include "predict_features.hpp"
#include "tables.hpp"

namespace mrg {

namespace {

const char kOrder[4] = {'A', 'T', 'C', 'G'};  // the reference's column order
const char* const kHeaderHead =
    "realMicRNA\trealMicRNAName\tchr\tstartPos\tendPos\tclusterName\tclusterSeq\tmajoritySeq\tstableClusterSeq\talignedClusterSeq\t"
    "adjustedClusterSeq\tclusterSecondSeq\ttemplateSeq\tseqCount\treadCountSum\texactMatchRatio\theadUnstableLength\ttailUnstableLength\t";

// global entry -> (part, local entry) and the entry's bases with N where the index holds none
struct Genome {
  struct Part {
    const FmIndex* ix;
    uint64_t first_entry;
    std::vector<uint32_t> first_seg;  // segments of local entry e: [first_seg[e], first_seg[e + 1])
  };
  std::vector<Part> parts;
  uint64_t n_entries = 0;

  explicit Genome(const std::vector<const FmIndex*>& ix) {
    for (const FmIndex* p : ix) {
      Part q{p, n_entries, std::vector<uint32_t>(p->names.size() + 1, 0u)};
      for (size_t s = 0; s < p->seg_ref.size(); ++s) {
        if ((s && p->seg_ref[s] < p->seg_ref[s - 1]) || p->seg_ref[s] >= p->names.size() || s + 1 >= p->seg_start.size())
          throw std::invalid_argument("genome index segments out of entry order");
        ++q.first_seg[p->seg_ref[s] + 1];
      }
      for (size_t e = 0; e < p->names.size(); ++e) q.first_seg[e + 1] += q.first_seg[e];
      n_entries += p->names.size();
      parts.push_back(std::move(q));
    }
  }
  const Part& part_of(uint64_t e, uint32_t& local) const {
    size_t k = 0;
    while (k + 1 < parts.size() && parts[k + 1].first_entry <= e) ++k;
    local = (uint32_t)(e - parts[k].first_entry);
    return parts[k];
  }
  const std::string& name(uint64_t e) const {
    uint32_t le;
    return part_of(e, le).ix->names[le];
  }
  uint64_t length(uint64_t e) const {
    uint32_t le;
    const Part& q = part_of(e, le);
    return q.ix->ref_len[le];
  }
  // bases [lo, hi] (1-based, inside the entry) appended to out
  void bases(uint64_t e, uint64_t lo, uint64_t hi, std::string& out) const {
    uint32_t le;
    const Part& q = part_of(e, le);
    const FmIndex& ix = *q.ix;
    for (uint64_t p = lo - 1; p < hi; ++p) {
      uint32_t a = q.first_seg[le], b = q.first_seg[le + 1];
      char ch = 'N';
      while (a < b) {  // the last segment that starts at or before p
        const uint32_t mid = a + (b - a) / 2;
        if (ix.seg_off[mid] <= p) a = mid + 1;
        else b = mid;
      }
      if (a > q.first_seg[le]) {
        const uint32_t s = a - 1;
        const uint64_t in = p - ix.seg_off[s];
        if (in < (uint64_t)ix.seg_start[s + 1] - ix.seg_start[s]) {
          const uint64_t t = (uint64_t)ix.seg_start[s] + in;
          ch = base_char(ix.text[t >> 4] >> ((t & 15) * 2));
        }
      }
      out.push_back(ch);
    }
  }
};

char complement(char c) {
  switch (c) {
    case 'A': return 'T';
    case 'C': return 'G';
    case 'G': return 'C';
    case 'T': return 'A';
    default: return c;
  }
}

[[noreturn]] void bad_group(uint64_t g, const std::string& what) { throw std::invalid_argument("group " + std::to_string(g) + ": " + what); }

void put_ratio(uint64_t num, uint64_t den, std::string& out) { py2_float((double)num / (double)den, out); }

struct Frame {
  std::vector<std::string> rows;  // rows[0] the cluster's, then the members'
  int64_t H = 0, T = 0;
};

// the frame of group g as text, checked against the arrays
void build_frame(const FeatWriteArgs& a, uint64_t g, Frame& fr) {
  const uint64_t r0 = a.group_off[g], r1 = a.group_off[g + 1];
  const uint32_t c = a.group_cluster[g];
  const int32_t* f = a.frame + 4 * g;
  const uint64_t la = a.kept_seq_off[c + 1] - a.kept_seq_off[c];
  fr.H = f[0];
  fr.T = f[1];
  if (fr.H < 0 || fr.T < 0 || fr.H > 255 || fr.T > 255) bad_group(g, "frame out of range");
  fr.rows.assign(1 + (r1 - r0), std::string());
  if (a.group_text && a.group_text[g]) {
    const char* p = a.group_text[g];
    for (std::string& row : fr.rows) {
      const char* e = std::strchr(p, '\n');
      if (!e) e = p + std::strlen(p);
      row.assign(p, (size_t)(e - p));
      p = *e ? e + 1 : e;
    }
    if (*p) bad_group(g, "more rows of text than members");
    const std::string& cl = fr.rows[0];
    const size_t h = cl.find_first_not_of('-'), t = cl.find_last_not_of('-');
    if (h == std::string::npos || (int64_t)h != fr.H || (int64_t)(cl.size() - 1 - t) != fr.T) bad_group(g, "the text's frame is not the arrays'");
    for (const std::string& row : fr.rows)
      if (row.size() != cl.size()) bad_group(g, "rows of text differ in length");
    return;
  }
  const int64_t width = fr.H + (int64_t)la + fr.T;
  fr.rows[0].assign((size_t)fr.H, '-');
  fr.rows[0].append(a.kept_orig + a.kept_seq_off[c], (size_t)la);
  fr.rows[0].append((size_t)fr.T, '-');
  for (uint64_t r = r0; r < r1; ++r) {
    const uint64_t read = a.row_read[r];
    const int64_t L = a.lens[read], at = fr.H + a.row_diag[r];
    if (L > 32 * (int64_t)a.W) bad_group(g, "a read does not fit its words");
    if (at < 0 || at + L > width) bad_group(g, "a read does not fit the frame");
    std::string& row = fr.rows[1 + (r - r0)];
    row.assign((size_t)at, '-');
    unpack_read(a.reads, a.nmask, a.stride, read, (uint32_t)L, row);
    row.append((size_t)(width - at - L), '-');
  }
}

// the dashes calculateFeature adds around the frame and the genome range [lo, hi] (1-based) of the re-padded frame's template
struct Padding {
  int64_t pad_h, pad_t, lo, hi;
};
Padding padding_of(const FeatWriteArgs& a, uint64_t g, const Frame& fr) {
  const uint32_t c = a.group_cluster[g];
  const int64_t head = a.frame[4 * g + 2], tail_add = -(int64_t)a.frame[4 * g + 3] - 1;
  Padding p;
  p.pad_h = std::max<int64_t>(0, 3 - head);
  p.pad_t = std::max<int64_t>(0, 6 - tail_add);
  const int64_t hd = fr.H + p.pad_h, td = fr.T + p.pad_t;
  p.lo = (int64_t)a.cl_start[c] - (a.cl_strand[c] ? td : hd);
  p.hi = (int64_t)a.cl_end[c] + (a.cl_strand[c] ? hd : td);
  return p;
}

void check_all(const FeatWriteArgs& a, const Genome& genome) {
  if (a.n_clusters && (!a.clusters || a.clusters->names.size() != a.n_clusters))
    throw std::invalid_argument("the cluster library does not hold the clusters given");
  if (a.W < 1 || a.W > 8 || a.stride < a.n_reads) throw std::invalid_argument("words_per_read must be 1 .. 8 and the stride cover the reads");
  for (uint64_t c = 0; c < a.n_clusters; ++c) {
    if (a.kept_seq_off[c + 1] < a.kept_seq_off[c]) throw std::invalid_argument("cluster sequence offsets out of order");
    if (a.cl_entry[c] >= genome.n_entries) throw std::invalid_argument("cluster " + std::to_string(c) + " on an unknown entry");
  }
  if (a.n_groups && (a.group_off[0] != 0 || a.group_off[a.n_groups] != a.n_rows)) throw std::invalid_argument("group offsets do not run from 0 to the rows");
  for (uint64_t g = 0; g < a.n_groups; ++g) {
    if (a.group_off[g] >= a.group_off[g + 1] || a.group_off[g + 1] > a.n_rows) bad_group(g, "row offsets do not ascend");
    if (a.group_cluster[g] >= a.n_clusters) bad_group(g, "of an unknown cluster");
  }
  for (uint64_t r = 0; r < a.n_rows; ++r)
    if (a.row_read[r] >= a.n_reads) throw std::invalid_argument("row " + std::to_string(r) + " of an unknown read");
  std::vector<uint8_t> seen(a.n_groups, 0);
  Frame fr;
  for (uint64_t j = 0; j < a.n_order; ++j) {
    const uint64_t g = a.order[j];
    if (g >= a.n_groups) throw std::invalid_argument("position " + std::to_string(j) + " of an unknown group");
    if (seen[g]) bad_group(g, "listed twice");
    seen[g] = 1;
    build_frame(a, g, fr);
    const int64_t width = (int64_t)fr.rows[0].size(), head = a.frame[4 * g + 2], tail = a.frame[4 * g + 3];
    if (head < 0 || head >= width || tail >= 0 || tail < -width || width + tail < head) bad_group(g, "head or tail outside the frame");
    const Padding p = padding_of(a, g, fr);
    const uint32_t c = a.group_cluster[g];
    if (p.lo < 1 || p.hi > (int64_t)genome.length(a.cl_entry[c]))
      throw std::invalid_argument("the template of " + a.clusters->names[c] + " leaves its chromosome");
    if (p.hi - p.lo + 1 != width + p.pad_h + p.pad_t) bad_group(g, "the cluster's coordinates do not span its frame");
    if ((a.nb_flags[g] >> kFeatStateShift) > 2) bad_group(g, "unknown neighbour state");
  }
}

void format_group(const FeatWriteArgs& a, const Genome& genome, uint64_t j, std::string& feats, std::string& clus, uint64_t& lines) {
  const uint64_t g = a.order[j], r0 = a.group_off[g];
  const uint32_t c = a.group_cluster[g];
  Frame fr;
  build_frame(a, g, fr);
  const std::string& cl = fr.rows[0];
  const size_t width = cl.size(), members = fr.rows.size() - 1;
  const int64_t head = a.frame[4 * g + 2], tail = a.frame[4 * g + 3], tail_add = -tail - 1;
  const std::string& chr = genome.name(a.cl_entry[c]);
  const std::string& cname = a.clusters->names[c];
  const char strand = a.cl_strand[c] ? '-' : '+';
  uint64_t total = 0;
  for (size_t m = 0; m < members; ++m) total += a.counts[a.row_read[r0 + m]];
  if (total == 0) bad_group(g, "no counts");

  // ---- `_cluster.txt`
  char num[96];
  clus += "Cluster Name: " + cname + "\n" + chr;
  std::snprintf(num, sizeof num, " (%u - %u%c) cluster %u:\n", a.cl_start[c], a.cl_end[c], strand, a.nb_t[g]);
  clus += num;
  std::string major(width, 'T'), cl_ratios, major_ratios;
  for (size_t x = 0; x < width; ++x) {
    uint64_t t[4] = {0, 0, 0, 0};  // A T C G
    for (size_t m = 0; m < members; ++m) {
      const char ch = fr.rows[1 + m][x];
      for (int b = 0; b < 4; ++b)
        if (ch == kOrder[b]) t[b] += a.counts[a.row_read[r0 + m]];
    }
    if (x) {
      cl_ratios.push_back('\t');
      major_ratios.push_back('\t');
    }
    int at = -1;
    for (int b = 0; b < 4; ++b)
      if (cl[x] == kOrder[b]) at = b;
    if (at < 0) cl_ratios.push_back('0');
    else put_ratio(t[at], total, cl_ratios);
    // the largest tally; equal tallies: T, then G, then C, then A
    static const int kTie[4] = {1, 3, 2, 0};
    int best = kTie[0];
    for (int k = 1; k < 4; ++k)
      if (t[kTie[k]] > t[best]) best = kTie[k];
    major[x] = kOrder[best];
    put_ratio(t[best], total, major_ratios);
  }
  clus += cl + ": " + cl_ratios + "\n" + major + ": " + major_ratios + "\n" + cl + "\n";
  for (size_t m = 0; m < members; ++m) {
    clus += fr.rows[1 + m];
    std::snprintf(num, sizeof num, "\t%u\n", a.counts[a.row_read[r0 + m]]);
    clus += num;
  }

  // ---- `_features.tsv`: only with a stable stretch of at least 7
  const Padding p = padding_of(a, g, fr);
  if ((int64_t)width + p.pad_h + p.pad_t - head - tail_add < 7) return;
  ++lines;
  std::string tmpl;
  genome.bases(a.cl_entry[c], (uint64_t)p.lo, (uint64_t)p.hi, tmpl);
  if (strand == '-') {
    std::reverse(tmpl.begin(), tmpl.end());
    for (char& ch : tmpl) ch = complement(ch);
  }
  size_t top = 0;  // the member with the largest (count, row)
  for (size_t m = 1; m < members; ++m) {
    const uint32_t cm = a.counts[a.row_read[r0 + m]], ct = a.counts[a.row_read[r0 + top]];
    if (cm > ct || (cm == ct && fr.rows[1 + m] > fr.rows[1 + top])) top = m;
  }
  auto without_dashes = [](const std::string& s, size_t lo, size_t hi, std::string& out) {
    for (size_t i = lo; i < hi; ++i)
      if (s[i] != '-') out.push_back(s[i]);
  };
  feats += a.mapped ? "-1\tNull\t" : "Null\tNull\t";
  feats += chr;
  std::snprintf(num, sizeof num, "\t%u\t%u\t", a.cl_start[c], a.cl_end[c]);
  feats += num;
  feats += cname;
  feats.push_back('\t');
  feats.append(a.kept_orig + a.kept_seq_off[c], (size_t)(a.kept_seq_off[c + 1] - a.kept_seq_off[c]));
  feats.push_back('\t');
  without_dashes(fr.rows[1 + top], 0, width, feats);
  feats.push_back('\t');
  without_dashes(cl, (size_t)head, (size_t)((int64_t)width + tail + 1), feats);
  feats.push_back('\t');
  feats += cl;
  feats.push_back('\t');
  for (int which = 0; which < 2; ++which) {  // adjustedClusterSeq, clusterSecondSeq
    feats.append((size_t)p.pad_h, '-');
    feats += fr.rows[which];
    feats.append((size_t)p.pad_t, '-');
    feats.push_back('\t');
  }
  feats += tmpl;
  std::snprintf(num, sizeof num, "\t%zu\t%llu\t", members, (unsigned long long)total);
  feats += num;
  put_ratio(a.exact[g], total, feats);
  std::snprintf(num, sizeof num, "\t%lld\t%lld", (long long)head, (long long)tail_add);
  feats += num;
  const int64_t tp = p.pad_t == 0 ? tail : -6;
  std::string four = "\t0\t0\t0\t0";  // the A, T, C and G shares of the last column that set them
  for (int k = 0; k < 9; ++k) {
    const int64_t x = (k < 3 ? head - 3 + k : (int64_t)width + p.pad_t + tp + (k - 3)) + p.pad_h;  // a column of the padded frame
    const char tn = tmpl[(size_t)x];
    const uint64_t* t = a.nine + 45 * g + 5 * k;  // A T C G dash
    const uint64_t acgt = t[0] + t[1] + t[2] + t[3];
    int at = -1;
    for (int b = 0; b < 4; ++b)
      if (tn == kOrder[b]) at = b;
    feats.push_back('\t');
    feats.push_back(tn);
    feats.push_back('\t');
    if (acgt == 0) {
      feats += "0\t0";
      four = "\t0\t0\t0\t0";
    } else if (at >= 0) {
      const uint64_t other = acgt - t[at];
      put_ratio(t[at], acgt, feats);
      feats.push_back('\t');
      put_ratio(other, acgt, feats);
      four.clear();
      for (int b = 0; b < 4; ++b) {
        four.push_back('\t');
        if (b == at || other == 0) four.push_back('0');
        else put_ratio(t[b], other, four);
      }
    } else {
      feats += "0.0\t0.0";  // (and the previous column's four; four 0 in the first column, where the reference dies)
    }
    feats += four;
  }
  static const char* const kState[3] = {"Null", "Good", "Bad"};
  feats.push_back('\t');
  feats += kState[a.nb_flags[g] >> kFeatStateShift];
  feats.push_back('\t');
  feats += (a.nb_flags[g] & kFeatNoUp) ? "None" : std::to_string((long long)a.nb_up[g]);
  feats.push_back('\t');
  feats += (a.nb_flags[g] & kFeatNoDown) ? "None" : std::to_string((long long)a.nb_down[g]);
  feats.push_back('\n');
}

}  // namespace

void write_predict_features(const FeatWriteArgs& a, uint64_t* written) {
  const Genome genome(*a.parts);
  check_all(a, genome);
  File feats(a.features_path), clus(a.cluster_path);
  std::string header = kHeaderHead;
  if (a.n_order) {
    static const char* const kWhat[7] = {"templateNucleotide", "TemplateNucleotide_percentage", "nonTemplateNucleotide_percentage",
                                         "A_percentage", "T_percentage", "C_percentage", "G_percentage"};
    for (int i = 0; i < 9; ++i)
      for (int w = 0; w < 7; ++w) {
        header += i < 3 ? "head_minus" + std::to_string(3 - i) : "tail_plus" + std::to_string(i - 2);
        header += std::string("_") + kWhat[w] + "\t";
      }
    header += "neighborState\tupstreamDistance\tdownstreamDistance\n";
  }
  feats.write(header);
  const uint64_t run = env_count("MIRGE_AMD_FEATURE_BLOCK_GROUPS", 64);  // groups per worker and round (tests lower it)
  const uint64_t n_runs = (a.n_order + run - 1) / run;
  const unsigned n_threads = writer_threads(n_runs);
  std::vector<std::string> ftext(n_threads), ctext(n_threads);
  std::vector<uint64_t> count(n_threads, 0);
  uint64_t lines = 0;
  in_batches(n_runs, n_threads,
             [&](unsigned t, uint64_t r) {
               ftext[t].clear();
               ctext[t].clear();
               count[t] = 0;
               for (uint64_t j = r * run; j < std::min(a.n_order, (r + 1) * run); ++j) format_group(a, genome, j, ftext[t], ctext[t], count[t]);
             },
             [&](uint64_t, unsigned live) {
               for (unsigned t = 0; t < live; ++t) {
                 feats.write(ftext[t]);
                 clus.write(ctext[t]);
                 lines += count[t];
               }
             });
  feats.close();
  clus.close();
  if (written) {
    written[0] = a.n_order;
    written[1] = lines;
  }
}

}  // namespace mrg
