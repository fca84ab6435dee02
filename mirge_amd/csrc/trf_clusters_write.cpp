// <sample>.potential_tRFs.clusters.detail and <sample>.tRFs.report.tsv of tRFs.samples.tmp/ from the downloaded row layout
// of mrg_trf_sample_groups and the arrays of mrg_trf_assign / mrg_trf_halo (host side, no GPU).  Replaces cluster_text and
// _write_clusters of mirge_amd/trf_samples.py (writeDataToCSV.py:914-1088); the bytes are theirs.
// The RP100K sums are floating point, so each is added in the Python's order by the one thread that owns the group: the halo
// and the core of a cluster over its members in row order, the tRF's own sum from the centre on, the group's sum cluster by
// cluster.  The integer tallies are added here as well and compared with the device's.  The members of a cluster are
// contiguous in `order` (one stable sort on the device), so a group is walked once and groups are independent: runs of
// groups are formatted by worker threads and written in order, and the files depend on neither the thread count nor the
// run size.  Nothing is written before every lookup the record route makes has been found.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "host_write.hpp"
#include "trf_labels.hpp"

namespace mrg {

// repr(float) of Python 3: the shortest digits that read back as the same double (the first precision of a correctly rounded
// %e that does), laid out as float_repr_style 'short' does: exponent form below 1e-4 and from 1e16, ".0" on whole numbers.
std::string py3_float_repr(double v) {
  if (std::isnan(v)) return "nan";
  if (std::isinf(v)) return v < 0 ? "-inf" : "inf";
  if (v == 0.0) return std::signbit(v) ? "-0.0" : "0.0";
  char buf[48];
  for (int p = 0; p <= 16; ++p) {
    std::snprintf(buf, sizeof buf, "%.*e", p, v);
    if (std::strtod(buf, nullptr) == v) break;
  }
  const char* s = buf;
  std::string out;
  if (*s == '-') {
    out.push_back('-');
    ++s;
  }
  std::string digits;
  for (; *s && *s != 'e'; ++s)
    if (*s != '.') digits.push_back(*s);
  const int decpt = std::atoi(s + 1) + 1;
  while (digits.size() > 1 && digits.back() == '0') digits.pop_back();
  const int nd = (int)digits.size();
  if (decpt <= -4 || decpt > 16) {
    out.push_back(digits[0]);
    if (nd > 1) {
      out.push_back('.');
      out.append(digits, 1, std::string::npos);
    }
    char e[16];
    std::snprintf(e, sizeof e, "e%+03d", decpt - 1);
    out += e;
  } else if (decpt <= 0) {
    out += "0.";
    out.append((size_t)-decpt, '0');
    out += digits;
  } else if (decpt >= nd) {
    out += digits;
    out.append((size_t)(decpt - nd), '0');
    out += ".0";
  } else {
    out.append(digits, 0, (size_t)decpt);
    out.push_back('.');
    out.append(digits, (size_t)decpt, std::string::npos);
  }
  return out;
}

namespace {

const char* const kTypeName[7] = {"tRF-1", "tRF-whole", "5'-half", "5'-tRF", "3'-half", "3'-tRF", "i-tRF"};

[[noreturn]] void bad(const char* what, uint64_t at) { throw std::invalid_argument(std::string(what) + " " + std::to_string(at)); }

void append_fmt(std::string& out, const char* fmt, double v) {
  char num[400];
  const int len = std::snprintf(num, sizeof num, fmt, v);
  out.append(num, (size_t)len);
}

struct Cluster {  // one cluster of one group, in the Python's sums
  uint64_t core_count = 0, halo_count = 0, trf_count = 0;
  double core_rpm = 0.0, halo_rpm = 0.0, trf_rpm = 0.0;
  uint32_t members = 0, cores = 0, first_member = 0;
};

struct Group {
  uint64_t sum_count = 0;
  double sum_rpm = 0.0;
};

struct Writer {
  const TrfClusterWriteArgs& a;
  std::vector<Cluster> clusters;
  std::vector<Group> groups;

  explicit Writer(const TrfClusterWriteArgs& args) : a(args), clusters(args.G ? args.cen_off[args.G] : 0), groups(args.G) {}

  uint32_t count_of(uint64_t r) const { return a.rows[3 * r + 1]; }

  // the sums of group g, and its tables against each other
  void analyse(uint32_t g) {
    const uint64_t a0 = a.off[g], size = a.off[g + 1] - a0;
    const uint32_t nc = a.nclust[g], c0 = a.cen_off[g];
    if (a.cen_off[g + 1] < c0 || a.cen_off[g + 1] - c0 != nc || nc > size) bad("centre table does not match NCLUST in group", g);
    if (a.group_len[g] < 1 || (uint32_t)a.group_len[g] > a.max_len || !a.group_names[g] || !a.group_keys[g]) bad("name or template length missing for group", g);
    Group& G = groups[g];
    for (uint64_t r = a0; r < a0 + size; ++r) {
      const uint32_t first = a.span[r] & 0xffu, last = a.span[r] >> 8;
      if (first < 1 || first > last || last > (uint32_t)a.group_len[g] || a.rows[3 * r + 2] > 6) bad("row outside its template:", r);
    }
    if (nc == 0) {
      for (uint64_t r = a0; r < a0 + size; ++r) {
        if (a.labels[r] != -1 || a.core[r]) bad("labelled row in a group without cluster:", r);
        G.sum_count += count_of(r);
        G.sum_rpm += a.rpm[r];
      }
      return;
    }
    uint64_t pos = a0;
    for (uint32_t i = 0; i < nc; ++i) {
      const uint64_t* t = a.tallies + 4ull * (c0 + i);
      Cluster& c = clusters[c0 + i];
      const uint64_t m = t[0];
      if (m > a0 + size - pos || a.centers[c0 + i] >= size) bad("cluster larger than its group:", g);
      const uint64_t center = a0 + a.centers[c0 + i];
      if (a.labels[center] != (int32_t)i + 1) bad("centre outside its cluster in group", g);
      c.members = (uint32_t)m;
      c.first_member = (uint32_t)pos;
      c.trf_count = count_of(center);
      c.trf_rpm = 0.0 + a.rpm[center];
      uint64_t prev = 0;
      for (uint64_t k = 0; k < m; ++k) {
        const uint64_t r = a.order[pos + k];
        if (r < a0 || r >= a0 + size || a.labels[r] != (int32_t)i + 1 || (k && r <= prev)) bad("member order broken at position", pos + k);
        prev = r;
        if (a.core[r]) {
          c.cores += 1;
          c.core_count += count_of(r);
          c.core_rpm += a.rpm[r];
          if (r != center) {
            c.trf_count += count_of(r);
            c.trf_rpm += a.rpm[r];
          }
        } else {
          c.halo_count += count_of(r);
          c.halo_rpm += a.rpm[r];
        }
      }
      if (t[1] != c.cores || t[2] != c.core_count || t[3] != c.halo_count) bad("tallies do not match the rows of group", g);
      pos += m;
      G.sum_count += c.halo_count;
      G.sum_count += c.core_count;
      G.sum_rpm += c.halo_rpm;
      G.sum_rpm += c.core_rpm;
    }
    for (; pos < a0 + size; ++pos) {
      const uint64_t r = a.order[pos];
      if (r < a0 || r >= a0 + size || a.labels[r] != -1 || a.core[r]) bad("member order broken at position", pos);
    }
  }

  void append_seq(std::string& out, uint64_t r, uint32_t L, bool dashes) const {
    const uint32_t first = a.span[r] & 0xffu, last = a.span[r] >> 8;
    if (dashes) out.append(first - 1, '-');
    const size_t at = out.size();
    out.resize(at + (last - first + 1));
    unpack_read(a.codes, a.nmask, a.stride, r, first - 1, last, &out[at]);
    if (dashes) out.append(L - last, '-');
  }

  void append_row(std::string& out, uint64_t r, uint32_t L) const {
    append_seq(out, r, L, true);
    out.push_back('\t');
    out += kTypeName[a.rows[3 * r + 2]];
    out.push_back('\t');
    out += std::to_string(count_of(r));
    out.push_back('\t');
    append_fmt(out, "%.2f", a.rpm[r]);
    out.push_back('\n');
  }

  // cluster_text's `con` of group g
  void format(uint32_t g, std::string& out) const {
    const uint64_t a0 = a.off[g];
    const uint32_t nc = a.nclust[g], c0 = a.cen_off[g], L = (uint32_t)a.group_len[g];
    out += a.group_names[g];
    out += ":\n";
    uint32_t n_out = 0;
    for (uint32_t i = 0; i < nc; ++i) {
      const Cluster& c = clusters[c0 + i];
      if (c.core_count == 0) continue;
      const uint64_t center = a0 + a.centers[c0 + i];
      ++n_out;
      out += "Cluster: " + std::to_string(n_out) + " Total Read Count in Core: " + std::to_string(c.core_count) +
             " Total Read Count in Halo: " + std::to_string(c.halo_count) + " Total RP100K in Core: ";
      append_fmt(out, "%.2f", c.core_rpm);
      out += " Total RP100K in Halo: ";
      append_fmt(out, "%.2f", c.halo_rpm);
      out += " Center Index: " + std::to_string(a.centers[c0 + i] + 1) + " Elements: " + std::to_string(c.members) +
             " Core: " + std::to_string(c.cores) + " Halo: " + std::to_string(c.members - c.cores) + "\nCenter:\n";
      append_row(out, center, L);
      for (uint32_t k = 0; k < c.members; ++k) {
        const uint64_t r = a.order[c.first_member + k];
        if (a.core[r] && r != center) append_row(out, r, L);
      }
      out += "**********************************\n";
    }
    const Group& G = groups[g];
    out += "Summary:\nNumber of Clusters: " + std::to_string(n_out) + "\ntotal Read Count : " + std::to_string(G.sum_count) +
           "\ntotal RP100K: ";
    append_fmt(out, "%.2f", G.sum_rpm);
    for (int halo = 0; halo < 2; ++halo) {
      uint64_t isum = 0;
      double fsum = 0.0;
      std::string ilist, flist;
      for (uint32_t i = 0; i < nc; ++i) {
        const Cluster& c = clusters[c0 + i];
        const uint64_t iv = halo ? c.halo_count : c.core_count;
        const double fv = halo ? c.halo_rpm : c.core_rpm;
        if (i) {
          ilist.push_back('+');
          flist.push_back('+');
        }
        ilist += std::to_string(iv);
        flist += py3_float_repr(fv);
        isum += iv;
        fsum += fv;
      }
      const char* which = halo ? "Halo" : "Core";
      out += std::string("\ntotal Cluster ") + which + " Read Count: " + ilist + "=" + std::to_string(isum);
      out += std::string("\ntotal Cluster ") + which + " RP100K: " + flist + "=";
      append_fmt(out, "%.3f", fsum);
    }
    out += "\n##################################\n";
  }

  // the lines of group g in tRFs.report.tsv under the key t (W2C:1066-1088); false: the record route's IndexError
  bool tsv_lines(uint32_t g, const std::string& t, const char* seq, bool trailer, std::string& out) const {
    const uint64_t a0 = a.off[g];
    const uint32_t nc = a.nclust[g], c0 = a.cen_off[g], L = (uint32_t)a.group_len[g];
    const int64_t n_seq = (int64_t)std::strlen(seq);
    for (uint32_t i = 0; i < nc; ++i) {
      const Cluster& c = clusters[c0 + i];
      if (c.core_count == 0) continue;
      const uint64_t center = a0 + a.centers[c0 + i];
      const int64_t first = a.span[center] & 0xffu, last = a.span[center] >> 8;
      std::string target;
      append_seq(target, center, L, false);
      // detect_mismatch on template[first - 1 : end] (a Python slice), the trailer without its last three bases
      const int64_t n_target = trailer ? std::max<int64_t>(0, (int64_t)target.size() - 3) : (int64_t)target.size();
      int64_t lo = std::min(first - 1, n_seq), hi = trailer ? last - 3 : last;
      if (hi < 0) hi = std::max<int64_t>(0, hi + n_seq);
      hi = std::min(hi, n_seq);
      std::string where;
      for (int64_t k = 0; k < n_target; ++k) {
        if (lo + k >= hi) return false;
        if (target[(size_t)k] != seq[lo + k]) {
          if (!where.empty()) where.push_back(',');
          where += std::to_string(first + k);
        }
      }
      out += t;
      out.push_back('\t');
      out += seq;
      out.push_back('\t');
      out += target;
      out += where.empty() ? "\tN:" : "\tY:";
      out += where;
      out.push_back('\t');
      out += kTypeName[a.rows[3 * center + 2]];
      out += "\t" + std::to_string(first) + ":" + std::to_string(last) + "\t" + std::to_string(c.trf_count) + "\t";
      append_fmt(out, "%.2f", c.trf_rpm);
      out.push_back('\n');
    }
    return true;
  }

  // _write_clusters' second file for the groups [lo, hi) of one sample; false with a.status set: a lookup fails
  bool tsv(uint32_t lo, uint32_t hi, std::string& out) const {
    std::unordered_map<std::string, uint32_t> by_name;
    std::unordered_set<std::string> selected, seen;
    std::vector<std::string> unified;
    for (uint32_t g = lo; g < hi; ++g) {
      by_name[a.group_names[g]] = g;
      if (groups[g].sum_rpm >= 10.0) {
        selected.insert(a.group_names[g]);
        if (seen.insert(a.group_keys[g]).second) unified.push_back(a.group_keys[g]);
      }
    }
    out += "tRNA name\ttRNA sequence\ttRF sequence\ttRF mismatch\ttRF type\ttRF coordinate\tRead count\tRP100K\n";
    for (const std::string& t : unified) {
      for (int trailer = 0; trailer < 2; ++trailer) {
        const std::string name = trailer ? "pre_" + t + "_trailer" : t;
        if (!selected.count(name)) continue;
        const uint32_t g = by_name[name];
        const char* seq = trailer ? a.group_trailer[g] : a.group_mature[g];
        if (!seq || !tsv_lines(g, t, seq, trailer != 0, out)) {
          a.status[0] = seq ? 2 : 1;
          a.status[1] = g;
          return false;
        }
      }
    }
    return true;
  }
};

}  // namespace

void write_trf_cluster_reports(const TrfClusterWriteArgs& a) {
  const uint64_t run_rows = env_count("MIRGE_AMD_TRF_SAMPLE_BLOCK_ROWS", 1u << 14);  // (tests lower it)
  for (uint32_t g = 0; g < a.G; ++g)
    if (a.group_sample[g] < 0 || (uint32_t)a.group_sample[g] >= a.S || (g && a.group_sample[g] < a.group_sample[g - 1]))
      bad("groups are not in sample order at group", g);
  for (uint32_t g = 0; g < a.G; ++g)  // (before any thread indexes the centres and tallies by them)
    if (a.cen_off[0] != 0 || a.cen_off[g + 1] < a.cen_off[g]) bad("centre offsets decrease at group", g);
  // runs of groups of one sample
  struct Run {
    uint32_t lo, hi, s;
  };
  std::vector<Run> runs;
  for (uint32_t g = 0; g < a.G;) {
    const uint32_t s = (uint32_t)a.group_sample[g];
    uint32_t e = g;
    uint64_t rows = 0;
    while (e < a.G && (uint32_t)a.group_sample[e] == s && (e == g || rows < run_rows)) {
      rows += a.off[e + 1] - a.off[e];
      ++e;
    }
    runs.push_back(Run{g, e, s});
    g = e;
  }
  const unsigned n_threads = writer_threads(runs.size());
  Writer w(a);
  in_batches(runs.size(), n_threads,
             [&](unsigned, uint64_t r) {
               for (uint32_t g = runs[r].lo; g < runs[r].hi; ++g) w.analyse(g);
             },
             [](uint64_t, unsigned) {});
  // the second file of every sample, before anything is written
  std::vector<std::string> tsv(a.S);
  uint32_t g = 0;
  for (uint32_t s = 0; s < a.S; ++s) {
    const uint32_t lo = g;
    while (g < a.G && (uint32_t)a.group_sample[g] == s) ++g;
    if (!w.tsv(lo, g, tsv[s])) return;
  }
  std::vector<std::unique_ptr<File>> detail;
  for (uint32_t s = 0; s < a.S; ++s) detail.emplace_back(new File(a.paths[2 * s]));
  std::vector<std::string> text(n_threads);
  in_batches(runs.size(), n_threads,
             [&](unsigned t, uint64_t r) {
               text[t].clear();
               for (uint32_t k = runs[r].lo; k < runs[r].hi; ++k) w.format(k, text[t]);
             },
             [&](uint64_t r0, unsigned live) {
               for (unsigned t = 0; t < live; ++t) detail[runs[r0 + t].s]->write(text[t]);
             });
  for (auto& f : detail) f->close();
  for (uint32_t s = 0; s < a.S; ++s) {
    File f(a.paths[2 * s + 1]);
    f.write(tsv[s]);
    f.close();
  }
}

}  // namespace mrg
