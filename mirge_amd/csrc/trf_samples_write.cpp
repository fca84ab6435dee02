// <sample>.potential_tRFs.report and <sample>.potential_tRFs.summary.report of tRFs.samples.tmp/ from the columnar arrays and
// the block tables of mrg_trf_sample_groups (host side, no GPU).  Replaces sample_trf_dic / sample_reports of
// mirge_amd/trf_samples.py (writeDataToCSV.py:802-874); the bytes are theirs.
//   <name>\tread count sum:<sum>\tRP100K sum:<%.3f>          per block, blocks without printed row included
//   <dashed read>\t<type>\t<count>\t<%.3f>                   per printed row
//   <template>\t<mature tRNA | primary tRNA trailer>\t<sum>\t<%.3f>
// The RP100K sum of a block is added in one thread over the rows of the tsv, items that overhang the template included, as
// the reference adds it; the summary's counts, RP100K and row numbers are added in print order.  Runs of blocks are
// formatted by worker threads and written in order: the files depend on neither the thread count nor the run size.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "host_write.hpp"
#include "trf_groups.hpp"
#include "trf_tables.hpp"

namespace mrg {

namespace {

const char* const kTypeName[7] = {"tRF-1", "tRF-whole", "5'-half", "5'-tRF", "3'-half", "3'-tRF", "i-tRF"};

[[noreturn]] void bad(const char* what, uint64_t at) { throw std::invalid_argument(std::string(what) + " " + std::to_string(at)); }

void append_fixed3(std::string& out, double v) {
  char num[400];
  const int len = std::snprintf(num, sizeof num, "%.3f", v);
  out.append(num, (size_t)len);
}

struct Row {  // a printed row, resolved and checked
  uint64_t read;
  uint32_t start, len, count, type;
};

Row row_of(const TrfSampleWriteArgs& a, uint64_t at, uint32_t sample, int32_t rep) {
  const uint32_t* x = a.rows + 3 * at;
  if (x[0] >= a.k || x[2] > 6) bad("printed row out of range:", at);
  const int32_t* rec = a.rec + (uint64_t)x[0] * kTrfRecInts;
  const uint64_t read = (uint32_t)rec[kTrfRecRead];
  const int32_t entry = rec[kTrfRecEntry], start = rec[kTrfRecStart];
  if ((uint32_t)rec[kTrfRecKind] > kTrfDele || read >= a.n || entry < 0 || (uint64_t)entry >= a.n_entries || start < 0)
    bad("printed row on an unclassified tsv row:", at);
  const int32_t* en = a.entries + (uint64_t)entry * kTrfSampleInts;
  const int32_t* rp = a.entries + (uint64_t)rep * kTrfSampleInts;
  const uint32_t len = a.lens[read];
  if (en[kTrfSampleName] != rp[kTrfSampleName] || a.quant[read * a.S + sample] != x[1] || x[1] == 0 || len > 32u * a.W ||
      (int64_t)start + len > rp[kTrfSampleTemplate])
    bad("printed row does not belong to its block:", at);
  return Row{read, (uint32_t)start, len, x[1], x[2]};
}

// blocks [lo, hi): their lines of the report
void format_blocks(const TrfSampleWriteArgs& a, const std::vector<double>& rpm_sum, uint64_t lo, uint64_t hi, std::string& text) {
  for (uint64_t b = lo; b < hi; ++b) {
    const int32_t* blk = a.blocks + b * 6;
    const uint32_t s = (uint32_t)blk[0];
    const int32_t rep = blk[1];
    const char* tmpl = a.templates[rep];
    const size_t tlen = std::strlen(tmpl);
    const std::string sum = std::to_string((unsigned long long)a.block_sums[b]);
    text += a.entry_names[rep];
    text += "\tread count sum:";
    text += sum;
    text += "\tRP100K sum:";
    append_fixed3(text, rpm_sum[b]);
    text.push_back('\n');
    for (uint64_t at = (uint32_t)blk[2]; at < (uint64_t)(uint32_t)blk[2] + (uint32_t)blk[3]; ++at) {
      const Row r = row_of(a, at, s, rep);
      text.append(r.start, '-');
      unpack_read(a.reads, a.nmask, a.stride, r.read, r.len, text);
      text.append(tlen - r.start - r.len, '-');
      text.push_back('\t');
      text += kTypeName[r.type];
      text.push_back('\t');
      text += std::to_string(r.count);
      text.push_back('\t');
      append_fixed3(text, trf_rp100k(r.count, a.denom[s]));
      text.push_back('\n');
    }
    text += tmpl;
    text += (a.entries[(uint64_t)rep * kTrfSampleInts + kTrfSampleFlags] & 2) ? "\tprimary tRNA trailer\t" : "\tmature tRNA\t";
    text += sum;
    text.push_back('\t');
    append_fixed3(text, rpm_sum[b]);
    text.push_back('\n');
  }
}

}  // namespace

void write_trf_sample_reports(const TrfSampleWriteArgs& a) {
  const uint32_t S = a.S;
  const uint64_t B = a.n_blocks;
  // ---- the tables against each other
  const uint64_t cells = (uint64_t)S * a.n_names;
  std::vector<int64_t> cell_block(cells, -1);
  uint64_t next_row = 0;
  for (uint64_t b = 0; b < B; ++b) {
    const int32_t* blk = a.blocks + b * 6;
    if (blk[0] < 0 || (uint32_t)blk[0] >= S || (b && blk[0] < blk[-6])) bad("blocks are not in sample order at block", b);
    if (blk[1] < 0 || (uint64_t)blk[1] >= a.n_entries) bad("representative entry out of range in block", b);
    const int32_t* en = a.entries + (uint64_t)blk[1] * kTrfSampleInts;
    if (!a.entry_names[blk[1]] || !a.templates[blk[1]] || !a.aa_types[blk[1]] || en[kTrfSampleTemplate] < 0 ||
        std::strlen(a.templates[blk[1]]) != (size_t)en[kTrfSampleTemplate])
      bad("name, template or amino acid missing for block", b);
    if (en[kTrfSampleName] < 0 || (uint32_t)en[kTrfSampleName] >= a.n_names) bad("name id out of range in block", b);
    if (blk[2] < 0 || blk[3] < 0 || (uint64_t)blk[2] != next_row || next_row + (uint64_t)blk[3] > a.n_rows)
      bad("printed rows are not consecutive at block", b);
    next_row += (uint64_t)blk[3];
    int64_t& slot = cell_block[(uint64_t)blk[0] * a.n_names + (uint32_t)en[kTrfSampleName]];
    if (slot >= 0) bad("two blocks of one sample and name: block", b);
    slot = (int64_t)b;
  }
  if (next_row != a.n_rows) bad("printed rows outside the blocks: rows", a.n_rows);
  // ---- RP100K sum and read count sum of every block, over the rows of the tsv
  std::vector<double> rpm_sum(B, 0.0);
  std::vector<uint64_t> read_sum(B, 0);
  for (uint64_t r = 0; r < a.k; ++r) {
    const int32_t* rec = a.rec + r * kTrfRecInts;
    if ((uint32_t)rec[kTrfRecKind] > kTrfDele) continue;
    const uint64_t read = (uint32_t)rec[kTrfRecRead];
    const int32_t entry = rec[kTrfRecEntry];
    if (read >= a.n || entry < 0 || (uint64_t)entry >= a.n_entries) bad("read or entry out of range in tsv row", r);
    const int32_t name = a.entries[(uint64_t)entry * kTrfSampleInts + kTrfSampleName];
    if (name < 0 || (uint32_t)name >= a.n_names) bad("name id out of range in tsv row", r);
    const uint32_t* q = a.quant + read * S;
    for (uint32_t s = 0; s < S; ++s) {
      if (!q[s]) continue;
      const int64_t b = cell_block[(uint64_t)s * a.n_names + (uint32_t)name];
      if (b < 0) bad("an item without block in tsv row", r);
      rpm_sum[b] += trf_rp100k(q[s], a.denom[s]);
      read_sum[b] += q[s];
    }
  }
  for (uint64_t b = 0; b < B; ++b)
    if (read_sum[b] != a.block_sums[b]) bad("read count sum does not match the items of block", b);

  // ---- the reports: runs of blocks of one sample
  const uint64_t run_rows = env_count("MIRGE_AMD_TRF_SAMPLE_BLOCK_ROWS", 1u << 14);  // (tests lower it)
  struct Run {
    uint64_t lo, hi;
    uint32_t s;
  };
  std::vector<Run> runs;
  for (uint64_t b = 0; b < B;) {
    const uint32_t s = (uint32_t)a.blocks[b * 6];
    uint64_t e = b, rows = 0;
    while (e < B && (uint32_t)a.blocks[e * 6] == s && (e == b || rows < run_rows)) rows += (uint32_t)a.blocks[e++ * 6 + 3] + 2;
    runs.push_back(Run{b, e, s});
    b = e;
  }
  std::vector<std::unique_ptr<File>> report;
  for (uint32_t s = 0; s < S; ++s) report.emplace_back(new File(a.paths[2 * s]));
  const unsigned n_threads = writer_threads(runs.size());
  std::vector<std::string> text(n_threads);
  in_batches(runs.size(), n_threads,
             [&](unsigned t, uint64_t r) {
               text[t].clear();
               format_blocks(a, rpm_sum, runs[r].lo, runs[r].hi, text[t]);
             },
             [&](uint64_t r0, unsigned live) {
               for (unsigned t = 0; t < live; ++t) report[runs[r0 + t].s]->write(text[t]);
             });
  for (auto& f : report) f->close();

  // ---- the summaries: keys in order of first appearance over the blocks, sums in print order
  uint64_t b = 0;
  for (uint32_t s = 0; s < S; ++s) {
    std::vector<std::string> keys;
    std::vector<uint64_t> count, unique;
    std::vector<double> rp;
    auto slot_of = [&](const std::string& key) {
      size_t i = std::find(keys.begin(), keys.end(), key) - keys.begin();
      if (i == keys.size()) {
        keys.push_back(key);
        count.push_back(0);
        unique.push_back(0);
        rp.push_back(0.0);
      }
      return i;
    };
    for (; b < B && (uint32_t)a.blocks[b * 6] == s; ++b) {
      const int32_t* blk = a.blocks + b * 6;
      const int32_t rep = blk[1];
      const int32_t* en = a.entries + (uint64_t)rep * kTrfSampleInts;
      std::string aa = a.aa_types[rep];
      if (en[kTrfSampleFlags] & 1) aa = "pre:" + aa;
      const bool trailer = aa.find("pre:") != std::string::npos;
      size_t slot[3];
      if (trailer) {
        slot[0] = slot[1] = slot[2] = slot_of(aa + " tRF-1");
      } else {
        slot[0] = slot_of(aa + " 5'");
        slot[1] = slot_of(aa + " 3'");
        slot[2] = slot_of(aa + " other");
      }
      const int64_t tlen = en[kTrfSampleTemplate];
      for (uint64_t at = (uint32_t)blk[2]; at < (uint64_t)(uint32_t)blk[2] + (uint32_t)blk[3]; ++at) {
        const Row r = row_of(a, at, s, rep);
        const size_t i = slot[r.start <= 2 ? 0 : tlen - (int64_t)r.start - (int64_t)r.len <= 2 ? 1 : 2];
        count[i] += r.count;
        rp[i] += trf_rp100k(r.count, a.denom[s]);
        unique[i] += 1;
      }
    }
    std::string out = "amino acid\tCounts\tRP100K\tUnique reads\n";
    for (size_t i = 0; i < keys.size(); ++i) {
      out += keys[i];
      out.push_back('\t');
      out += std::to_string((unsigned long long)count[i]);
      out.push_back('\t');
      append_fixed3(out, rp[i]);
      out.push_back('\t');
      out += std::to_string((unsigned long long)unique[i]);
      out.push_back('\n');
    }
    File f(a.paths[2 * s + 1]);
    f.write(out);
    f.close();
  }
}

}  // namespace mrg
