// `<table>_features_precusor.fa` of predict mode (reference utils/get_precursors.py; the rule:
// tests/predict_precursors_model.py) from host arrays, no GPU: the records and bases of mrg_predict_precursors and
// mrg_predict_precursor_bases.  Record 2 w is `>name:precusor_1`, record 2 w + 1 `>name:precusor_2` of the w-th written
// group; the name is the cluster library's entry name, as in `_features.tsv`.  The reference skips a name it has seen: a
// group listed twice is refused here instead (every cluster has one group and its own name).
// Everything is checked before the file is opened.  Blocks of records are formatted by worker threads and written in order:
// the bytes depend on neither the thread count nor the block length.
#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "fm_index.hpp"
#include "host_write.hpp"
#include "predict_precursors.hpp"

namespace mrg {

namespace {

[[noreturn]] void bad_record(uint64_t r, const std::string& what) { throw std::invalid_argument("record " + std::to_string(r) + ": " + what); }

void check_all(const PrecWriteArgs& a) {
  std::vector<uint32_t> entry_len;
  for (const FmIndex* p : *a.parts) entry_len.insert(entry_len.end(), p->ref_len.begin(), p->ref_len.end());
  if (a.n_clusters && (!a.clusters || a.clusters->names.size() != a.n_clusters))
    throw std::invalid_argument("the cluster library does not hold the clusters given");
  if (a.n_rec & 1) throw std::invalid_argument("an odd number of records: every written group has two");
  for (uint64_t c = 0; c < a.n_clusters; ++c)
    if (a.cl_entry[c] >= entry_len.size()) throw std::invalid_argument("cluster " + std::to_string(c) + " on an unknown entry");
  for (uint64_t g = 0; g < a.n_groups; ++g)
    if (a.group_cluster[g] >= a.n_clusters) throw std::invalid_argument("group " + std::to_string(g) + " of an unknown cluster");
  if (a.rec_off[0] != 0 || a.rec_off[a.n_rec] != a.seq_len) throw std::invalid_argument("record offsets do not run from 0 to the sequence length");
  std::vector<uint8_t> seen(a.n_groups, 0);
  for (uint64_t r = 0; r < a.n_rec; ++r) {
    const uint64_t g = a.rec_group[r];
    if (g >= a.n_groups) bad_record(r, "of an unknown group");
    if (r & 1) {
      if (g != a.rec_group[r - 1]) bad_record(r, "its group is not the record's before it");
    } else {
      if (seen[g]) bad_record(r, "its group is listed twice");
      seen[g] = 1;
    }
    if (a.rec_off[r] > a.rec_off[r + 1] || a.rec_off[r + 1] > a.seq_len) bad_record(r, "offsets do not ascend inside the sequence bytes");
    if (a.rec_lo[r] > a.rec_hi[r] || a.rec_off[r + 1] - a.rec_off[r] != (uint64_t)(a.rec_hi[r] - a.rec_lo[r]))
      bad_record(r, "its bytes are not its window's");
    if (a.rec_hi[r] > entry_len[a.cl_entry[a.group_cluster[g]]]) bad_record(r, "its window leaves its chromosome");
  }
}

void format_record(const PrecWriteArgs& a, uint64_t r, std::string& out) {
  out.push_back('>');
  out += a.clusters->names[a.group_cluster[a.rec_group[r]]];
  out += (r & 1) ? ":precusor_2\n" : ":precusor_1\n";
  out.append(a.seq + a.rec_off[r], (size_t)(a.rec_off[r + 1] - a.rec_off[r]));
  out.push_back('\n');
}

}  // namespace

void write_precursors(const PrecWriteArgs& a, uint64_t* written) {
  check_all(a);
  File fa(a.path);
  const uint64_t run = env_count("MIRGE_AMD_PRECURSOR_BLOCK_RECORDS", 4096);  // records per worker and round (tests lower it)
  const uint64_t n_runs = (a.n_rec + run - 1) / run;
  const unsigned n_threads = writer_threads(n_runs);
  std::vector<std::string> text(n_threads);
  uint64_t bytes = 0;
  in_batches(n_runs, n_threads,
             [&](unsigned t, uint64_t b) {
               text[t].clear();
               for (uint64_t r = b * run; r < std::min(a.n_rec, (b + 1) * run); ++r) format_record(a, r, text[t]);
             },
             [&](uint64_t, unsigned live) {
               for (unsigned t = 0; t < live; ++t) {
                 fa.write(text[t]);
                 bytes += text[t].size();
               }
             });
  fa.close();
  if (written) {
    written[0] = a.n_rec;
    written[1] = bytes;
  }
}

}  // namespace mrg
