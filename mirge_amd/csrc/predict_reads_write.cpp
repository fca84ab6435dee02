// The FASTA files of convert2Fasta.py (unmapped_mirna[_raw].fa and the per-sample pairs) from the columnar arrays and the
// rows of mrg_predict_select / mrg_predict_sample_reads (host side, no GPU):
//   >mir<number>_<count>
//   <sequence>
// in list order.  The reads beyond 255 nt, which the packed arrays do not hold, are the last rows of unmapped.csv: they come
// as extra rows whose numbers continue after the packed ones.  The whole list is checked before the file is opened: an index
// that is no read, a number of 0 or numbers that do not increase write nothing (that holds for these list checks only: the
// file is open while the rows are formatted, so an I/O error met later can leave a truncated file).  Runs of rows are
// formatted by worker threads (host_write.hpp; MIRGE_AMD_PREDICT_BLOCK_ROWS = rows per run, lowered by tests) and written in
// order; the bytes depend on neither setting.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "host_write.hpp"
#include "predict_reads.hpp"

namespace mrg {

namespace {

inline uint64_t count_at(const void* counts, uint32_t count_bytes, uint64_t j) {
  return count_bytes == 8 ? ((const uint64_t*)counts)[j] : ((const uint32_t*)counts)[j];
}

// decimal digits of v into buf (at least 20 bytes); returns their number
inline uint32_t put_u64(char* buf, uint64_t v) {
  char tmp[20];
  uint32_t d = 0;
  do {
    tmp[d++] = (char)('0' + v % 10);
    v /= 10;
  } while (v);
  for (uint32_t i = 0; i < d; ++i) buf[i] = tmp[d - 1 - i];
  return d;
}

// ">mir<num>_<count>" without the '>' into buf (at least 48 bytes); returns the length
inline uint32_t put_name(char* buf, uint64_t num, uint64_t count) {
  std::memcpy(buf, "mir", 3);
  uint32_t at = 3 + put_u64(buf + 3, num);
  buf[at++] = '_';
  return at + put_u64(buf + at, count);
}

void format_rows(const PredictFastaArgs& a, uint64_t lo, uint64_t hi, std::string& text) {
  char head[48], seq[256];
  for (uint64_t j = lo; j < hi; ++j) {
    const uint64_t u = a.idx[j];
    const uint32_t L = a.lens[u];
    unpack_read(a.reads, a.nmask, a.stride, u, L, seq);
    text.push_back('>');
    text.append(head, put_name(head, a.num[j], count_at(a.counts, a.count_bytes, j)));
    text.push_back('\n');
    text.append(seq, L);
    text.push_back('\n');
  }
}

}  // namespace

uint64_t write_predict_fasta(const PredictFastaArgs& a) {
  uint64_t last = 0;
  for (uint64_t j = 0; j < a.k; ++j) {
    const uint64_t u = a.idx[j];
    if (u >= a.n) throw std::invalid_argument("index[" + std::to_string(j) + "] = " + std::to_string(u) + " is no read of " + std::to_string(a.n));
    if (a.num[j] == 0) throw std::invalid_argument("row " + std::to_string(j) + " has number 0");
    if (a.num[j] <= last) throw std::invalid_argument("the numbers of rows " + std::to_string(j - 1) + " and " + std::to_string(j) + " do not increase");
    if (j && a.idx[j - 1] >= u) throw std::invalid_argument("the indices of rows " + std::to_string(j - 1) + " and " + std::to_string(j) + " do not increase");
    if (a.lens[u] > 32u * a.W) throw std::invalid_argument("read " + std::to_string(u) + " does not fit its words");
    last = a.num[j];
  }
  for (uint64_t e = 0; e < a.n_extra; ++e) {
    if (!a.extra_seqs[e]) throw std::invalid_argument("extra row " + std::to_string(e) + ": null sequence");
    if (a.extra_nums[e] == 0) throw std::invalid_argument("extra row " + std::to_string(e) + " has number 0");
    if (a.extra_nums[e] <= last) throw std::invalid_argument("the number of extra row " + std::to_string(e) + " does not increase");
    last = a.extra_nums[e];
  }
  File out(a.path);
  const uint64_t run = env_count("MIRGE_AMD_PREDICT_BLOCK_ROWS", 65536);  // rows per worker and round
  const uint64_t n_runs = (a.k + run - 1) / run;
  const unsigned n_threads = writer_threads(n_runs);
  std::vector<std::string> text(n_threads);
  in_batches(n_runs, n_threads,
             [&](unsigned t, uint64_t r) {
               text[t].clear();
               format_rows(a, r * run, std::min(a.k, (r + 1) * run), text[t]);
             },
             [&](uint64_t, unsigned live) {
               for (unsigned t = 0; t < live; ++t) out.write(text[t]);
             });
  std::string tail;
  char head[48];
  for (uint64_t e = 0; e < a.n_extra; ++e) {
    tail.push_back('>');
    tail.append(head, put_name(head, a.extra_nums[e], a.extra_counts[e]));
    tail.push_back('\n');
    tail += a.extra_seqs[e];
    tail.push_back('\n');
  }
  out.write(tail);
  out.close();
  return a.k + a.n_extra;
}

uint64_t predict_read_names(const uint32_t* num, const void* counts, uint32_t count_bytes, uint64_t k, char* blob, uint64_t cap,
                            uint64_t* offsets) {
  char name[48];
  uint64_t at = 0;
  for (uint64_t j = 0; j < k; ++j) {
    const uint32_t len = put_name(name, num[j], count_at(counts, count_bytes, j));
    offsets[j] = at;
    if (blob && at + len <= cap) std::memcpy(blob + at, name, len);
    at += len;
  }
  offsets[k] = at;
  return at;
}

}  // namespace mrg
