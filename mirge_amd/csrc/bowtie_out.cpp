// bowtie 1.1.2's text output for the bowtie front end (mirge_amd/bowtie.py; host side, no GPU).
//
// miRge2.0 reads its aligner's answers back as text: SAM (`-S`: processSam.py, cluster_basedon_location.py,
// parseAlignment* of runAnnotationPipeline.py) or bowtie's default format (the two -ai genome runs of
// writeDataToCSV.py:1263 / :1488).  A predict-mode genome run prints 10^6..10^7 lines, so they are formatted here from
// the columnar alignment arrays, never line by line in Python: worker threads format blocks of reads and hand them on
// to the output in block order (write_read_table's scheme, tables.cpp, with ordered write(2) so that the target may be
// a pipe).  What is formatted is documented at mrg_write_bowtie (include/mirge_amd.h).
//
// Predict mode's own route (mirge_amd/predict.py) ends here too: the coordinate-sorted SAM file (the same lines in the
// order of the device's sort) and the cluster table of cluster_basedon_location.py, from the cluster arrays of
// predict_cluster.hip (mrg_write_sorted_sam, mrg_write_clusters).
#include <unistd.h>
#include <fcntl.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "fm_index.hpp"
#include "host_write.hpp"
#include "tables.hpp"

namespace mrg {

namespace {

// Entry e of the concatenated parts -> its text, through the N-free segments of its part.
struct Entries {
  struct Part {
    const FmIndex* ix;
    uint64_t first_entry;
    std::vector<uint32_t> first_seg;  // segments of local entry e: [first_seg[e], first_seg[e + 1])
  };
  std::vector<Part> parts;
  std::vector<uint64_t> starts;  // global entry number of each part's entry 0, then the total

  explicit Entries(const std::vector<const FmIndex*>& ix) {
    uint64_t e0 = 0;
    for (const FmIndex* p : ix) {
      Part q{p, e0, std::vector<uint32_t>(p->names.size() + 1, 0u)};
      const size_t n_seg = p->seg_ref.size();
      for (size_t s = 0; s < n_seg; ++s) {
        if (s && p->seg_ref[s] < p->seg_ref[s - 1]) throw std::runtime_error("index segments out of entry order");
        if (p->seg_ref[s] >= p->names.size()) throw std::runtime_error("index segment of an unknown entry");
        ++q.first_seg[p->seg_ref[s] + 1];
      }
      for (size_t e = 0; e < p->names.size(); ++e) q.first_seg[e + 1] += q.first_seg[e];
      starts.push_back(e0);
      e0 += p->names.size();
      parts.push_back(std::move(q));
    }
    starts.push_back(e0);
  }

  const Part& part_of(uint64_t e, uint32_t& local) const {
    const size_t k = (size_t)(std::upper_bound(starts.begin(), starts.end() - 1, e) - starts.begin()) - 1;
    if (e >= starts.back()) throw std::runtime_error("alignment entry out of range");
    local = (uint32_t)(e - starts[k]);
    return parts[k];
  }

  // reference bases [off, off + len) of entry e as ACGT
  void bases(uint64_t e, uint32_t off, uint32_t len, std::string& out) const {
    uint32_t le;
    const Part& q = part_of(e, le);
    const FmIndex& ix = *q.ix;
    const uint32_t s0 = q.first_seg[le], s1 = q.first_seg[le + 1];
    // the segment holding `off`: the last one that starts at or before it
    uint32_t lo = s0, hi = s1;
    while (hi - lo > 1) {
      const uint32_t mid = (lo + hi) / 2;
      if (ix.seg_off[mid] <= off) lo = mid;
      else hi = mid;
    }
    if (lo >= s1 || ix.seg_off[lo] > off || off + len - ix.seg_off[lo] > ix.seg_start[lo + 1] - ix.seg_start[lo])
      throw std::runtime_error("alignment outside the N-free part of its entry");
    const uint64_t p0 = (uint64_t)ix.seg_start[lo] + (off - ix.seg_off[lo]);
    out.resize(len);
    for (uint32_t i = 0; i < len; ++i) {
      const uint64_t p = p0 + i;
      out[i] = base_char(ix.text[p >> 4] >> ((p & 15) * 2));
    }
  }

  const std::string& name(uint64_t e) const {
    uint32_t le;
    return part_of(e, le).ix->names[le];
  }
};

char complement(char c) {
  switch (c) {
    case 'A': return 'T';
    case 'C': return 'G';
    case 'G': return 'C';
    case 'T': return 'A';
    default: return 'N';
  }
}

void put_u64(std::string& out, uint64_t v) {
  char buf[24];
  int k = 0;
  do {
    buf[k++] = (char)('0' + v % 10);
    v /= 10;
  } while (v);
  while (k) out += buf[--k];
}

struct BowtieArgs {
  bool sam;
  const Entries* entries;
  const char* names;
  const uint64_t* names_off;
  const char* seqs;
  const uint64_t* seqs_off;
  const uint64_t* offsets;
  const int32_t* entry;
  const int32_t* offset;
  const uint8_t* strand;
  const uint8_t* mm;
  const uint8_t* suppressed;
  int32_t m;
};

struct BlockCounts {
  uint64_t aligned = 0, suppressed = 0, lines = 0;
};

// scratch strings of a formatting thread
struct LineScratch {
  std::string q, ref, qual;
};

// the FLAG 4 line of read r (SAM only): unaligned, or suppressed by -m
void format_unaligned(const BowtieArgs& a, uint64_t r, std::string& out, LineScratch& t) {
  const uint32_t L = (uint32_t)(a.seqs_off[r + 1] - a.seqs_off[r]);
  t.qual.assign(L, 'I');
  out.append(a.names + a.names_off[r], (size_t)(a.names_off[r + 1] - a.names_off[r]));
  out += "\t4\t*\t0\t0\t*\t*\t0\t0\t";
  out.append(a.seqs + a.seqs_off[r], L);
  out += '\t';
  out += t.qual;
  out += "\tXM:i:";
  put_u64(out, (a.suppressed && a.suppressed[r]) ? (uint64_t)a.m + 1 : 0u);
  out += '\n';
}

// a SAM line's fields after the read name, from the tab before FLAG to the last of NM:i: (no line end): q = the sequence as
// printed, ref = the reference bases under it
void put_sam_fields(std::string& out, bool minus, const std::string& rname, uint32_t off, const std::string& q, const std::string& qual,
                    const std::string& ref, uint32_t mm) {
  const uint32_t L = (uint32_t)q.size();
  out += minus ? "\t16\t" : "\t0\t";
  out += rname;
  out += '\t';
  put_u64(out, (uint64_t)off + 1);
  out += "\t255\t";
  put_u64(out, L);
  out += "M\t*\t0\t0\t";
  out += q;
  out += '\t';
  out += qual;
  out += "\tXA:i:";
  put_u64(out, mm);
  out += "\tMD:Z:";
  uint32_t run = 0;
  for (uint32_t i = 0; i < L; ++i) {
    if (q[i] == ref[i]) {
      ++run;
      continue;
    }
    put_u64(out, run);
    out += ref[i];
    run = 0;
  }
  put_u64(out, run);
  out += "\tNM:i:";
  put_u64(out, mm);
}

// the line of alignment k (entry / offset / strand / mm [k]) of read r
void format_aligned(const BowtieArgs& a, uint64_t r, uint64_t k, std::string& out, LineScratch& t) {
  const char* name = a.names + a.names_off[r];
  const size_t name_len = (size_t)(a.names_off[r + 1] - a.names_off[r]);
  const char* seq = a.seqs + a.seqs_off[r];
  const uint32_t L = (uint32_t)(a.seqs_off[r + 1] - a.seqs_off[r]);
  std::string& q = t.q;
  std::string& ref = t.ref;
  t.qual.assign(L, 'I');
  const bool minus = a.strand[k] != 0;
  q.assign(seq, L);
  if (minus) {
    std::reverse(q.begin(), q.end());
    for (char& ch : q) ch = complement(ch);
  }
  const uint64_t e = (uint64_t)(uint32_t)a.entry[k];
  const uint32_t off = (uint32_t)a.offset[k];
  a.entries->bases(e, off, L, ref);
  const std::string& rname = a.entries->name(e);
  out.append(name, name_len);
  if (a.sam) {
    put_sam_fields(out, minus, rname, off, q, t.qual, ref, a.mm[k]);
  } else {
    out += minus ? "\t-\t" : "\t+\t";
    out += rname;
    out += '\t';
    put_u64(out, off);
    out += '\t';
    out += q;
    out += '\t';
    out += t.qual;
    out += "\t0\t";
    bool first = true;
    for (uint32_t i = 0; i < L; ++i) {
      if (q[i] == ref[i]) continue;
      if (!first) out += ',';
      first = false;
      put_u64(out, i);
      out += ':';
      out += ref[i];
      out += '>';
      out += q[i];
    }
  }
  out += '\n';
}

void format_reads(const BowtieArgs& a, uint64_t lo, uint64_t hi, std::string& out, BlockCounts& c) {
  LineScratch t;
  for (uint64_t r = lo; r < hi; ++r) {
    const uint64_t k0 = a.offsets[r], k1 = a.offsets[r + 1];
    if ((a.suppressed && a.suppressed[r]) || k0 == k1) {
      if (a.suppressed && a.suppressed[r]) ++c.suppressed;
      if (a.sam) format_unaligned(a, r, out, t);
      continue;
    }
    ++c.aligned;
    for (uint64_t k = k0; k < k1; ++k) {
      format_aligned(a, r, k, out, t);
      ++c.lines;
    }
  }
}

// An output file (path null = standard output) written with ordered write(2), so that the target may be a pipe.
struct OutFile {
  int fd;
  const char* path;
  explicit OutFile(const char* p) : fd(p ? ::open(p, O_WRONLY | O_CREAT | O_TRUNC, 0644) : 1), path(p) {
    if (fd < 0) throw std::runtime_error(std::string("cannot open ") + p);
  }
  ~OutFile() {
    if (path && fd >= 0) ::close(fd);
  }
  void write_all(const char* data, size_t len) {
    while (len) {
      const ssize_t w = ::write(fd, data, len);
      if (w < 0) {
        if (errno == EINTR) continue;
        throw std::runtime_error(std::string("write to ") + (path ? path : "standard output") + " failed");
      }
      data += w;
      len -= (size_t)w;
    }
  }
  void close() {
    if (!path) return;
    const int f = fd;
    fd = -1;
    if (::close(f) != 0) throw std::runtime_error(std::string("cannot close ") + path);
  }
};

// format(b, texts) for every block b < n_blocks on worker threads; texts[f] goes to files[f], every file in block order.
// turn = the block whose texts go out next: a worker formats its block, waits for its turn, writes, passes the turn on
template <size_t N, class Format>
void write_file_blocks_in_order(OutFile* const (&files)[N], uint64_t n_blocks, Format format) {
  const unsigned n_threads = writer_threads(n_blocks);
  std::atomic<uint64_t> next{0}, turn{0};
  std::atomic<bool> stop{false};
  std::vector<std::exception_ptr> failed(n_threads);
  auto worker = [&](unsigned t) {
    std::string texts[N];
    try {
      for (;;) {
        const uint64_t b = next.fetch_add(1, std::memory_order_relaxed);
        if (b >= n_blocks || stop.load(std::memory_order_relaxed)) break;
        for (std::string& text : texts) text.clear();
        format(b, texts);
        while (turn.load(std::memory_order_acquire) != b) {
          if (stop.load(std::memory_order_relaxed)) return;
          std::this_thread::yield();
        }
        for (size_t f = 0; f < N; ++f) files[f]->write_all(texts[f].data(), texts[f].size());
        turn.store(b + 1, std::memory_order_release);
      }
    } catch (...) {
      failed[t] = std::current_exception();
      stop.store(true, std::memory_order_relaxed);
    }
  };
  if (n_threads == 1) {
    worker(0);
  } else {
    std::vector<std::thread> pool;
    struct Joiner {
      std::vector<std::thread>& p;
      ~Joiner() {
        for (auto& th : p)
          if (th.joinable()) th.join();
      }
    };
    Joiner joiner{pool};
    try {
      for (unsigned t = 0; t < n_threads; ++t) pool.emplace_back(worker, t);
    } catch (...) {
      stop.store(true, std::memory_order_relaxed);
      throw;
    }
  }
  for (unsigned t = 0; t < n_threads; ++t)
    if (failed[t]) std::rethrow_exception(failed[t]);
}

// one file: format(b, text)
template <class Format>
void write_blocks_in_order(OutFile& file, uint64_t n_blocks, Format format) {
  OutFile* const files[1] = {&file};
  write_file_blocks_in_order(files, n_blocks, [&](uint64_t b, std::string (&texts)[1]) { format(b, texts[0]); });
}

void sam_sq_lines(const std::vector<const FmIndex*>& parts, std::string& h) {
  for (const FmIndex* ix : parts)
    for (size_t e = 0; e < ix->names.size(); ++e) {
      h += "@SQ\tSN:";
      h += ix->names[e];
      h += "\tLN:";
      put_u64(h, ix->ref_len[e]);
      h += '\n';
    }
}

}  // namespace

void write_bowtie(const char* path, bool sam, const char* cmdline, const std::vector<const FmIndex*>& parts, uint64_t n_reads,
                  const char* names, const uint64_t* names_off, const char* seqs, const uint64_t* seqs_off, const uint64_t* offsets,
                  const int32_t* entry, const int32_t* offset, const uint8_t* strand, const uint8_t* mm, const uint8_t* suppressed,
                  int32_t m, uint64_t* summary) {
  const Entries entries(parts);
  OutFile file(path);
  if (sam) {
    std::string h = "@HD\tVN:1.0\tSO:unsorted\n";
    sam_sq_lines(parts, h);
    h += "@PG\tID:Bowtie\tVN:1.1.2\tCL:\"";
    h += cmdline ? cmdline : "";
    h += "\"\n";
    file.write_all(h.data(), h.size());
  }
  const BowtieArgs a{sam, &entries, names, names_off, seqs, seqs_off, offsets, entry, offset, strand, mm, suppressed, m};
  constexpr uint64_t kBlockReads = 1u << 16;
  const uint64_t n_blocks = (n_reads + kBlockReads - 1) / kBlockReads;
  std::atomic<uint64_t> aligned{0}, supp{0}, lines{0};
  write_blocks_in_order(file, n_blocks, [&](uint64_t b, std::string& text) {
    BlockCounts c;
    format_reads(a, b * kBlockReads, std::min(n_reads, (b + 1) * kBlockReads), text, c);
    aligned.fetch_add(c.aligned, std::memory_order_relaxed);
    supp.fetch_add(c.suppressed, std::memory_order_relaxed);
    lines.fetch_add(c.lines, std::memory_order_relaxed);
  });
  file.close();
  summary[0] = n_reads;
  summary[1] = aligned.load();
  summary[2] = supp.load();
  summary[3] = lines.load();
}

void write_sorted_sam(const char* path, const std::vector<const FmIndex*>& parts, uint64_t n_reads, const char* names,
                      const uint64_t* names_off, const char* seqs, const uint64_t* seqs_off, uint64_t n_rows, const uint32_t* row_read,
                      const int32_t* entry, const int32_t* offset, const uint8_t* strand, const uint8_t* mm, const uint8_t* suppressed,
                      int32_t m, uint64_t* summary) {
  const Entries entries(parts);
  OutFile file(path);
  std::string h = "@HD\tVN:1.0\tSO:coordinate\n";
  sam_sq_lines(parts, h);
  file.write_all(h.data(), h.size());
  const BowtieArgs a{true, &entries, names, names_off, seqs, seqs_off, nullptr, entry, offset, strand, mm, suppressed, m};
  std::vector<uint8_t> has_row(n_reads, 0);
  for (uint64_t k = 0; k < n_rows; ++k) {
    if (row_read[k] >= n_reads) throw std::runtime_error("alignment row of an unknown read");
    has_row[row_read[k]] = 1;
  }
  // the aligned rows in the order given, then the reads without one in input order
  constexpr uint64_t kBlock = 1u << 16;
  const uint64_t row_blocks = (n_rows + kBlock - 1) / kBlock, read_blocks = (n_reads + kBlock - 1) / kBlock;
  std::atomic<uint64_t> supp{0}, unaligned{0};
  write_blocks_in_order(file, row_blocks + read_blocks, [&](uint64_t b, std::string& text) {
    LineScratch t;
    if (b < row_blocks) {
      for (uint64_t k = b * kBlock; k < std::min(n_rows, (b + 1) * kBlock); ++k) format_aligned(a, row_read[k], k, text, t);
      return;
    }
    b -= row_blocks;
    uint64_t n_supp = 0, n_un = 0;
    for (uint64_t r = b * kBlock; r < std::min(n_reads, (b + 1) * kBlock); ++r) {
      if (has_row[r]) continue;
      ++n_un;
      if (suppressed && suppressed[r]) ++n_supp;
      format_unaligned(a, r, text, t);
    }
    supp.fetch_add(n_supp, std::memory_order_relaxed);
    unaligned.fetch_add(n_un, std::memory_order_relaxed);
  });
  file.close();
  summary[0] = n_reads;
  summary[1] = n_reads - unaligned.load();
  summary[2] = supp.load();
  summary[3] = n_rows;
}

void write_clusters(const char* path, const char* sample, const std::vector<const FmIndex*>& parts, uint64_t n_clusters,
                    const uint32_t* entry, const uint8_t* strand, const uint32_t* start, const uint32_t* end, const uint64_t* seq_off,
                    const char* seq, const uint64_t* count_sum, const uint32_t* member_off, const uint32_t* members, uint64_t n_reads,
                    const char* names, const uint64_t* names_off, uint64_t* rows) {
  const Entries entries(parts);
  OutFile file(path);
  const std::string h = "miRClusterID\tChr\tStrand\tStart\tEnd\tSequence\tSequenceLenght\tCoutOfReads\tCountOfMembers\tMembers\n";
  file.write_all(h.data(), h.size());
  constexpr uint64_t kBlock = 1u << 13;
  write_blocks_in_order(file, (n_clusters + kBlock - 1) / kBlock, [&](uint64_t b, std::string& text) {
    for (uint64_t c = b * kBlock; c < std::min(n_clusters, (b + 1) * kBlock); ++c) {
      const uint64_t len = seq_off[c + 1] - seq_off[c];
      text += sample ? sample : "";
      text += ":miRCluster_";
      put_u64(text, c + 1);
      text += '_';
      put_u64(text, len);
      text += '\t';
      text += entries.name(entry[c]);
      text += strand[c] ? "\t-\t" : "\t+\t";
      put_u64(text, start[c]);
      text += '\t';
      put_u64(text, end[c]);
      text += '\t';
      text.append(seq + seq_off[c], (size_t)len);
      text += '\t';
      put_u64(text, len);
      text += '\t';
      put_u64(text, count_sum[c]);
      text += '\t';
      put_u64(text, member_off[c + 1] - member_off[c]);
      text += '\t';
      for (uint32_t k = member_off[c]; k < member_off[c + 1]; ++k) {
        const uint32_t r = members[k];
        if (r >= n_reads) throw std::runtime_error("cluster member of an unknown read");
        if (k != member_off[c]) text += ',';
        text.append(names + names_off[r], (size_t)(names_off[r + 1] - names_off[r]));
      }
      text += '\n';
    }
  });
  file.close();
  *rows = n_clusters;
}

// preTrimClusteredSeq.py's table and generate_Seq.py's two FASTA files from the cluster arrays and the arrays of mrg_predict_trim
void write_trimmed_clusters(const TrimmedClustersArgs& a, uint64_t* rows, uint64_t* kept) {
  const Entries entries(*a.parts);
  for (uint64_t c = 0; c < a.n_clusters; ++c) {
    if (a.seq_off[c + 1] < a.seq_off[c]) throw std::invalid_argument("cluster sequence offsets out of order");
    if (a.rep[c] >= 0 && (uint64_t)a.rep[c] >= a.n_elements) throw std::invalid_argument("repeat element out of range");
    if (a.rep[c] >= 0 && a.rep_name_id[a.rep[c]] >= a.n_rep_names) throw std::invalid_argument("repeat name out of range");
  }
  OutFile tsv(a.tsv_path), fa(a.fa_path), orig_fa(a.orig_fa_path);
  const std::string h =
      "miRClusterID\tOriginalSeq\tFlag\trepetitiveElementName\tChr\tStrand\tStart\tEnd\tSequence\tSequenceLenght\tCoutOfReads\t"
      "CountOfMembers\tMembers\n";
  tsv.write_all(h.data(), h.size());
  constexpr uint64_t kBlock = 1u << 13;
  std::atomic<uint64_t> n_kept{0};
  OutFile* const files[3] = {&tsv, &fa, &orig_fa};
  write_file_blocks_in_order(files, (a.n_clusters + kBlock - 1) / kBlock, [&](uint64_t b, std::string (&texts)[3]) {
    std::string id, where;
    uint64_t k = 0;
    for (uint64_t c = b * kBlock; c < std::min(a.n_clusters, (b + 1) * kBlock); ++c) {
      const uint64_t len = a.seq_off[c + 1] - a.seq_off[c];
      id = a.sample;
      id += ":miRCluster_";
      put_u64(id, c + 1);
      id += '_';
      put_u64(id, len);
      const std::string& chr = entries.name(a.entry[c]);
      std::string& text = texts[0];
      text += id;
      text += '\t';
      text.append(a.orig + a.seq_off[c], (size_t)len);
      text += a.flag[c] ? "\t1\t" : "\t0\t";
      if (a.rep[c] < 0) {
        text += '*';
      } else {
        const uint32_t nm = a.rep_name_id[a.rep[c]];
        text.append(a.rep_names + a.rep_names_off[nm], (size_t)(a.rep_names_off[nm + 1] - a.rep_names_off[nm]));
      }
      text += '\t';
      text += chr;
      text += a.strand[c] ? "\t-\t" : "\t+\t";
      put_u64(text, a.start[c]);
      text += '\t';
      put_u64(text, a.end[c]);
      text += '\t';
      text.append(a.seq + a.seq_off[c], (size_t)len);
      text += '\t';
      put_u64(text, len);
      text += '\t';
      put_u64(text, a.count_sum[c]);
      text += '\t';
      put_u64(text, a.member_off[c + 1] - a.member_off[c]);
      text += '\t';
      for (uint32_t m = a.member_off[c]; m < a.member_off[c + 1]; ++m) {
        const uint32_t r = a.members[m];
        if (r >= a.n_reads) throw std::runtime_error("cluster member of an unknown read");
        if (m != a.member_off[c]) text += ',';
        text.append(a.names + a.names_off[r], (size_t)(a.names_off[r + 1] - a.names_off[r]));
      }
      text += '\n';
      if (!a.flag[c]) continue;
      ++k;
      where = ">";
      where += id;
      where += ':';
      where += chr;
      where += ':';
      put_u64(where, a.start[c]);
      where += '_';
      put_u64(where, a.end[c]);
      where += a.strand[c] ? "-\n" : "+\n";
      texts[1] += where;
      texts[1].append(a.seq + a.seq_off[c], (size_t)len);
      texts[1] += '\n';
      texts[2] += where;
      texts[2].append(a.orig + a.seq_off[c], (size_t)len);
      texts[2] += '\n';
    }
    n_kept.fetch_add(k, std::memory_order_relaxed);
  });
  tsv.close();
  fa.close();
  orig_fa.close();
  *rows = a.n_clusters;
  *kept = n_kept.load();
}

// `<sample>_vs_representative_seq_modified_selected_sorted.tsv` (decorateSam + parse_refine_sam + `sort -k6,6 -k1,1` of the
// reference) from the rows of mrg_predict_remap_rows: per row the read's name, count and whole sequence, the cluster's
// OriginalSeq and the SAM fields of the alignment (put_sam_fields: forward strand, the sequence a pass-2 row aligned with is
// the read cut by trim5 / trim3).  The rows come ordered by (cluster name, read name); the rows of one read on one cluster are
// put into the byte order of their lines here, which is `sort`'s last resort.
uint64_t write_remapped_rows(const RemappedRowsArgs& a) {
  if (a.n_clusters && (!a.clusters || a.clusters->names.size() != a.n_clusters))
    throw std::invalid_argument("the cluster library does not hold the clusters given");
  for (uint64_t c = 0; c < a.n_clusters; ++c)
    if (a.kept_seq_off[c + 1] < a.kept_seq_off[c]) throw std::invalid_argument("cluster sequence offsets out of order");
  for (uint64_t k = 0; k < a.n_rows; ++k) {
    const uint64_t r = a.row_read[k], c = a.row_cluster[k];
    if (r >= a.n_reads) throw std::invalid_argument("row " + std::to_string(k) + " of an unknown read");
    if (c >= a.n_clusters) throw std::invalid_argument("row " + std::to_string(k) + " of an unknown cluster");
    if (a.row_pass[k] > 1) throw std::invalid_argument("row " + std::to_string(k) + " of an unknown pass");
    const uint32_t full = a.lens[r], cut = a.row_pass[k] ? a.trim5 + a.trim3 : 0u;
    if (full > 32u * a.W) throw std::invalid_argument("read " + std::to_string(r) + " does not fit its words");
    if (full <= cut) throw std::invalid_argument("row " + std::to_string(k) + " aligns an empty read");
    if ((uint64_t)a.row_offset[k] + (full - cut) > a.kept_seq_off[c + 1] - a.kept_seq_off[c])
      throw std::invalid_argument("row " + std::to_string(k) + " runs past the end of its cluster");
  }
  OutFile file(a.path);
  const uint64_t block = env_count("MIRGE_AMD_PREDICT_BLOCK_ROWS", 1u << 12);  // (tests lower it)
  // a block starts at the first row at or after its nominal start that continues no (cluster, read) run
  auto run_start = [&](uint64_t k) {
    k = std::min(k, a.n_rows);
    while (k && k < a.n_rows && a.row_cluster[k] == a.row_cluster[k - 1] && a.row_read[k] == a.row_read[k - 1]) ++k;
    return k;
  };
  auto format_row = [&](uint64_t k, std::string& out, LineScratch& t, std::string& whole) {
    const uint64_t r = a.row_read[k], c = a.row_cluster[k];
    const uint32_t full = a.lens[r];
    whole.clear();
    unpack_read(a.reads, a.nmask, a.stride, r, full, whole);
    const uint32_t t5 = a.row_pass[k] ? a.trim5 : 0u, t3 = a.row_pass[k] ? a.trim3 : 0u;
    const uint32_t L = full - t5 - t3;
    const char* orig = a.kept_orig + a.kept_seq_off[c];
    t.q.assign(whole, t5, L);
    t.qual.assign(L, 'I');
    t.ref.assign(orig + a.row_offset[k], L);
    out += "mir";
    put_u64(out, a.numbers[r]);
    out += '_';
    put_u64(out, a.counts[r]);
    out += '\t';
    put_u64(out, a.counts[r]);
    out += '\t';
    out += whole;
    out += '\t';
    out.append(orig, (size_t)(a.kept_seq_off[c + 1] - a.kept_seq_off[c]));
    put_sam_fields(out, false, a.clusters->names[c], a.row_offset[k], t.q, t.qual, t.ref, a.row_mm[k]);
    out += '\n';
  };
  write_blocks_in_order(file, (a.n_rows + block - 1) / block, [&](uint64_t b, std::string& text) {
    LineScratch t;
    std::string whole;
    std::vector<std::string> lines;
    const uint64_t lo = run_start(b * block), hi = run_start((b + 1) * block);
    for (uint64_t k = lo; k < hi;) {
      uint64_t e = k + 1;
      while (e < hi && a.row_cluster[e] == a.row_cluster[k] && a.row_read[e] == a.row_read[k]) ++e;
      if (e - k == 1) {
        format_row(k, text, t, whole);
      } else {
        lines.assign(e - k, std::string());
        for (uint64_t j = k; j < e; ++j) format_row(j, lines[j - k], t, whole);
        std::sort(lines.begin(), lines.end());
        for (const std::string& s : lines) text += s;
      }
      k = e;
    }
  });
  file.close();
  return a.n_rows;
}

// the integer between the first and the second '_' of every read name (`mir<k>_<count>`, reference convert2Fasta.py:131)
int64_t read_counts_from_names(uint64_t n_reads, const char* names, const uint64_t* names_off, uint32_t* counts) {
  for (uint64_t r = 0; r < n_reads; ++r) {
    const char* p = names + names_off[r];
    const char* e = names + names_off[r + 1];
    while (p < e && *p != '_') ++p;
    if (p == e || p + 1 == e || p[1] < '0' || p[1] > '9') return (int64_t)r;
    uint64_t v = 0;
    for (++p; p < e && *p != '_'; ++p) {
      if (*p < '0' || *p > '9') return (int64_t)r;
      v = v * 10 + (uint64_t)(*p - '0');
      if (v > 0xffffffffull) return (int64_t)r;
    }
    counts[r] = (uint32_t)v;
  }
  return -1;
}

}  // namespace mrg
