// bowtie 1.1.2's text output for the bowtie front end (mirge_amd/bowtie.py; host side, no GPU).
//
// miRge2.0 reads its aligner's answers back as text: SAM (`-S`: processSam.py, cluster_basedon_location.py,
// parseAlignment* of runAnnotationPipeline.py) or bowtie's default format (the two -ai genome runs of
// writeDataToCSV.py:1263 / :1488).  A predict-mode genome run prints 10^6..10^7 lines, so they are formatted here from
// the columnar alignment arrays, never line by line in Python: worker threads format blocks of reads and hand them on
// to the output in block order (write_read_table's scheme, tables.cpp, with ordered write(2) so that the target may be
// a pipe).  What is formatted is documented at mrg_write_bowtie (include/mirge_amd.h).
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
    static const char kBase[4] = {'A', 'C', 'G', 'T'};
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
      out[i] = kBase[(ix.text[p >> 4] >> ((p & 15) * 2)) & 3u];
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

void format_reads(const BowtieArgs& a, uint64_t lo, uint64_t hi, std::string& out, BlockCounts& c) {
  std::string q, ref, qual;
  for (uint64_t r = lo; r < hi; ++r) {
    const char* name = a.names + a.names_off[r];
    const size_t name_len = (size_t)(a.names_off[r + 1] - a.names_off[r]);
    const char* seq = a.seqs + a.seqs_off[r];
    const uint32_t L = (uint32_t)(a.seqs_off[r + 1] - a.seqs_off[r]);
    const uint64_t k0 = a.offsets[r], k1 = a.offsets[r + 1];
    qual.assign(L, 'I');
    if ((a.suppressed && a.suppressed[r]) || k0 == k1) {
      if (a.suppressed && a.suppressed[r]) ++c.suppressed;
      if (!a.sam) continue;
      out.append(name, name_len);
      out += "\t4\t*\t0\t0\t*\t*\t0\t0\t";
      out.append(seq, L);
      out += '\t';
      out += qual;
      out += "\tXM:i:";
      put_u64(out, (a.suppressed && a.suppressed[r]) ? (uint64_t)a.m + 1 : 0u);
      out += '\n';
      continue;
    }
    ++c.aligned;
    for (uint64_t k = k0; k < k1; ++k) {
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
        put_u64(out, a.mm[k]);
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
        put_u64(out, a.mm[k]);
      } else {
        out += minus ? "\t-\t" : "\t+\t";
        out += rname;
        out += '\t';
        put_u64(out, off);
        out += '\t';
        out += q;
        out += '\t';
        out += qual;
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
      ++c.lines;
    }
  }
}

}  // namespace

void write_bowtie(const char* path, bool sam, const char* cmdline, const std::vector<const FmIndex*>& parts, uint64_t n_reads,
                  const char* names, const uint64_t* names_off, const char* seqs, const uint64_t* seqs_off, const uint64_t* offsets,
                  const int32_t* entry, const int32_t* offset, const uint8_t* strand, const uint8_t* mm, const uint8_t* suppressed,
                  int32_t m, uint64_t* summary) {
  const Entries entries(parts);
  const int fd = path ? ::open(path, O_WRONLY | O_CREAT | O_TRUNC, 0644) : 1;
  if (fd < 0) throw std::runtime_error(std::string("cannot open ") + path);
  struct Closer {
    int fd;
    bool own;
    ~Closer() {
      if (own && fd >= 0) ::close(fd);
    }
  } closer{fd, path != nullptr};
  auto write_all = [&](const char* data, size_t len) {
    while (len) {
      const ssize_t w = ::write(fd, data, len);
      if (w < 0) {
        if (errno == EINTR) continue;
        throw std::runtime_error(std::string("write to ") + (path ? path : "standard output") + " failed");
      }
      data += w;
      len -= (size_t)w;
    }
  };
  if (sam) {
    std::string h = "@HD\tVN:1.0\tSO:unsorted\n";
    for (const FmIndex* ix : parts)
      for (size_t e = 0; e < ix->names.size(); ++e) {
        h += "@SQ\tSN:";
        h += ix->names[e];
        h += "\tLN:";
        put_u64(h, ix->ref_len[e]);
        h += '\n';
      }
    h += "@PG\tID:Bowtie\tVN:1.1.2\tCL:\"";
    h += cmdline ? cmdline : "";
    h += "\"\n";
    write_all(h.data(), h.size());
  }
  const BowtieArgs a{sam, &entries, names, names_off, seqs, seqs_off, offsets, entry, offset, strand, mm, suppressed, m};
  unsigned n_threads = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  if (const char* e = std::getenv("MIRGE_AMD_TABLE_THREADS")) n_threads = (unsigned)std::max(1, std::atoi(e));
  constexpr uint64_t kBlockReads = 1u << 16;
  const uint64_t n_blocks = (n_reads + kBlockReads - 1) / kBlockReads;
  n_threads = (unsigned)std::min<uint64_t>(n_threads, std::max<uint64_t>(n_blocks, 1));
  // turn = the block whose text goes out next: a worker formats its block, waits for its turn, writes, passes the turn on
  std::atomic<uint64_t> next{0}, turn{0}, aligned{0}, supp{0}, lines{0};
  std::atomic<bool> stop{false};
  std::vector<std::exception_ptr> failed(n_threads);
  auto worker = [&](unsigned t) {
    std::string text;
    try {
      for (;;) {
        const uint64_t b = next.fetch_add(1, std::memory_order_relaxed);
        if (b >= n_blocks || stop.load(std::memory_order_relaxed)) break;
        text.clear();
        BlockCounts c;
        format_reads(a, b * kBlockReads, std::min(n_reads, (b + 1) * kBlockReads), text, c);
        while (turn.load(std::memory_order_acquire) != b) {
          if (stop.load(std::memory_order_relaxed)) return;
          std::this_thread::yield();
        }
        write_all(text.data(), text.size());
        turn.store(b + 1, std::memory_order_release);
        aligned.fetch_add(c.aligned, std::memory_order_relaxed);
        supp.fetch_add(c.suppressed, std::memory_order_relaxed);
        lines.fetch_add(c.lines, std::memory_order_relaxed);
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
  if (path) {
    closer.own = false;
    if (::close(fd) != 0) throw std::runtime_error(std::string("cannot close ") + path);
  }
  summary[0] = n_reads;
  summary[1] = aligned.load();
  summary[2] = supp.load();
  summary[3] = lines.load();
}

}  // namespace mrg
