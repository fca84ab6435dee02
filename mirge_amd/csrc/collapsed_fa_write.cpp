// <sample>.trim.collapse.fa from the columnar arrays and the order of mrg_collapsed_order (host side, no GPU).  Replaces the
// sort and the row loop of quantReads.py:26-44:
//   >seq<i>_<count>
//   <sequence>
// for i = 1.. over the sample's distinct reads by (count, sequence) descending.  The reads beyond 255 nt, which the packed
// arrays do not hold, come as extra rows in that order and are merged in by the same comparison.  `order` is checked in full
// before the file is opened: an entry that is no read, or a read without a count in the sample, writes nothing.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>

#include "collapsed_order.hpp"
#include "host_write.hpp"

namespace mrg {

namespace {

// Python's str comparison of two ASCII strings: < 0, 0, > 0
int compare(const char* x, size_t nx, const char* y, size_t ny) {
  const int c = std::memcmp(x, y, nx < ny ? nx : ny);
  return c ? c : nx < ny ? -1 : nx > ny ? 1 : 0;
}

void append_row(std::string& out, uint64_t i, uint64_t count, const char* seq, size_t len) {
  char head[64];
  const int h = std::snprintf(head, sizeof head, ">seq%llu_%llu\n", (unsigned long long)i, (unsigned long long)count);
  out.append(head, (size_t)h);
  out.append(seq, len);
  out.push_back('\n');
}

}  // namespace

uint64_t write_collapsed_fasta(const CollapsedFaArgs& a) {
  for (uint64_t j = 0; j < a.k; ++j) {
    const uint64_t u = a.order[j];
    if (u >= a.n) throw std::invalid_argument("order[" + std::to_string(j) + "] = " + std::to_string(u) + " is no read of " + std::to_string(a.n));
    if (a.quant[u * a.S + a.sample] == 0)
      throw std::invalid_argument("order[" + std::to_string(j) + "]: read " + std::to_string(u) + " has no count in sample " +
                                  std::to_string(a.sample));
    if (a.lens[u] > 32u * a.W) throw std::invalid_argument("read " + std::to_string(u) + " does not fit its words");
  }
  for (uint64_t e = 0; e < a.n_extra; ++e) {
    if (!a.extra_seqs[e]) throw std::invalid_argument("extra row " + std::to_string(e) + ": null sequence");
    if (a.extra_counts[e] == 0) throw std::invalid_argument("extra row " + std::to_string(e) + " has no count");
    if (e && (a.extra_counts[e - 1] < a.extra_counts[e] ||
              (a.extra_counts[e - 1] == a.extra_counts[e] && std::strcmp(a.extra_seqs[e - 1], a.extra_seqs[e]) < 0)))
      throw std::invalid_argument("extra rows " + std::to_string(e - 1) + " and " + std::to_string(e) + " are not in descending order");
  }
  File out(a.path);
  constexpr size_t kFlush = 1u << 20;
  std::string text;
  text.reserve(kFlush + 4096);
  char seq[256];
  uint64_t j = 0, e = 0, row = 0;
  while (j < a.k || e < a.n_extra) {
    bool take_extra = j >= a.k;
    uint32_t L = 0;
    uint64_t count = 0;
    if (j < a.k) {
      const uint64_t u = a.order[j];
      count = a.quant[u * a.S + a.sample];
      L = a.lens[u];
      unpack_read(a.reads, a.nmask, a.stride, u, L, seq);
      if (e < a.n_extra)
        take_extra = a.extra_counts[e] != count ? a.extra_counts[e] > count
                                                : compare(a.extra_seqs[e], std::strlen(a.extra_seqs[e]), seq, L) > 0;
    }
    if (take_extra) {
      append_row(text, ++row, a.extra_counts[e], a.extra_seqs[e], std::strlen(a.extra_seqs[e]));
      ++e;
    } else {
      append_row(text, ++row, count, seq, L);
      ++j;
    }
    if (text.size() >= kFlush) {
      out.write(text);
      text.clear();
    }
  }
  out.write(text);
  out.close();
  return row;
}

}  // namespace mrg
