// a2IEditing.detail.txt from the columnar arrays and the records of mrg_a2i_align (host side, no GPU).  Replaces the
// detail.write calls of A2IEditing (writeDataToCSV.py:145-229, mirge_amd.a2i.a2i_editing): one block per (miRNA, sample)
//   Canonical_Seq of <miRNA>: <target>
//   seqList size is: <k>, <k>
//   <read in the block's frame>\t<count>\t<True|False>       every read
//   ****************
//   retained seqList size is: <reads judged True that the genome filter retained>
//   ...                                                      the reads judged True
//   ****************
//   retained sequences after filering are:
//   ...                                                      the reads judged True that the genome filter retained
// The frame of a block holds `head` dashes in front of the target and `tail` behind it; a read of diagonal d starts at
// head + d.  A block that comes with its own text (the Python route formatted it) is written as it is.
// Runs of blocks are formatted by worker threads and written in block order: the bytes depend on neither the thread
// count nor the run length.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "a2i_align.hpp"
#include "host_write.hpp"

namespace mrg {

namespace {

[[noreturn]] void bad_block(uint64_t b, const char* what) { throw std::invalid_argument("block " + std::to_string(b) + ": " + what); }

// blocks [lo, hi): their text appended to `text`, their lines added to `lines`
void format_blocks(const A2iDetailArgs& a, uint64_t lo, uint64_t hi, std::string& text, uint64_t& lines) {
  std::vector<std::string> row_text;
  char num[32];
  for (uint64_t b = lo; b < hi; ++b) {
    if (a.block_text && a.block_text[b]) {
      const size_t len = std::strlen(a.block_text[b]);
      text.append(a.block_text[b], len);
      lines += (uint64_t)std::count(a.block_text[b], a.block_text[b] + len, '\n');
      continue;
    }
    const uint64_t r0 = a.block_off[b], r1 = a.block_off[b + 1];
    const int32_t g = a.block_group[b];
    if (r1 < r0) bad_block(b, "row offsets decrease");
    if (g < 0 || (uint64_t)g >= a.n_groups) bad_block(b, "group out of range");
    const int64_t head = a.block_frame[2 * b], tail = a.block_frame[2 * b + 1];
    const int64_t la = (int64_t)std::strlen(a.group_targets[g]);
    if (head < 0 || tail < 0 || head > 255 || tail > 255) bad_block(b, "frame out of range");
    const int64_t width = head + la + tail;
    row_text.assign(r1 - r0, std::string());
    uint64_t n_true = 0, n_kept = 0;
    for (uint64_t r = r0; r < r1; ++r) {
      const uint64_t read = a.row_read[r];
      if (read >= a.n) bad_block(b, "read out of range");
      const int64_t L = a.lens[read], at = head + a.row_d[r];
      if (L > 32 * (int64_t)a.W) bad_block(b, "a read does not fit its words");
      if (at < 0 || at + L > width) bad_block(b, "a read does not fit the frame");
      std::string& line = row_text[r - r0];
      line.assign((size_t)at, '-');
      unpack_read(a.reads, a.nmask, a.stride, read, (uint32_t)L, line);
      line.append((size_t)(width - at - L), '-');
      const int len = std::snprintf(num, sizeof num, "\t%u\t", a.row_count[r]);
      line.append(num, (size_t)len);
      line += (a.row_flags[r] & 1) ? "True\n" : "False\n";
      n_true += (a.row_flags[r] & 1) ? 1 : 0;
      n_kept += (a.row_flags[r] & 3) == 3 ? 1 : 0;
    }
    text += "Canonical_Seq of ";
    text += a.group_names[g];
    text += ": ";
    text += a.group_targets[g];
    text.push_back('\n');
    const std::string k = std::to_string(r1 - r0);
    text += "seqList size is: " + k + ", " + k + "\n";
    for (const std::string& line : row_text) text += line;
    text += "****************\nretained seqList size is: " + std::to_string(n_kept) + "\n";
    for (uint64_t r = r0; r < r1; ++r)
      if (a.row_flags[r] & 1) text += row_text[r - r0];
    text += "****************\nretained sequences after filering are:\n";
    for (uint64_t r = r0; r < r1; ++r)
      if ((a.row_flags[r] & 3) == 3) text += row_text[r - r0];
    lines += 5 + (r1 - r0) + n_true + n_kept;
  }
}

}  // namespace

void write_a2i_detail(const A2iDetailArgs& a, uint64_t* lines) {
  File out(a.path);
  const uint64_t run = env_count("MIRGE_AMD_A2I_RUN_BLOCKS", 256);  // blocks per worker and round (tests lower it)
  const uint64_t n_runs = (a.n_blocks + run - 1) / run;
  const unsigned n_threads = writer_threads(n_runs);
  std::vector<std::string> text(n_threads);
  std::vector<uint64_t> count(n_threads, 0);
  uint64_t total = 0;
  in_batches(n_runs, n_threads,
             [&](unsigned t, uint64_t r) {
               text[t].clear();
               count[t] = 0;
               format_blocks(a, r * run, std::min(a.n_blocks, (r + 1) * run), text[t], count[t]);
             },
             [&](uint64_t, unsigned live) {
               for (unsigned t = 0; t < live; ++t) {
                 out.write(text[t]);
                 total += count[t];
               }
             });
  out.close();
  if (lines) *lines = total;
}

}  // namespace mrg
