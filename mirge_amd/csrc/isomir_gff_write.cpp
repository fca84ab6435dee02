// <sample>_isomiRs.gff for every sample, from the columnar arrays and the records of mrg_isomir_classify (host side, no
// GPU).  Replaces the per-sample loop over isomiRContentDic of writeDataToCSV.py:621-646 and, for the text of a row, make_id
// and make_cigar (runAnnotationPipeline.py:180-235, called from RAP:86-446): the bytes are those of
// mirge_amd.isomir.write_isomir_gff.
//   <miRNA>\t<source>\t<type>\t<pre_start>\t<pre_end>\t.\t+\t.\tRead <seq>; UID <uid>; Name <miRNA>; Parent <precursor>;
//   Variant <list>; Cigar <cigar>; Expression <count>; Filter Pass
// A row's text is formatted once and copied to every sample that saw the read, with that sample's count.  Blocks of rows
// are formatted by worker threads and written in block order: the files do not depend on the thread count.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "host_write.hpp"
#include "isomir_gff.hpp"

namespace mrg {

namespace {

// 3-mer -> UID character (mirGFF3 / mirtop read-UID alphabet), codons in ACGT order
const char kUidChars[] = "@fcoladsmkhwgebpvtDnx#yiCEGSrjqHT84FVXZ6KM$AWY35LNJzU9P07IuBQOR%";
const char* const kSnpClass[6] = {"", "", "_seed", "_central_offset", "_central", "central_supp"};

struct GffArgs {
  uint32_t S;
  const char* source;
  const uint64_t* reads;
  uint32_t W;
  uint64_t stride;
  const uint8_t* lens;
  const uint64_t* nmask;
  uint64_t n;
  const uint32_t* quant;
  const uint32_t* idx;
  const int32_t* rec;
  const uint64_t* mask;
  uint32_t mask_words;
  const char* const* entry_names;
  const char* const* pre_names;
  uint64_t n_entries;
};

void append_signed(std::string& out, int32_t v) {  // "+3" / "-2"
  if (v > 0) out.push_back('+');
  append_int(out, v);
}

void flush_run(std::string& out, uint32_t& run) {
  if (run > 1) append_int(out, run);
  if (run) out.push_back('M');
  run = 0;
}

// rows [lo, hi): their lines appended to text[s] for every sample s that holds the read; counts[s] += lines
void format_rows(const GffArgs& a, uint64_t lo, uint64_t hi, std::vector<std::string>& text, std::vector<uint64_t>& counts) {
  std::string head, seq;
  auto code = [](char c) { return ((c >> 1) ^ (c >> 2)) & 3; };  // A, C, G, T -> 0, 1, 2, 3 (0x41, 0x43, 0x47, 0x54)
  for (uint64_t r = lo; r < hi; ++r) {
    const int32_t* rec = a.rec + r * kIsoRecInts;
    const uint32_t flags = (uint32_t)rec[kIsoRecFlags];
    const uint32_t kind = flags & 0xFFu, snp = (flags >> 8) & 0xFFu, add = (flags >> 16) & 1u;
    if (kind == kIsoDropped) continue;
    if (kind != kIsoRef && kind != kIsoIsomir) throw std::invalid_argument("row " + std::to_string(r) + " is not classified");
    const uint64_t read = a.idx[r];
    const int32_t entry = rec[kIsoRecEntry];
    if (read >= a.n || entry < 0 || (uint64_t)entry >= a.n_entries || snp > 5)
      throw std::invalid_argument("row " + std::to_string(r) + ": read or entry out of range");
    const uint32_t L = a.lens[read];
    const uint32_t lead = (uint32_t)rec[kIsoRecEnds] & 0xFFFFu, trail = (uint32_t)rec[kIsoRecEnds] >> 16;
    if (L > 32u * a.W || lead + trail > L) throw std::invalid_argument("row " + std::to_string(r) + " does not fit its read");
    const uint32_t* q = a.quant + read * a.S;
    bool seen = false;
    for (uint32_t s = 0; s < a.S && !seen; ++s) seen = q[s] >= 1;
    if (!seen) continue;
    const char* name = a.entry_names[entry];
    const char* parent = a.pre_names[entry];
    if (!name || !parent) throw std::invalid_argument("row " + std::to_string(r) + ": entry without a name");
    seq.clear();
    unpack_read(a.reads, a.nmask, a.stride, read, L, seq);
    head.clear();
    head += name;
    head.push_back('\t');
    head += a.source;
    head += kind == kIsoRef ? "\tref_miRNA\t" : "\tisomiR\t";
    append_int(head, rec[kIsoRecStart]);
    head.push_back('\t');
    append_int(head, rec[kIsoRecEnd]);
    head += "\t.\t+\t.\tRead ";
    head += seq;
    head += "; UID ";
    if (seq.find('N') != std::string::npos) {
      head.push_back('.');  // make_id: a 3-mer with a non-ACGT character has no code
    } else {
      const uint32_t full = L / 3, rest = L - 3 * full;
      for (uint32_t t = 0; t < full; ++t) head.push_back(kUidChars[16 * code(seq[3 * t]) + 4 * code(seq[3 * t + 1]) + code(seq[3 * t + 2])]);
      if (rest) {  // padded with A, followed by the pad length
        head.push_back(kUidChars[16 * code(seq[3 * full]) + (rest == 2 ? 4 * code(seq[3 * full + 1]) : 0)]);
        head.push_back(rest == 2 ? '1' : '2');
      }
    }
    head += "; Name ";
    head += name;
    head += "; Parent ";
    head += parent;
    head += "; Variant ";
    if (kind == kIsoRef) {
      head += "NA";
    } else {  // snp, add, 5p, 3p
      bool any = false;
      auto item = [&](const char* label) {
        if (any) head.push_back(',');
        any = true;
        head += label;
      };
      if (snp) {
        item("iso_snp");
        head += kSnpClass[snp];
      }
      if (add && rec[kIsoRec3p]) {
        item("iso_add:");
        append_signed(head, rec[kIsoRec3p]);
      }
      if (rec[kIsoRec5p]) {
        item("iso_5p:");
        append_signed(head, rec[kIsoRec5p]);
      }
      if (!add && rec[kIsoRec3p]) {
        item("iso_3p:");
        append_signed(head, rec[kIsoRec3p]);
      }
    }
    head += "; Cigar ";
    {  // make_cigar: runs of M (a lone one without its count), I outside the precursor, the read's base on a substitution
      const uint64_t* m = a.mask + r * a.mask_words;
      uint32_t run = 0;
      for (uint32_t i = 0; i < L; ++i) {
        if (i < lead || i >= L - trail) {
          flush_run(head, run);
          head.push_back('I');
        } else if ((m[i >> 6] >> (i & 63)) & 1ull) {
          flush_run(head, run);
          head.push_back(seq[i]);
        } else {
          ++run;
        }
      }
      flush_run(head, run);
    }
    head += "; Expression ";
    for (uint32_t s = 0; s < a.S; ++s) {
      if (q[s] < 1) continue;
      text[s] += head;
      append_int(text[s], q[s]);
      text[s] += "; Filter Pass\n";
      ++counts[s];
    }
  }
}

}  // namespace

void write_isomir_gff(const char* const* paths, const char* const* coldata, uint32_t S, const char* source, const uint64_t* reads,
                      uint32_t W, uint64_t stride, const uint8_t* lens, const uint64_t* nmask, uint64_t n, const uint32_t* quant,
                      const uint32_t* idx, const int32_t* rec, const uint64_t* mask, uint64_t k, const char* const* entry_names,
                      const char* const* pre_names, uint64_t n_entries, uint64_t* rows) {
  const GffArgs a{S, source, reads, W, stride, lens, nmask, n, quant, idx, rec, mask, (W + 1) / 2, entry_names, pre_names, n_entries};
  std::vector<std::unique_ptr<File>> files;
  for (uint32_t s = 0; s < S; ++s) {
    files.emplace_back(new File(paths[s]));
    std::string header = "# GFF3 adapted for miRNA sequencing data\n## VERSION 0.0.1\n## source-ontology: ";
    header += source;
    header += "\n## COLDATA: ";
    header += coldata[s];
    header += "\n";
    files[s]->write(header);
  }
  const uint64_t block_rows = env_count("MIRGE_AMD_GFF_BLOCK_ROWS", 1u << 15);  // (tests lower it)
  const uint64_t n_blocks = (k + block_rows - 1) / block_rows;
  const unsigned n_threads = writer_threads(n_blocks);
  // each worker formats one block into its own S strings, then the blocks are written in order
  std::vector<std::vector<std::string>> text(n_threads, std::vector<std::string>(S));
  std::vector<std::vector<uint64_t>> counts(n_threads, std::vector<uint64_t>(S, 0));
  in_batches(n_blocks, n_threads,
             [&](unsigned t, uint64_t b) {
               for (auto& x : text[t]) x.clear();
               format_rows(a, b * block_rows, std::min(k, (b + 1) * block_rows), text[t], counts[t]);
             },
             [&](uint64_t, unsigned live) {
               for (unsigned t = 0; t < live; ++t)
                 for (uint32_t s = 0; s < S; ++s) files[s]->write(text[t][s]);
             });
  for (uint32_t s = 0; s < S; ++s) {
    files[s]->close();
    if (rows) {
      rows[s] = 0;
      for (unsigned t = 0; t < n_threads; ++t) rows[s] += counts[t][s];
    }
  }
}

}  // namespace mrg
