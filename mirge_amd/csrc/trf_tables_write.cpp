// tRFs.potential.report.tsv, discarded.reads.summary.assigningtRFs.csv, tRF.Counts.csv and tRF.RP100K.csv from the columnar
// arrays and the rows of mrg_trf_classify (host side, no GPU).  Replaces the per-read loop of writeDataToCSV.py:648-800; the
// bytes are those of mirge_amd.trf.write_trf_tables with choose = min.
//   <read>\t<uid>\t<counts>\t<RP100K>\t<aa, all hits>\t<aa-anticodon, all hits>\t<name:type:start:end, all hits>\t
//   <the same three over the de-duplicated hits>\t<the same three for the selected tRNA>
// "All hits" walks a read's alignments from the highest entry down (the dict order the Python route builds from the
// reversed listing); the de-duplicated hits are the representatives' names in Python string order (their ranks).
// Blocks of rows are formatted by worker threads and written in block order.  The per-entity sums are added afterwards,
// row by row in one thread, from the RP100K values re-read from their 3-decimal text, as the reference adds them: the
// files depend on neither the thread count nor the block size.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "host_write.hpp"
#include "trf_tables.hpp"

namespace mrg {

namespace {

// 3-mer -> UID character (make_id, as isomir_gff_write.cpp), codons in ACGT order
const char kUidChars[] = "@fcoladsmkhwgebpvtDnx#yiCEGSrjqHT84FVXZ6KM$AWY35LNJzU9P07IuBQOR%";
const char* const kTypeName[7] = {"tRF-1", "tRF-whole", "5'-half", "5'-tRF", "3'-half", "3'-tRF", "i-tRF"};

[[noreturn]] void bad_row(uint64_t r, const char* what) { throw std::invalid_argument("row " + std::to_string(r) + ": " + what); }

void add_unique(std::vector<std::string>& list, const std::string& item) {
  if (std::find(list.begin(), list.end(), item) == list.end()) list.push_back(item);
}

void join(std::string& out, const std::vector<std::string>& items) {
  for (size_t i = 0; i < items.size(); ++i) {
    if (i) out.push_back(',');
    out += items[i];
  }
}

// rows [lo, hi): their lines appended to text; written[r] = 1 and rp[r * S + s] = float("%.3f" % RP100K) for a written row
void format_rows(const TrfWriteArgs& a, uint64_t lo, uint64_t hi, std::string& text, std::vector<uint8_t>& written,
                 std::vector<double>& rp) {
  std::string seq;
  auto code = [](char c) { return ((c >> 1) ^ (c >> 2)) & 3; };  // A, C, G, T -> 0, 1, 2, 3 (0x41, 0x43, 0x47, 0x54)
  std::vector<std::string> aa_types, aa_pairs, infos, d_types, d_pairs, d_infos;
  std::vector<int32_t> reps;
  char num[400];
  auto info = [&](std::string& out, const int32_t* hit) {
    out += a.entry_names[hit[0]];
    out.push_back(':');
    out += kTypeName[hit[3]];
    out.push_back(':');
    append_int(out, (long long)hit[1] + 1);
    out.push_back(':');
    append_int(out, (long long)hit[2] + 1);
  };
  auto aa_of = [&](int32_t name_entry, int32_t type_entry) {
    std::string t = (a.desc[(uint64_t)name_entry * kTrfDescInts + kTrfDescFlags] & 1) ? "pre:" : "";
    return t + a.aa_types[type_entry];
  };
  for (uint64_t r = lo; r < hi; ++r) {
    const int32_t* rec = a.rec + r * kTrfRecInts;
    const uint32_t kind = (uint32_t)rec[kTrfRecKind];
    if (kind == kTrfNoCandidate) continue;   // (the read is dropped, as `del trfContentDic[read]`)
    if (kind > kTrfDele) bad_row(r, "not classified");
    const uint64_t read = (uint32_t)rec[kTrfRecRead];
    const int64_t h0 = rec[kTrfRecHit0], nh = rec[kTrfRecHits];
    const int32_t sel = rec[kTrfRecEntry];
    if (read >= a.n || h0 < 0 || nh < 1 || (uint64_t)(h0 + nh) > a.h || sel < 0 || (uint64_t)sel >= a.n_entries)
      bad_row(r, "read, alignments or entry out of range");
    const uint32_t L = a.lens[read];
    if (L > 32u * a.W) bad_row(r, "the read does not fit its words");
    const int32_t* hits = a.hits + h0 * kTrfHitInts;
    for (int64_t j = 0; j < nh; ++j) {
      const int32_t* hit = hits + j * kTrfHitInts;
      if (hit[0] < 0 || (uint64_t)hit[0] >= a.n_entries || hit[3] < 0 || hit[3] > 6) bad_row(r, "an alignment is not typed");
      if (!a.entry_names[hit[0]] || !a.aa_types[hit[0]] || !a.anticodons[hit[0]]) bad_row(r, "an entry without amino acid");
    }
    seq.clear();
    unpack_read(a.reads, a.nmask, a.stride, read, L, seq);
    text += seq;
    text.push_back('\t');
    if (seq.find('N') != std::string::npos) {
      text.push_back('.');  // make_id: a 3-mer with a non-ACGT character has no code
    } else {
      const uint32_t full = L / 3, rest = L - 3 * full;
      for (uint32_t t = 0; t < full; ++t) text.push_back(kUidChars[16 * code(seq[3 * t]) + 4 * code(seq[3 * t + 1]) + code(seq[3 * t + 2])]);
      if (rest) {  // padded with A, followed by the pad length
        text.push_back(kUidChars[16 * code(seq[3 * full]) + (rest == 2 ? 4 * code(seq[3 * full + 1]) : 0)]);
        text.push_back(rest == 2 ? '1' : '2');
      }
    }
    text.push_back('\t');
    const uint32_t* q = a.quant + read * a.S;
    for (uint32_t s = 0; s < a.S; ++s) {
      if (s) text.push_back(',');
      append_int(text, q[s]);
    }
    text.push_back('\t');
    for (uint32_t s = 0; s < a.S; ++s) {
      const double v = a.denom[s] ? 100000.0 * (double)q[s] / (double)a.denom[s] : 0.0;
      const int len = std::snprintf(num, sizeof num, "%.3f", v);
      if (s) text.push_back(',');
      text.append(num, (size_t)len);
      rp[r * a.S + s] = std::strtod(num, nullptr);
    }
    // all hits, from the highest entry down
    aa_types.clear();
    aa_pairs.clear();
    infos.clear();
    reps.clear();
    for (int64_t j = nh - 1; j >= 0; --j) {
      const int32_t* hit = hits + j * kTrfHitInts;
      infos.emplace_back();
      info(infos.back(), hit);
      const std::string t = aa_of(hit[0], hit[0]);
      if (t != "Und" && t != "pre:Und") {
        add_unique(aa_pairs, t + "-" + a.anticodons[hit[0]]);
        add_unique(aa_types, t);
      }
      reps.push_back(a.desc[(uint64_t)hit[0] * kTrfDescInts + kTrfDescRep]);
    }
    // the de-duplicated hits: sorted(set(dup.get(c, c))), each of them an alignment of this read
    auto hit_of = [&](int32_t entry) -> const int32_t* {
      for (int64_t j = 0; j < nh; ++j)
        if (hits[j * kTrfHitInts] == entry) return hits + j * kTrfHitInts;
      return nullptr;
    };
    for (int32_t u : reps)
      if (u < 0 || !hit_of(u)) bad_row(r, "a de-duplicated tRNA is no alignment of the read");
    std::sort(reps.begin(), reps.end(), [&](int32_t x, int32_t y) {
      return a.desc[(uint64_t)x * kTrfDescInts + kTrfDescRank] < a.desc[(uint64_t)y * kTrfDescInts + kTrfDescRank];
    });
    reps.erase(std::unique(reps.begin(), reps.end()), reps.end());
    if (reps[0] != sel) bad_row(r, "the selected tRNA is not the smallest de-duplicated name");
    d_types.clear();
    d_pairs.clear();
    d_infos.clear();
    for (int32_t u : reps) {
      d_types.push_back(aa_of(u, sel));   // (W2C:727: the type of every de-duplicated hit is read from the selected tRNA)
      d_pairs.push_back(d_types.back() + "-" + a.anticodons[u]);
      d_infos.emplace_back();
      info(d_infos.back(), hit_of(u));
    }
    for (const auto* col : {&aa_types, &aa_pairs, &infos, &d_types, &d_pairs, &d_infos}) {
      text.push_back('\t');
      join(text, *col);
    }
    const std::string one = aa_of(sel, sel);
    text.push_back('\t');
    text += one;
    text.push_back('\t');
    text += one;
    text.push_back('-');
    text += a.anticodons[sel];
    text.push_back('\t');
    info(text, hit_of(sel));
    text.push_back('\n');
    written[r] = 1;
  }
}

}  // namespace

void write_trf_tables(const TrfWriteArgs& a, uint64_t* rows) {
  const uint32_t S = a.S;
  std::string samples;
  for (uint32_t s = 0; s < S; ++s) {
    if (s) samples.push_back(',');
    samples += a.samples[s];
  }
  File tsv(a.paths[0]);
  tsv.write("read sequence\tuid\tread count(" + samples + ")\tRP100K (" + samples +
            ")\tamino acid all hits\tamino acid-anticodon all hits\ttRF information all hits\tamino acid all deduplicated "
            "hits\tamino acid-anticodon all deduplicated hits\ttRF information all deduplicated hits\tamino acid one hit\tamino "
            "acid-anticodon one hit\ttRF information one hit\n");
  const uint64_t block_rows = env_count("MIRGE_AMD_TRF_BLOCK_ROWS", 1u << 14);  // (tests lower it)
  const uint64_t n_blocks = (a.k + block_rows - 1) / block_rows;
  const unsigned n_threads = writer_threads(n_blocks);
  std::vector<uint8_t> written(a.k, 0);
  std::vector<double> rp(a.k * S, 0.0);
  // each worker formats one block into its own string, then the blocks are written in order
  std::vector<std::string> text(n_threads);
  in_batches(n_blocks, n_threads,
             [&](unsigned t, uint64_t b) {
               text[t].clear();
               format_rows(a, b * block_rows, std::min(a.k, (b + 1) * block_rows), text[t], written, rp);
             },
             [&](uint64_t, unsigned live) {
               for (unsigned t = 0; t < live; ++t) tsv.write(text[t]);
             });
  tsv.close();

  // W2C:749-800: counts per predefined tRF entity, in row order
  std::vector<uint64_t> entity_count(a.n_merged * S, 0), discarded(S, 0), total(S, 0);
  std::vector<double> entity_rp(a.n_merged * S, 0.0);
  uint64_t n_rows = 0;
  for (uint64_t r = 0; r < a.k; ++r) {
    if (!written[r]) continue;
    ++n_rows;
    const int32_t* rec = a.rec + r * kTrfRecInts;
    const uint32_t* q = a.quant + (uint64_t)(uint32_t)rec[kTrfRecRead] * S;
    int64_t m = -1;
    if ((uint32_t)rec[kTrfRecKind] == kTrfAssigned) {
      const int32_t c = rec[kTrfRecCluster];
      if (c < 0 || (uint64_t)c >= a.n_clusters) bad_row(r, "predefined tRF out of range");
      m = a.clusters[(uint64_t)c * kTrfClusterInts + kTrfClusterMerged];
      if (m < 0 || (uint64_t)m >= a.n_merged) bad_row(r, "a predefined tRF without merged entity");
    }
    for (uint32_t s = 0; s < S; ++s) {
      total[s] += q[s];
      if (m >= 0) {
        entity_count[(uint64_t)m * S + s] += q[s];
        entity_rp[(uint64_t)m * S + s] += rp[r * S + s];
      } else {
        discarded[s] += q[s];
      }
    }
  }
  char num[400];
  {
    File f(a.paths[1]);
    std::string out = "sample name,percentage of discarded reads,details\n";
    for (uint32_t s = 0; s < S; ++s) {
      const double pct = total[s] ? (double)discarded[s] / (double)total[s] * 100.0 : 0.0;
      out += a.samples[s];
      const int len = std::snprintf(num, sizeof num, ",%.2f%%,%llu\\%llu\n", pct, (unsigned long long)discarded[s],
                                    (unsigned long long)total[s]);
      out.append(num, (size_t)len);
    }
    f.write(out);
    f.close();
  }
  {
    File f1(a.paths[2]), f2(a.paths[3]);
    std::string o1 = "entry name," + samples + "\n", o2 = o1;
    for (uint64_t m = 0; m < a.n_merged; ++m) {
      o1 += a.merged_names[m];
      o2 += a.merged_names[m];
      for (uint32_t s = 0; s < S; ++s) {
        o1.push_back(',');
        append_int(o1, (long long)entity_count[m * S + s]);
        const int len = std::snprintf(num, sizeof num, ",%.2f", entity_rp[m * S + s]);
        o2.append(num, (size_t)len);
      }
      o1.push_back('\n');
      o2.push_back('\n');
    }
    f1.write(o1);
    f2.write(o2);
    f1.close();
    f2.close();
  }
  if (rows) *rows = n_rows;
}

}  // namespace mrg
