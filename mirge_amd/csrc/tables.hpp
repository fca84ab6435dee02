// Streaming writers of mapped.csv / unmapped.csv from columnar arrays (internal header).
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace mrg {

// str(float) as Python 2.7 prints it (%.12g, `.0` appended when neither `.` nor `e` shows), appended to out; tables.cpp.
void py2_float(double x, std::string& out);

// Returns the number of rows written; throws std::runtime_error on I/O errors.
uint64_t write_read_table(const char* path, bool mapped, const char* header, bool append, const uint64_t* reads,
                          uint32_t W, uint64_t stride, const uint8_t* lens, const uint64_t* nmask, uint64_t n,
                          const int8_t* pass_id, const int32_t* ref_id, const uint32_t* quant, uint32_t n_samples,
                          uint32_t n_slots, const char* const* names, const uint64_t* names_off);

// isomirs.csv + isomirs.samples.csv (writeDataToCSV.py:1090-1170) from the arrays: reads claimed by canon_pass / isomir_pass
// grouped by group_of_entry[ref] (the miRNA name with its SNP suffix stripped), groups in order of first appearance.
// Returns the rows of isomirs.csv; throws std::runtime_error.
uint64_t write_isomir_tables(const char* isomirs_path, const char* samples_path, const char* header1, const char* header2,
                             const uint64_t* reads, uint32_t W, uint64_t stride, const uint8_t* lens, const uint64_t* nmask,
                             uint64_t n, const int8_t* pass_id, const int32_t* ref_id, const uint32_t* quant, uint32_t S,
                             int32_t canon_pass, int32_t isomir_pass, const int32_t* group_of_entry, uint64_t n_entries,
                             const char* const* group_names, uint32_t n_groups, const double* filtered);

struct FmIndex;
// bowtie 1.1.2's SAM / default text (mrg_write_bowtie, include/mirge_amd.h); bowtie_out.cpp.  Throws std::runtime_error.
void write_bowtie(const char* path, bool sam, const char* cmdline, const std::vector<const FmIndex*>& parts, uint64_t n_reads,
                  const char* names, const uint64_t* names_off, const char* seqs, const uint64_t* seqs_off, const uint64_t* offsets,
                  const int32_t* entry, const int32_t* offset, const uint8_t* strand, const uint8_t* mm, const uint8_t* suppressed,
                  int32_t m, uint64_t* summary);
// Predict mode (mrg_write_sorted_sam, mrg_write_clusters, mrg_read_counts_from_names); bowtie_out.cpp.  The writers throw
// std::runtime_error; read_counts_from_names returns the first read whose name has no `_<count>` field, or -1.
void write_sorted_sam(const char* path, const std::vector<const FmIndex*>& parts, uint64_t n_reads, const char* names,
                      const uint64_t* names_off, const char* seqs, const uint64_t* seqs_off, uint64_t n_rows, const uint32_t* row_read,
                      const int32_t* entry, const int32_t* offset, const uint8_t* strand, const uint8_t* mm, const uint8_t* suppressed,
                      int32_t m, uint64_t* summary);
void write_clusters(const char* path, const char* sample, const std::vector<const FmIndex*>& parts, uint64_t n_clusters,
                    const uint32_t* entry, const uint8_t* strand, const uint32_t* start, const uint32_t* end, const uint64_t* seq_off,
                    const char* seq, const uint64_t* count_sum, const uint32_t* member_off, const uint32_t* members, uint64_t n_reads,
                    const char* names, const uint64_t* names_off, uint64_t* rows);
// mrg_write_trimmed_clusters: the cluster arrays of write_clusters plus flag / rep / orig of mrg_predict_trim and the repeat
// table's names.  Throws std::invalid_argument (arrays that contradict each other: nothing is written) or std::runtime_error.
struct TrimmedClustersArgs {
  const char *tsv_path, *fa_path, *orig_fa_path, *sample;
  const std::vector<const FmIndex*>* parts;
  uint64_t n_clusters;
  const uint32_t* entry;
  const uint8_t* strand;
  const uint32_t *start, *end;
  const uint64_t* seq_off;
  const char* seq;
  const uint64_t* count_sum;
  const uint32_t *member_off, *members;
  uint64_t n_reads;
  const char* names;
  const uint64_t* names_off;
  const uint8_t* flag;
  const int32_t* rep;  // element index or -1
  const char* orig;
  uint64_t n_elements;
  const uint32_t* rep_name_id;  // [n_elements]
  uint64_t n_rep_names;
  const char* rep_names;
  const uint64_t* rep_names_off;  // [n_rep_names + 1]
};
void write_trimmed_clusters(const TrimmedClustersArgs& a, uint64_t* rows, uint64_t* kept);
// mrg_write_remapped_rows: the packed reads with their numbers and counts, the cluster library (its entry names are the
// cluster names) with the retained clusters' OriginalSeq bytes, and the rows of mrg_predict_remap_rows.  Throws
// std::invalid_argument (arrays that contradict each other: the file is not opened) or std::runtime_error.  Returns the lines.
struct RemappedRowsArgs {
  const char* path;
  const uint64_t* reads;  // [W][stride]
  uint32_t W;
  uint64_t stride;
  const uint8_t* lens;
  const uint64_t* nmask;  // or null
  uint64_t n_reads;
  const uint32_t *numbers, *counts;  // `mir<number>_<count>`
  const FmIndex* clusters;
  uint64_t n_clusters;
  const uint64_t* kept_seq_off;  // [n_clusters + 1]
  const char* kept_orig;
  uint64_t n_rows;
  const uint32_t *row_read, *row_cluster, *row_offset;
  const uint8_t *row_mm, *row_pass;
  uint32_t trim5, trim3;  // what a pass-2 row's aligned sequence lost
};
uint64_t write_remapped_rows(const RemappedRowsArgs& a);
int64_t read_counts_from_names(uint64_t n_reads, const char* names, const uint64_t* names_off, uint32_t* counts);

}  // namespace mrg
