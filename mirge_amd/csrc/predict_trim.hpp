// Predict mode's preliminary trim of the location clusters on the device (predict_trim.hip, strung together by
// mrg_predict_trim in capi.hip): what the reference does line by line over the cluster table in
// utils/preTrimClusteredSeq.py -- OriginalSeq, the length cutoff, the poly-A / poly-T ends and the two nearest repeat
// elements -- and the retained set generate_Seq.py prints.  Internal header; everything is asynchronous on `stream`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mrg {

constexpr uint32_t kTrimRun = 6;  // `A{6,}$` and `^T{6,}`

// stat words of mrg_predict_trim (zeroed by the caller): set to 1 by the kernels when an input array contradicts another
constexpr uint32_t kTrimStatBadSeqOff = 0;  // seq_off not ascending inside [0, total_len]
constexpr uint32_t kTrimStatBadEntry = 1;   // a cluster's entry >= n_entries
constexpr uint32_t kTrimStatBadTable = 2;   // rep_off not ascending inside [0, n_elements]
constexpr uint32_t kTrimStatWords = 4;

struct TrimClusters {
  uint32_t n;               // clusters
  const uint32_t* entry;    // [n]
  const uint8_t* strand;    // [n] 0 = +, else -
  const uint32_t* start;    // [n] 1-based
  const uint32_t* end;      // [n] 1-based inclusive
  const uint64_t* seq_off;  // [n + 1]
  const char* seq;          // [total_len] ASCII
  uint64_t total_len;
};

// The repeat elements of every genome entry, sorted stably by start inside an entry.
struct TrimRepeats {
  uint32_t n_entries;
  uint32_t n_elements;
  const uint32_t* off;    // [n_entries + 1] into the element arrays
  const uint32_t* start;  // [n_elements] 1-based
  const uint32_t* end;    // [n_elements] 1-based inclusive; end < start: an element that covers nothing
};

// orig[i] for every byte of seq: a + cluster's byte, or the complement (A<->T, C<->G, anything else itself) of the byte
// mirrored inside a - cluster's own range.  One lane per output byte.
hipError_t trim_orig_launch(const TrimClusters& c, char* orig, uint32_t* stat, hipStream_t stream);

// Per cluster (one lane each, n + 1 lanes: the last writes the zeros that close the scans' inputs):
//   flag = 1 iff  seq_off[c + 1] - seq_off[c] <= cutoff,  orig does not end in kTrimRun 'A' nor begin with kTrimRun 'T',
//   and (reached only then) neither of the two elements of the cluster's entry whose start is nearest `start` shares a
//   coordinate with [start, end].  Nearest: by |element start - start|, at equal distance the lower element start, then the
//   lower element index.  rep = the nearer of the two that intersects, else the other one if it does, else -1.
//   flag32 / keep_len [n + 1]: the flag and the retained bytes as scan inputs.
hipError_t trim_flags_launch(const TrimClusters& c, const TrimRepeats& r, const char* orig, uint32_t cutoff, uint8_t* flag, int32_t* rep,
                             uint32_t* flag32, uint32_t* keep_len, uint32_t* stat, hipStream_t stream);

// kept[rank[c]] = c and kept_seq_off[rank[c]] = keep_off[c] for every retained cluster (rank / keep_off: the exclusive sums
// of flag32 / keep_len, [n + 1]); kept_seq_off[rank[n]] = keep_off[n] closes the list.
hipError_t trim_compact_launch(uint32_t n, const uint32_t* rank, const uint64_t* keep_off, uint32_t* kept, uint64_t* kept_seq_off,
                               hipStream_t stream);

// kept_orig = the retained clusters' orig bytes, one after the other (one lane per byte of orig; the bytes of a cluster that
// was not retained are skipped).
hipError_t trim_gather_launch(const TrimClusters& c, const char* orig, const uint32_t* rank, const uint64_t* keep_off, char* kept_orig,
                              hipStream_t stream);

}  // namespace mrg
