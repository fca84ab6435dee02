// `-tcf`: the order of <sample>.trim.collapse.fa (quantReads.py:26-44: every distinct read of the sample by count, then by
// sequence, both descending) from the packed reads and quant (csrc/collapsed_order.hip, strung together by mrg_seq_rank /
// mrg_collapsed_order in capi.hip) and the writer of the file (collapsed_fa_write.cpp, mrg_write_collapsed_fasta).
// Internal header.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mrg {

constexpr uint32_t kSeqChunkBases = 21;  // 3 bits per base in a 64-bit key

// stat words of mrg_seq_rank / mrg_collapsed_order
constexpr int kSeqStatTooLong = 0;   // a read is longer than max_len or than its words hold
constexpr int kSeqStatMaxCount = 1;  // the largest count of the sample column
constexpr uint32_t kSeqStatWords = 4;

struct SeqRankParams {
  const uint64_t* reads;  // [W][stride]
  const uint64_t* nmask;  // or nullptr
  const uint8_t* lens;
  uint64_t stride;
  uint32_t n, W, max_len;
};

// vals[i] = i
hipError_t seq_iota_launch(uint32_t* vals, uint32_t n, hipStream_t stream);
// keys[j] = bases [21 c, 21 c + nb) of read perm[j], nb = min(21, max_len - 21 c), 3 bits each in the low 3 nb bits, first base
// highest: end of read 0, A 1, C 2, G 3, N 4, T 5 (Python string order, a proper prefix first).  Only the first lens[u]
// bases of a read are looked at.  A read longer than max_len or than 32 W sets stat[kSeqStatTooLong].
hipError_t seq_chunk_keys_launch(const SeqRankParams& p, const uint32_t* perm, uint32_t chunk, uint64_t* keys, uint32_t* stat,
                                 hipStream_t stream);
// rank[perm[j]] = j
hipError_t seq_rank_scatter_launch(const uint32_t* perm, uint32_t n, uint32_t* rank, hipStream_t stream);

// flags[u] = quant[u][s] > 0 for u < n, flags[n] = 0; stat[kSeqStatMaxCount] = the largest count
hipError_t collapsed_flags_launch(const uint32_t* quant, uint32_t n, uint32_t S, uint32_t s, uint32_t* flags, uint32_t* stat,
                                  hipStream_t stream);
// read u of the sample (scan = the exclusive sums of flags, [n + 1]): keys[scan[u]] = count << rank_bits | rank[u], vals[..] = u
hipError_t collapsed_keys_launch(const uint32_t* scan, const uint32_t* quant, uint32_t n, uint32_t S, uint32_t s, const uint32_t* rank,
                                 uint32_t rank_bits, uint64_t* keys, uint32_t* vals, hipStream_t stream);
// order[j] = vals[k - 1 - j]
hipError_t collapsed_reverse_launch(const uint32_t* vals, uint32_t k, uint32_t* order, hipStream_t stream);

struct CollapsedFaArgs {
  const char* path;
  const uint64_t* reads;  // [W][stride]
  uint32_t W;
  uint64_t stride;
  const uint8_t* lens;
  const uint64_t* nmask;  // or nullptr
  uint64_t n;
  const uint32_t* quant;  // [n][S]
  uint32_t S, sample;
  const uint32_t* order;  // [k]
  uint64_t k;
  const char* const* extra_seqs;  // [n_extra], by (count, sequence) descending
  const uint64_t* extra_counts;
  uint64_t n_extra;
};
// Returns the rows written.  Throws std::invalid_argument (an order entry out of range or without a count in the sample,
// extra rows out of order: nothing is written) or std::runtime_error (I/O).
uint64_t write_collapsed_fasta(const CollapsedFaArgs& a);

}  // namespace mrg
