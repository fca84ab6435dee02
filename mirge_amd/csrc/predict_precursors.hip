// Predict mode's precursor candidates on the device (mrg_predict_precursors / mrg_predict_precursor_bases,
// include/mirge_amd.h): the two genome windows get_precursors.py cuts around the stable part of every cluster the feature
// file holds.  gfx950, wave64, no LDS, no atomics, no scratch: one lane per group (precursor_windows_kernel,
// precursor_compact_kernel), per record (precursor_check_kernel) or per output byte (precursor_bases_kernel); every output
// word has one writer and nothing depends on lane order.  The stat words are the one exception to "one writer": every lane
// that finds an input array contradicting another stores the same 1 there.  The scans between the kernels are
// prims::exclusive_sum_u32 / _to_u64, called from capi.hip.
//
// precursor_bases_kernel stores one byte per lane: the 64 lanes of a wave write 64 consecutive bytes, which the memory
// pipeline merges into whole lines, and a record (about 110 bytes) would need padding to be written a dword at a time.
// Its two binary searches (the record of a byte, the segment of a base) diverge only where a wave crosses a record or a
// segment: neighbouring lanes walk the same path.
#include "predict_precursors.hpp"

namespace mrg {

namespace {

constexpr uint32_t kThreads = 256;

inline uint32_t grid_for(uint64_t n) { return (uint32_t)((n + kThreads - 1) / kThreads); }

__device__ __forceinline__ void set_stat(uint32_t* __restrict__ stat, uint32_t word) { stat[word] = 1u; }

__global__ __launch_bounds__(kThreads) void precursor_windows_kernel(PrecGroups g, PrecClusters cl, uint8_t* __restrict__ written,
                                                                    uint32_t* __restrict__ flag32, uint32_t* __restrict__ win,
                                                                    uint32_t* __restrict__ stat) {
  const uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (j > g.n_order) return;
  if (j == g.n_order) {
    flag32[j] = 0u;
    return;
  }
  uint32_t w = 0u, out[4] = {0u, 0u, 0u, 0u};
  const uint32_t grp = g.order[j];
  if (grp >= g.n_groups || g.valid[grp] == 0) {
    set_stat(stat, kPrecStatBadGroup);
  } else {
    const uint32_t c = g.group_cluster[grp];
    const uint32_t entry = c < cl.n ? cl.entry[c] : 0u;
    if (c >= cl.n) {
      set_stat(stat, kPrecStatBadCluster);
    } else if (entry >= cl.n_entries) {
      set_stat(stat, kPrecStatBadEntry);
    } else {
      const int64_t H = g.frame[4 * (uint64_t)grp], T = g.frame[4 * (uint64_t)grp + 1], head = g.frame[4 * (uint64_t)grp + 2];
      const int64_t tail_add = -(int64_t)g.frame[4 * (uint64_t)grp + 3] - 1;
      const int64_t start = cl.start[c], end = cl.end[c], len = cl.entry_len[entry];
      const int64_t pad_h = 3 - head > 0 ? 3 - head : 0, pad_t = 6 - tail_add > 0 ? 6 - tail_add : 0;
      // the feature writer's rule: the stable stretch of the re-padded frame holds at least seven columns
      if (H + (end - start + 1) + T + pad_h + pad_t - head - tail_add >= kPrecMinStable) {
        w = 1u;
        const bool minus = cl.strand[c] != 0;
        const int64_t s = minus ? start - T + tail_add : start - H + head;
        const int64_t e = minus ? end + H - head : end + T - tail_add;
        const int64_t up[2] = {kPrecLong, kPrecShort}, down[2] = {kPrecShort, kPrecLong};
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          int64_t lo = s - 1 - up[k], hi = e + down[k];
          if (hi <= 0) {  // (Python would count a negative end from the chromosome's far end)
            set_stat(stat, kPrecStatBadWindow);
            hi = 0;
          }
          if (lo < 0) lo = 0;
          if (hi > len) hi = len;
          if (lo > hi) lo = hi;
          out[2 * k] = (uint32_t)lo;
          out[2 * k + 1] = (uint32_t)hi;
        }
      }
    }
  }
  written[j] = (uint8_t)w;
  flag32[j] = w;
#pragma unroll
  for (int k = 0; k < 4; ++k) win[4 * j + k] = out[k];
}

__global__ __launch_bounds__(kThreads) void precursor_compact_kernel(PrecGroups g, const uint32_t* __restrict__ rank,
                                                                    const uint32_t* __restrict__ win, uint32_t* __restrict__ rec_group,
                                                                    uint32_t* __restrict__ rec_lo, uint32_t* __restrict__ rec_hi,
                                                                    uint32_t* __restrict__ len32) {
  const uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (j > g.n_order) return;
  const uint64_t r = 2 * (uint64_t)rank[j];  // rank[j] <= j: records 2 rank[j] + 1 <= 2 n_order - 1
  if (j == g.n_order) {
    len32[r] = 0u;
    return;
  }
  if (rank[j + 1] == rank[j]) return;
  const uint32_t grp = g.order[j];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const uint32_t lo = win[4 * j + 2 * k], hi = win[4 * j + 2 * k + 1];
    rec_group[r + k] = grp;
    rec_lo[r + k] = lo;
    rec_hi[r + k] = hi;
    len32[r + k] = hi - lo;
  }
}

__global__ __launch_bounds__(kThreads) void precursor_check_kernel(PrecRecords r, PrecGroups g, PrecClusters cl, uint64_t seq_len,
                                                                  uint32_t* __restrict__ stat) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i > r.n) return;
  if (i == r.n) {
    if (r.off[0] != 0 || r.off[r.n] != seq_len) set_stat(stat, kPrecStatBadRecord);
    return;
  }
  const uint64_t a = r.off[i], b = r.off[i + 1];
  const uint32_t lo = r.lo[i], hi = r.hi[i], grp = r.group[i];
  if (a > b || b > seq_len || lo > hi || b - a != (uint64_t)(hi - lo)) set_stat(stat, kPrecStatBadRecord);
  if (grp >= g.n_groups) {
    set_stat(stat, kPrecStatBadGroup);
    return;
  }
  const uint32_t c = g.group_cluster[grp];
  if (c >= cl.n) {
    set_stat(stat, kPrecStatBadCluster);
    return;
  }
  const uint32_t entry = cl.entry[c];
  if (entry >= cl.n_entries) {
    set_stat(stat, kPrecStatBadEntry);
    return;
  }
  if (hi > cl.entry_len[entry]) set_stat(stat, kPrecStatBadRecord);
}

// the record whose bytes hold byte i: the last r < n with off[r] <= i (n >= 1, i < off[n])
__device__ __forceinline__ uint32_t record_of_byte(const uint64_t* __restrict__ off, uint32_t n, uint64_t i) {
  uint32_t lo = 0, hi = n;  // off[lo] <= i < off[hi]
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (off[mid] <= i) lo = mid;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kThreads) void precursor_bases_kernel(PrecRecords r, PrecGroups g, PrecClusters cl, PrecGenome genome,
                                                                  uint64_t seq_len, char* __restrict__ seq) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= seq_len) return;
  const uint32_t rec = record_of_byte(r.off, r.n, i);
  const uint64_t j = i - r.off[rec];
  const uint32_t lo = r.lo[rec], hi = r.hi[rec];
  if (j >= (uint64_t)(hi - lo)) return;  // (precursor_check_kernel ruled it out)
  const uint32_t c = g.group_cluster[r.group[rec]];
  const bool minus = cl.strand[c] != 0;
  const uint32_t entry = cl.entry[c];
  const uint32_t p = minus ? hi - 1u - (uint32_t)j : lo + (uint32_t)j;  // the base's offset in its entry
  // the entry's part: the last one that starts at or before it (constant indices: the table stays in scalar registers)
  const uint32_t* text = genome.part[0].text;
  const uint32_t* seg_start = genome.part[0].seg_start;
  const uint32_t* seg_off = genome.part[0].seg_off;
  const uint32_t* first_seg = genome.part[0].first_seg;
  uint32_t base = genome.part[0].entry_base, n_ref = genome.part[0].n_ref;
#pragma unroll
  for (uint32_t k = 1; k < kPrecMaxParts; ++k) {
    if (k < genome.n_parts && genome.part[k].entry_base <= entry) {
      text = genome.part[k].text;
      seg_start = genome.part[k].seg_start;
      seg_off = genome.part[k].seg_off;
      first_seg = genome.part[k].first_seg;
      base = genome.part[k].entry_base;
      n_ref = genome.part[k].n_ref;
    }
  }
  char ch = 'N';
  const uint32_t le = entry - base;
  if (entry >= base && le < n_ref) {
    const uint32_t s0 = first_seg[le];
    uint32_t a = s0, b = first_seg[le + 1];
    while (a < b) {  // the first segment of the entry that starts beyond p
      const uint32_t mid = a + (b - a) / 2;
      if (seg_off[mid] <= p) a = mid + 1;
      else b = mid;
    }
    if (a > s0) {
      const uint32_t s = a - 1u, in = p - seg_off[s], t0 = seg_start[s];
      if (in < seg_start[s + 1] - t0) {
        const uint32_t t = t0 + in;
        uint32_t code = (text[t >> 4] >> ((t & 15u) * 2u)) & 3u;
        if (minus) code = 3u - code;
        ch = (char)((0x55474341u >> (8u * code)) & 0xffu);  // "ACGU"
      }
    }
  }
  seq[i] = ch;
}

}  // namespace

hipError_t prec_windows_launch(const PrecGroups& g, const PrecClusters& cl, uint8_t* written, uint32_t* flag32, uint32_t* win, uint32_t* stat,
                               hipStream_t stream) {
  hipLaunchKernelGGL(precursor_windows_kernel, dim3(grid_for((uint64_t)g.n_order + 1)), dim3(kThreads), 0, stream, g, cl, written, flag32, win,
                     stat);
  return hipGetLastError();
}

hipError_t prec_compact_launch(const PrecGroups& g, const uint32_t* rank, const uint32_t* win, uint32_t* rec_group, uint32_t* rec_lo,
                               uint32_t* rec_hi, uint32_t* len32, hipStream_t stream) {
  hipLaunchKernelGGL(precursor_compact_kernel, dim3(grid_for((uint64_t)g.n_order + 1)), dim3(kThreads), 0, stream, g, rank, win, rec_group,
                     rec_lo, rec_hi, len32);
  return hipGetLastError();
}

hipError_t prec_check_launch(const PrecRecords& r, const PrecGroups& g, const PrecClusters& cl, uint64_t seq_len, uint32_t* stat,
                             hipStream_t stream) {
  hipLaunchKernelGGL(precursor_check_kernel, dim3(grid_for((uint64_t)r.n + 1)), dim3(kThreads), 0, stream, r, g, cl, seq_len, stat);
  return hipGetLastError();
}

hipError_t prec_bases_launch(const PrecRecords& r, const PrecGroups& g, const PrecClusters& cl, const PrecGenome& genome, uint64_t seq_len,
                             char* seq, hipStream_t stream) {
  if (seq_len == 0 || r.n == 0) return hipSuccess;
  hipLaunchKernelGGL(precursor_bases_kernel, dim3(grid_for(seq_len)), dim3(kThreads), 0, stream, r, g, cl, genome, seq_len, seq);
  return hipGetLastError();
}

}  // namespace mrg
