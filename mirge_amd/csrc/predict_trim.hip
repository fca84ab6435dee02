// Predict mode's preliminary trim on the device (mrg_predict_trim, include/mirge_amd.h): OriginalSeq of every location
// cluster, the flag and repeat element of preTrimClusteredSeq.py and the retained set of generate_Seq.py.  gfx950, wave64,
// no LDS, no atomics: one lane per output byte (trim_orig_kernel, trim_gather_kernel) or per cluster (trim_flags_kernel,
// trim_compact_kernel), every output word has one writer and nothing depends on lane order.  The stat words are the one
// exception to "one writer": every lane that finds an input array contradicting another stores the same 1 there.  The scans
// between the kernels are prims::exclusive_sum_u32 / _to_u64, called from capi.hip.
#include "predict_trim.hpp"

namespace mrg {

namespace {

constexpr uint32_t kThreads = 256;

inline uint32_t grid_for(uint64_t n) { return (uint32_t)((n + kThreads - 1) / kThreads); }

__device__ __forceinline__ void set_stat(uint32_t* __restrict__ stat, uint32_t word) { stat[word] = 1u; }

// the cluster whose bytes hold byte i: the last c < n with seq_off[c] <= i (n >= 1, i < seq_off[n])
__device__ __forceinline__ uint32_t cluster_of_byte(const uint64_t* __restrict__ seq_off, uint32_t n, uint64_t i) {
  uint32_t lo = 0, hi = n;  // seq_off[lo] <= i < seq_off[hi]
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (seq_off[mid] <= i) lo = mid;
    else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ char complement(char b) {
  return b == 'A' ? 'T' : b == 'T' ? 'A' : b == 'C' ? 'G' : b == 'G' ? 'C' : b;
}

__global__ __launch_bounds__(kThreads) void trim_orig_kernel(TrimClusters c, char* __restrict__ orig, uint32_t* __restrict__ stat) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= c.total_len) return;
  const uint32_t k = cluster_of_byte(c.seq_off, c.n, i);
  const uint64_t s = c.seq_off[k], e = c.seq_off[k + 1];
  if (s > i || e <= i || e > c.total_len) {  // (seq_off[0] != 0, not ascending, or past the buffer)
    set_stat(stat, kTrimStatBadSeqOff);
    orig[i] = 'N';
    return;
  }
  orig[i] = c.strand[k] ? complement(c.seq[s + (e - 1 - i)]) : c.seq[i];
}

// first element of [lo, hi) whose start is >= v
__device__ __forceinline__ uint32_t lower_bound(const uint32_t* __restrict__ start, uint32_t lo, uint32_t hi, uint32_t v) {
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (start[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ bool run_of(const char* __restrict__ p, char b) {
  bool all = true;
#pragma unroll
  for (uint32_t j = 0; j < kTrimRun; ++j) all = all && p[j] == b;
  return all;
}

__global__ __launch_bounds__(kThreads) void trim_flags_kernel(TrimClusters c, TrimRepeats r, const char* __restrict__ orig, uint32_t cutoff,
                                                              uint8_t* __restrict__ flag, int32_t* __restrict__ rep,
                                                              uint32_t* __restrict__ flag32, uint32_t* __restrict__ keep_len,
                                                              uint32_t* __restrict__ stat) {
  const uint32_t k = blockIdx.x * kThreads + threadIdx.x;  // (n + 1 lanes)
  if (k > c.n) return;
  if (k == c.n) {
    flag32[k] = 0;
    keep_len[k] = 0;
    return;
  }
  const uint64_t s = c.seq_off[k], e = c.seq_off[k + 1];
  uint32_t f = 0;
  int32_t name = -1;
  uint64_t len = 0;
  if (s > e || e > c.total_len) {
    set_stat(stat, kTrimStatBadSeqOff);
  } else {
    len = e - s;
    bool pass = len <= cutoff;
    if (pass && len >= kTrimRun) pass = !run_of(orig + (e - kTrimRun), 'A') && !run_of(orig + s, 'T');
    if (pass) {
      const uint32_t entry = c.entry[k];
      uint32_t r0 = 0, r1 = 0;
      if (entry >= r.n_entries) {
        set_stat(stat, kTrimStatBadEntry);
        pass = false;
      } else {
        r0 = r.off[entry];
        r1 = r.off[entry + 1];
        if (r0 > r1 || r1 > r.n_elements) {
          set_stat(stat, kTrimStatBadTable);
          pass = false;
          r0 = r1 = 0;
        }
      }
      if (r1 > r0) {
        const uint32_t cs = c.start[k], ce = c.end[k];
        // the elements in the order (start, index): [r0, p) start below cs, [p, r1) at or above it
        const uint32_t p = lower_bound(r.start, r0, r1, cs);
        // up to two candidates on each side, each side in the order of the rule: on the left the nearest start's run of
        // equal starts from its first element on, then the first element of the run before it
        constexpr uint32_t kNone = 0xffffffffu;
        uint32_t left[2] = {kNone, kNone}, right[2] = {kNone, kNone};
        if (p > r0) {
          const uint32_t a1 = lower_bound(r.start, r0, p, r.start[p - 1]);
          left[0] = a1;
          if (p - a1 >= 2) left[1] = a1 + 1;
          else if (a1 > r0) left[1] = lower_bound(r.start, r0, a1, r.start[a1 - 1]);
        }
        if (p < r1) right[0] = p;
        if (p + 1 < r1) right[1] = p + 1;
        // merge the two sides by distance; at equal distance the left side has the lower start
        uint32_t cand[2] = {kNone, kNone};
        uint32_t li = 0, ri = 0;
#pragma unroll
        for (uint32_t t = 0; t < 2; ++t) {
          const uint32_t l = li < 2 ? left[li] : kNone, g = ri < 2 ? right[ri] : kNone;
          bool take_left = false;
          if (l != kNone && g != kNone) take_left = (uint64_t)cs - r.start[l] <= (uint64_t)r.start[g] - cs;
          else take_left = l != kNone;
          if (take_left) {
            cand[t] = l;
            ++li;
          } else {
            cand[t] = g;  // (kNone when both sides are used up)
            ++ri;
          }
        }
#pragma unroll
        for (int t = 1; t >= 0; --t) {
          const uint32_t x = cand[t];
          if (x == kNone) continue;
          const uint32_t xs = r.start[x], xe = r.end[x];
          if (xe >= xs && cs <= ce && xs <= ce && xe >= cs) {
            pass = false;
            name = (int32_t)x;  // (t = 0 last: the nearer one's name stays)
          }
        }
      }
    }
    f = pass ? 1u : 0u;
  }
  flag[k] = (uint8_t)f;
  rep[k] = name;
  flag32[k] = f;
  keep_len[k] = f ? (uint32_t)len : 0u;
}

__global__ __launch_bounds__(kThreads) void trim_compact_kernel(uint32_t n, const uint32_t* __restrict__ rank,
                                                                const uint64_t* __restrict__ keep_off, uint32_t* __restrict__ kept,
                                                                uint64_t* __restrict__ kept_seq_off) {
  const uint32_t k = blockIdx.x * kThreads + threadIdx.x;  // (n + 1 lanes)
  if (k > n) return;
  const uint32_t at = rank[k];  // (<= rank[n] <= n: inside kept [n] for a retained k, inside kept_seq_off [n + 1] always)
  if (k == n) {
    kept_seq_off[at] = keep_off[k];
    return;
  }
  if (rank[k + 1] == at) return;
  kept[at] = k;
  kept_seq_off[at] = keep_off[k];
}

__global__ __launch_bounds__(kThreads) void trim_gather_kernel(TrimClusters c, const char* __restrict__ orig,
                                                               const uint32_t* __restrict__ rank, const uint64_t* __restrict__ keep_off,
                                                               char* __restrict__ kept_orig) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= c.total_len) return;
  const uint32_t k = cluster_of_byte(c.seq_off, c.n, i);
  if (rank[k + 1] == rank[k]) return;
  const uint64_t s = c.seq_off[k];
  // a retained cluster has s <= i < seq_off[k + 1] <= total_len (trim_flags_kernel checked its range), and the retained
  // bytes before it are at most the bytes before it: keep_off[k] <= s
  if (s > i) return;
  const uint64_t at = keep_off[k] + (i - s);
  if (at < c.total_len) kept_orig[at] = orig[i];
}

}  // namespace

hipError_t trim_orig_launch(const TrimClusters& c, char* orig, uint32_t* stat, hipStream_t stream) {
  if (c.total_len == 0 || c.n == 0) return hipSuccess;
  hipLaunchKernelGGL(trim_orig_kernel, dim3(grid_for(c.total_len)), dim3(kThreads), 0, stream, c, orig, stat);
  return hipGetLastError();
}

hipError_t trim_flags_launch(const TrimClusters& c, const TrimRepeats& r, const char* orig, uint32_t cutoff, uint8_t* flag, int32_t* rep,
                             uint32_t* flag32, uint32_t* keep_len, uint32_t* stat, hipStream_t stream) {
  hipLaunchKernelGGL(trim_flags_kernel, dim3(grid_for((uint64_t)c.n + 1)), dim3(kThreads), 0, stream, c, r, orig, cutoff, flag, rep, flag32,
                     keep_len, stat);
  return hipGetLastError();
}

hipError_t trim_compact_launch(uint32_t n, const uint32_t* rank, const uint64_t* keep_off, uint32_t* kept, uint64_t* kept_seq_off,
                               hipStream_t stream) {
  hipLaunchKernelGGL(trim_compact_kernel, dim3(grid_for((uint64_t)n + 1)), dim3(kThreads), 0, stream, n, rank, keep_off, kept, kept_seq_off);
  return hipGetLastError();
}

hipError_t trim_gather_launch(const TrimClusters& c, const char* orig, const uint32_t* rank, const uint64_t* keep_off, char* kept_orig,
                              hipStream_t stream) {
  if (c.total_len == 0 || c.n == 0) return hipSuccess;
  hipLaunchKernelGGL(trim_gather_kernel, dim3(grid_for(c.total_len)), dim3(kThreads), 0, stream, c, orig, rank, keep_off, kept_orig);
  return hipGetLastError();
}

}  // namespace mrg
