// Predict mode's cluster feature table on the device (mrg_predict_feature_groups / _align / _tally / _neighbors,
// include/mirge_amd.h; the rule: tests/predict_features_model.py).  gfx950, wave64, no LDS.
//
//   groups      one lane per row marks the start of a run of equal cluster, prims::exclusive_sum_u32 numbers the runs, one
//               wave per group sums its members' counts in 64 bits and applies the filter.  Nothing is compacted: a group
//               that fails keeps its slot with pass = 0 and its rows are skipped, so every array stays in file order.
//   align       32 lanes per row, column per lane, rows walked: a2i_align_kernel's tables U, Hg, E, F with three gap
//               shuffles, and a2i_settle_kernel's second walk where the best score ends in several cells.  The table loop
//               is restated here and not shared with a2i_align.hip.
//   tally       one wave per group; lane l owns frame columns l and l + 64 (at most 31 + 32 + 31 = 94), the wave walks the
//               members 64 at a time (one coalesced load, then lane broadcasts) and every lane adds the member's count to
//               the counter of the base it sees.  64-bit counters in registers, no atomics, no LDS.
//   neighbours  three stable prims::radix_sort_pairs_u64 passes order the groups by (chromosome rank, start, end, cluster
//               number); one lane per position finds its chromosome's range by bisection and its two distances.
//
// One writer per output word; the exceptions are the stat words and group_host, where every lane that has a reason stores
// the same 1, and the two counters, which are integer atomics whose sum does not depend on the order.
#include "predict_features.hpp"

#include <algorithm>

namespace mrg {

namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kPairsPerBlock = kBlock / 32, kWavesPerBlock = kBlock / 64;
constexpr uint64_t kEven = 0x5555555555555555ull;
constexpr int32_t kNeg = -1000;  // "no such path"; 32 rows of -1 keep it far below every score

inline uint32_t grid_for(uint64_t n) { return (uint32_t)((std::max<uint64_t>(n, 1) + kBlock - 1) / kBlock); }

// ------------------------------------------------------------------------------------------------ groups
__global__ __launch_bounds__(kBlock) void feat_mark_kernel(FeatRows rows, uint32_t n_reads, uint32_t n_clusters, uint32_t* __restrict__ flag32,
                                                           uint32_t* __restrict__ stat) {
  const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;  // (n_rows + 1 lanes)
  if (t > rows.n_rows) return;
  if (t == rows.n_rows) {
    flag32[t] = 0u;
    return;
  }
  const uint32_t c = rows.cluster[t];
  if (rows.read[t] >= n_reads || c >= n_clusters) stat[kFeatStatBadRow] = 1u;
  flag32[t] = (t == 0 || rows.cluster[t - 1] != c) ? 1u : 0u;
}

__global__ __launch_bounds__(kBlock) void feat_starts_kernel(FeatRows rows, const uint32_t* __restrict__ rank, uint32_t* __restrict__ row_group,
                                                             uint32_t* __restrict__ group_off, uint32_t* __restrict__ group_cluster) {
  const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (t >= rows.n_rows) return;
  const uint32_t before = rank[t], upto = rank[t + 1];  // (upto <= t + 1: the scan of 0 / 1 flags)
  if (upto == 0 || upto > t + 1) return;                // (row 0 always starts a group: a broken scan only)
  const uint32_t g = upto - 1;
  row_group[t] = g;
  if (upto != before) {
    group_off[g] = (uint32_t)t;
    group_cluster[g] = rows.cluster[t];
  }
  if (t + 1 == rows.n_rows) group_off[g + 1] = rows.n_rows;  // (g + 1 <= n_rows: inside group_off [n_rows + 1])
}

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
  for (int o = 32; o; o >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int32_t)(uint32_t)v, o, 64);
    const uint32_t hi = (uint32_t)__shfl_xor((int32_t)(uint32_t)(v >> 32), o, 64);
    v += ((uint64_t)hi << 32) | lo;
  }
  return v;
}

__device__ __forceinline__ int32_t wave_max(int32_t v) {
  for (int o = 32; o; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return v;
}

// what a group's cluster says, checked against the arrays: false (and a stat word) when they contradict each other
__device__ __forceinline__ bool cluster_facts(const FeatClusters& cl, uint32_t c, uint32_t n_entries, uint32_t* __restrict__ stat, uint32_t& len) {
  len = 0;
  if (c >= cl.n) {
    stat[kFeatStatBadGroups] = 1u;
    return false;
  }
  const uint64_t a = cl.seq_off[c], b = cl.seq_off[c + 1];
  const uint32_t s = cl.start[c], e = cl.end[c];
  if (b < a || b > cl.orig_len || cl.entry[c] >= n_entries || e < s || (uint64_t)e - s + 1 != b - a) {
    stat[kFeatStatBadCluster] = 1u;
    return false;
  }
  len = (uint32_t)(b - a);
  return true;
}

__global__ __launch_bounds__(kBlock) void feat_filter_kernel(uint32_t n_groups, const uint32_t* __restrict__ group_off,
                                                             const uint32_t* __restrict__ group_cluster, FeatRows rows, FeatReads reads,
                                                             FeatClusters cl, uint32_t n_entries, const uint32_t* __restrict__ entry_len,
                                                             uint64_t* __restrict__ group_sum, uint8_t* __restrict__ group_pass,
                                                             uint32_t* __restrict__ stat) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t g = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (g >= n_groups) return;  // (the whole wave)
  uint32_t lo = group_off[g], hi = group_off[g + 1];
  if (lo >= hi || hi > rows.n_rows) {
    stat[kFeatStatBadGroups] = 1u;
    lo = hi = 0;
  }
  uint64_t sum = 0;
  for (uint32_t t = lo + lane; t < hi; t += 64u) {
    const uint32_t r = rows.read[t];
    if (r < reads.n) sum += reads.counts[r];
    else stat[kFeatStatBadRow] = 1u;
  }
  sum = wave_sum_u64(sum);
  if (lane != 0u) return;
  const uint32_t c = group_cluster[g];
  uint32_t len;
  bool pass = cluster_facts(cl, c, n_entries, stat, len);
  if (pass) {
    const uint64_t chr_len = entry_len[cl.entry[c]];
    pass = sum >= kFeatMinCount && hi - lo >= kFeatMinMembers && cl.start[c] > kFeatTerminal && (uint64_t)cl.end[c] + kFeatTerminal < chr_len;
  }
  group_sum[g] = sum;
  group_pass[g] = pass ? 1 : 0;
  if (pass) atomicAdd(&stat[kFeatStatPassed], 1u);
}

// ------------------------------------------------------------------------------------------------ packing
__global__ __launch_bounds__(kBlock) void feat_pack_kernel(FeatClusters cl, uint64_t* __restrict__ cl_word, uint8_t* __restrict__ cl_len,
                                                           uint32_t* __restrict__ stat) {
  const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
  if (c >= cl.n) return;
  const uint64_t a = cl.seq_off[c], b = cl.seq_off[c + 1];
  uint64_t word = 0;
  uint32_t len = 255u;
  if (b < a || b > cl.orig_len) {
    stat[kFeatStatBadCluster] = 1u;
  } else if (b - a >= 1 && b - a <= 32) {
    len = (uint32_t)(b - a);
    for (uint32_t i = 0; i < len; ++i) {
      const char ch = cl.orig[a + i];
      const uint32_t code = ch == 'A' ? 0u : ch == 'C' ? 1u : ch == 'G' ? 2u : ch == 'T' ? 3u : 4u;
      if (code > 3u) {
        len = 255u;
        word = 0;
        break;
      }
      word |= (uint64_t)code << (2u * i);
    }
  }
  cl_word[c] = word;
  cl_len[c] = (uint8_t)len;
}

// ------------------------------------------------------------------------------------------------ row alignment
// the even bits of x, squeezed together
__device__ __forceinline__ uint32_t squeeze_even(uint64_t x) {
  x &= kEven;
  x = (x | (x >> 1)) & 0x3333333333333333ull;
  x = (x | (x >> 2)) & 0x0F0F0F0F0F0F0F0Full;
  x = (x | (x >> 4)) & 0x00FF00FF00FF00FFull;
  x = (x | (x >> 8)) & 0x0000FFFF0000FFFFull;
  x = (x | (x >> 16)) & 0x00000000FFFFFFFFull;
  return (uint32_t)x;
}

// bits [a, b) of a 32-bit word, a and b anywhere
__device__ __forceinline__ uint32_t bit_range(int32_t a, int32_t b) {
  const int32_t lo = min(max(a, 0), 32), hi = min(max(b, 0), 32);
  if (hi <= lo) return 0u;
  const uint32_t upto = hi == 32 ? 0xFFFFFFFFu : (1u << hi) - 1u;
  return upto & ~((1u << lo) - 1u);
}

__device__ __forceinline__ int32_t up(int32_t v, uint32_t k, uint32_t lane, int32_t edge) {
  const int32_t got = __shfl_up(v, k, 32);
  return lane < k ? edge : got;
}

__device__ __forceinline__ int32_t group_max(int32_t v) {
  for (int o = 16; o; o >>= 1) v = max(v, __shfl_xor(v, o, 32));
  return v;
}

__device__ __forceinline__ int32_t group_sum(int32_t v) {
  for (int o = 16; o; o >>= 1) v += __shfl_xor(v, o, 32);
  return v;
}

__global__ __launch_bounds__(kBlock) void feat_align_kernel(const FeatAlignArgs a) {
  const uint32_t lane = threadIdx.x & 31u;
  const uint32_t half = threadIdx.x & 32u;  // where this row's lanes sit in the wave's ballot
  const uint32_t wanted = blockIdx.x * kPairsPerBlock + (threadIdx.x >> 5);
  const uint32_t t = min(wanted, a.rows.n_rows - 1u);  // (a group of lanes past the end repeats the last row and stores nothing)
  const uint32_t read = a.rows.read[t], cluster = a.rows.cluster[t], group = a.row_group[t];
  const bool known = read < a.reads.n && cluster < a.n_clusters && group < a.n_groups;
  const bool pass = known && a.group_pass[group] != 0;
  const int32_t lb = known ? (int32_t)a.reads.lens[read] : 0;
  const int32_t la = known ? (int32_t)a.cl_len[cluster] : 255;
  const bool usable = pass && la >= 1 && la <= 32 && lb >= 1 && lb <= 32;
  const uint64_t keep = lb >= 32 ? ~0ull : (1ull << (2 * max(lb, 0))) - 1ull;
  const uint64_t tw = usable ? a.cl_word[cluster] : 0ull;
  const uint64_t rn = (usable && a.reads.nmask) ? (a.reads.nmask[read] & kEven & keep) : 0ull;
  const uint64_t rw = usable ? (a.reads.words[read] & ~(rn * 3ull) & keep) : 0ull;

  // ---- the score tables, row by row; this lane is column `lane`
  const bool col = (int32_t)lane < lb;
  const uint32_t my_base = (uint32_t)(rw >> (2u * lane)) & 3u;
  const bool my_n = ((rn >> (2u * lane)) & 1ull) != 0ull || !col;
  int32_t U = 0, X = kNeg, H1 = kNeg, H2 = kNeg, H3 = kNeg;
  int32_t best = 0, cnt = 0, r_best = 0, g = kNeg;
  for (int32_t r = 0; r < 32; ++r) {
    const uint32_t t_base = (uint32_t)(tw >> (2u * r)) & 3u;
    const int32_t s = (!my_n && t_base == my_base) ? 2 : -1;
    const int32_t Un = max(0, up(U, 1u, lane, 0) + s);
    const int32_t Hg = up(X, 1u, lane, kNeg) + s;
    const int32_t H = max(Un, Hg);
    const int32_t E = max(max(up(H, 1u, lane, kNeg) - 20, up(H, 2u, lane, kNeg) - 40), up(H, 3u, lane, kNeg) - 60);
    const int32_t F = max(max(H1 - 20, H2 - 40), H3 - 60);
    if (col && r < la) {
      if (Un > best) {
        best = Un;
        cnt = 1;
        r_best = r;
      } else if (Un == best) {
        ++cnt;
      }
      g = max(g, Hg);
    }
    X = max(max(Hg, E), max(F, kNeg));
    H3 = H2;
    H2 = H1;
    H1 = H;
    U = Un;
  }
  const int32_t m = group_max(best);
  const int32_t ends = group_sum(best == m ? cnt : 0);
  const int32_t gmax = group_max(g);
  int32_t diag = group_sum((best == m && ends == 1) ? r_best - (int32_t)lane : 0);

  // ---- several best cells: the diagonal pairwise2 lists first (a2i_settle_kernel's rule).  The branch is the same for
  // the whole wave, so every lane takes part in the shuffles and ballots inside.
  const bool tied = usable && m > 0 && ends > 1 && gmax < m;
  int32_t key = -1;
  if (__any(tied)) {
    int32_t UT = 0;  // U << 1 | "this run already holds a top"
    uint32_t tops = 0u, elig = 0u;
    for (int32_t r = 0; r < 32; ++r) {
      const uint32_t t_base = (uint32_t)(tw >> (2u * r)) & 3u;
      const int32_t s = (!my_n && t_base == my_base) ? 2 : -1;
      const int32_t ul = up(UT, 1u, lane, 0);
      const int32_t Un = max(0, (ul >> 1) + s);
      const bool top = Un == m;
      if (col && r < la && top) {
        tops |= 1u << r;
        if (!(ul & 1)) elig |= 1u << r;
      }
      UT = (Un << 1) | ((Un > 0 && ((ul & 1) || top)) ? 1 : 0);
    }
    const uint32_t last_col = (uint32_t)__shfl((int32_t)tops, min(max(lb - 1, 0), 31), 32);
    const uint32_t prev_col = lb >= 2 ? (uint32_t)__shfl((int32_t)tops, min(max(lb - 2, 0), 31), 32) : 0u;
    int32_t row_cut = 32;
    if (last_col) {
      const uint32_t from = prev_col & ~((1u << (__ffs(last_col) - 1)) - 1u);
      if (from) row_cut = __ffs(from);
    }
    const int32_t la_bit = min(max(la - 1, 0), 31), la_bit2 = min(max(la - 2, 0), 31);
    const uint32_t last_row = (uint32_t)(__ballot(la >= 1 && ((tops >> la_bit) & 1u)) >> half);
    const uint32_t prev_row = (uint32_t)(__ballot(la >= 2 && ((tops >> la_bit2) & 1u)) >> half);
    uint32_t lane_cut = 32u;
    if (last_row) {
      const uint32_t from = (prev_row << 1) & ~((2u << (__ffs(last_row) - 1)) - 1u) & bit_range(0, lb);
      if (from) lane_cut = (uint32_t)__ffs(from) - 1u;
    }
    uint32_t e = elig & bit_range(0, row_cut + 1);
    if (lane > lane_cut) e &= ~(1u << la_bit);
    key = group_max(e ? (((31 - __clz(e)) << 6) | (int32_t)lane) : -1);  // the largest (row, column)
  }

  uint32_t status;
  if (!pass) status = kFeatRowSkipped;
  else if (!usable) status = kFeatRowUnsupported;
  else if (rn != 0ull) status = kFeatRowN;
  else if (m <= 0) status = kFeatRowNoScore;
  else if (gmax >= m) status = kFeatRowGapped;
  else if (ends == 1) status = kFeatRowSimple;
  else if (key >= 0) {
    status = kFeatRowTied;
    diag = (key >> 6) - (key & 63);
  } else status = kFeatRowUnsettled;

  uint32_t ident = 0u;
  if (status > kFeatRowTied) {
    diag = 0;
  } else {
    const uint64_t rs = diag >= 0 ? rw << (2 * diag) : rw >> (2 * -diag);  // (|diag| <= 31)
    const uint64_t x = tw ^ rs;
    ident = (uint32_t)__popc(~squeeze_even(x | (x >> 1)) & bit_range(max(0, diag), min(la, diag + lb)));
  }
  if (lane == 0u && wanted < a.rows.n_rows) {
    a.row_status[t] = (uint8_t)status;
    a.row_diag[t] = diag;
    a.row_ident[t] = (uint8_t)ident;
    if (status >= kFeatRowHost) a.group_host[group] = 1;  // (group < n_groups: pass implies known)
  }
}

// ------------------------------------------------------------------------------------------------ column tally
__device__ __forceinline__ uint64_t lane_value_u64(uint64_t v, uint32_t j) {
  const uint32_t lo = (uint32_t)__shfl((int32_t)(uint32_t)v, (int32_t)j, 64);
  const uint32_t hi = (uint32_t)__shfl((int32_t)(uint32_t)(v >> 32), (int32_t)j, 64);
  return ((uint64_t)hi << 32) | lo;
}

__global__ __launch_bounds__(kBlock) void feat_tally_kernel(const FeatTallyArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t g = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  if (g >= a.n_groups) return;  // (the whole wave)
  const uint32_t lo = a.group_off[g], hi = a.group_off[g + 1], c = a.group_cluster[g];
  const bool sane = lo < hi && hi <= a.rows.n_rows && c < a.n_clusters;
  const int32_t la = sane ? (int32_t)a.cl_len[c] : 255;
  const bool mine = sane && a.group_pass[g] && !a.group_host[g] && la >= 1 && la <= 32;
  uint64_t* const nine = a.nine + (uint64_t)g * kFeatNineWords;
  int32_t* const frame = a.frame + (uint64_t)g * 4u;
  if (!mine) {  // (the same for the whole wave)
    if (lane < kFeatNineWords) nine[lane] = 0ull;
    if (lane < 4u) frame[lane] = 0;
    if (lane == 0u) {
      a.valid[g] = 0;
      a.exact[g] = 0ull;
    }
    return;
  }
  // ---- the frame: H dashes before the cluster, T behind it
  int32_t H = 0, T = 0;
  for (uint32_t base = lo; base < hi; base += 64u) {
    const uint32_t t = base + lane;
    if (t < hi) {
      const uint32_t r = a.rows.read[t];
      const int32_t lb = r < a.reads.n ? min((int32_t)a.reads.lens[r], 32) : 0;
      const int32_t d = min(max(a.row_diag[t], -31), 31);
      H = max(H, -d);
      T = max(T, d + lb - la);
    }
  }
  H = min(wave_max(H), 31);
  T = min(max(wave_max(T), 0), 31);
  const int32_t ncols = H + la + T;  // (<= 94: two columns per lane cover it)

  // ---- the walk: 64 members per load, then one broadcast per member
  uint64_t a0 = 0, c0 = 0, g0 = 0, t0 = 0, a1 = 0, c1 = 0, g1 = 0, t1 = 0, total = 0, exact = 0;
  for (uint32_t base = lo; base < hi; base += 64u) {
    const uint32_t t = base + lane;
    uint64_t my_w = 0;
    uint32_t my_cnt = 0;
    int32_t my_d = 0, my_lb = 0, my_exact = 0;
    if (t < hi) {
      const uint32_t r = a.rows.read[t];
      if (r < a.reads.n) {
        my_lb = min((int32_t)a.reads.lens[r], 32);
        my_w = a.reads.words[r];
        my_cnt = a.reads.counts[r];
        my_exact = (int32_t)a.row_ident[t] == my_lb ? 1 : 0;
      }
      my_d = min(max(a.row_diag[t], -31), 31);
    }
    const uint32_t n = min(64u, hi - base);
    for (uint32_t j = 0; j < n; ++j) {
      const uint64_t w = lane_value_u64(my_w, j);
      const uint64_t cnt = (uint32_t)__shfl((int32_t)my_cnt, (int32_t)j, 64);
      const int32_t d = __shfl(my_d, (int32_t)j, 64), lb = __shfl(my_lb, (int32_t)j, 64);
      total += cnt;
      exact += __shfl(my_exact, (int32_t)j, 64) ? cnt : 0ull;
      const int32_t i0 = (int32_t)lane - H - d, i1 = i0 + 64;
      const uint32_t b0 = (uint32_t)(w >> (2u * ((uint32_t)i0 & 31u))) & 3u;
      const uint32_t b1 = (uint32_t)(w >> (2u * ((uint32_t)i1 & 31u))) & 3u;
      const uint64_t v0 = (i0 >= 0 && i0 < lb) ? cnt : 0ull, v1 = (i1 >= 0 && i1 < lb) ? cnt : 0ull;
      a0 += b0 == 0u ? v0 : 0ull;
      c0 += b0 == 1u ? v0 : 0ull;
      g0 += b0 == 2u ? v0 : 0ull;
      t0 += b0 == 3u ? v0 : 0ull;
      a1 += b1 == 0u ? v1 : 0ull;
      c1 += b1 == 1u ? v1 : 0ull;
      g1 += b1 == 2u ? v1 : 0ull;
      t1 += b1 == 3u ? v1 : 0ull;
    }
  }

  // ---- per column: the majority count (the base itself plays no part in what follows) and 5 c >= 4 total
  const uint64_t m0 = max(max(a0, c0), max(g0, t0)), m1 = max(max(a1, c1), max(g1, t1));
  const uint64_t need = 4ull * total;
  const uint64_t s0 = __ballot((int32_t)lane < ncols && 5ull * m0 >= need);
  const uint64_t s1 = __ballot((int32_t)lane + 64 < ncols && 5ull * m1 >= need);
  const bool any = (s0 | s1) != 0ull;
  int32_t head = 0, tail = 0;
  if (any) {
    head = s0 ? __ffsll((unsigned long long)s0) - 1 : 64 + __ffsll((unsigned long long)s1) - 1;
    const int32_t last = s1 ? 64 + 63 - __clzll((long long)s1) : 63 - __clzll((long long)s0);
    tail = last - ncols;
  }
  if (lane == 0u) {
    frame[0] = H;
    frame[1] = T;
    frame[2] = head;
    frame[3] = tail;
    a.valid[g] = any ? 1 : 0;
    a.exact[g] = exact;
  }
  if (!any) {
    if (lane < kFeatNineWords) nine[lane] = 0ull;
    return;
  }
  // ---- the nine feature columns of the re-padded frame, as columns of this one: a column outside it is padding
  const int32_t tail_add = -tail - 1;
  const int32_t pad_t = max(0, 6 - tail_add);
  const int32_t tp = pad_t == 0 ? tail : -6;
#pragma unroll
  for (int32_t k = 0; k < (int32_t)kFeatNine; ++k) {
    const int32_t x = k < 3 ? head - 3 + k : ncols + pad_t + tp + (k - 3);
    const bool inside = x >= 0 && x < ncols;
    const uint32_t owner = inside ? (uint32_t)x & 63u : 0u;
    if (lane == owner) {
      const bool second = inside && x >= 64;
      const uint64_t A = inside ? (second ? a1 : a0) : 0ull, C = inside ? (second ? c1 : c0) : 0ull;
      const uint64_t G = inside ? (second ? g1 : g0) : 0ull, Tt = inside ? (second ? t1 : t0) : 0ull;
      uint64_t* out = nine + 5 * k;
      out[0] = A;
      out[1] = Tt;
      out[2] = C;
      out[3] = G;
      out[4] = total - (A + C + G + Tt);
    }
  }
}

// ------------------------------------------------------------------------------------------------ neighbours
// the decimal digits of v (< 10^10) from bit 39 down, four bits each, the rest filled with 15 (predict_remap.hpp: the byte
// order of `<digits>_`)
__device__ __forceinline__ uint64_t digits_key(uint64_t v) {
  uint32_t d = 1;
  for (uint64_t p = 10; d < 10 && v >= p; p *= 10) ++d;
  uint64_t key = d < 10 ? (1ull << (4u * (10u - d))) - 1ull : 0ull;
  for (uint32_t at = 10u - d; at < 10u; ++at) {
    key |= (v % 10) << (4u * at);
    v /= 10;
  }
  return key;
}

__global__ __launch_bounds__(kBlock) void feat_keys_kernel(FeatNeighborArgs a, uint64_t* __restrict__ key_c, uint64_t* __restrict__ key_se,
                                                           uint64_t* __restrict__ key_r, uint32_t* __restrict__ vals,
                                                           uint32_t* __restrict__ stat) {
  const uint32_t g = blockIdx.x * kBlock + threadIdx.x;
  if (g >= a.n_groups) return;
  const uint32_t c = a.group_cluster[g];
  uint64_t kc = 0, kse = 0, kr = kFeatNoRank;
  if (c >= a.cl.n) {
    stat[kFeatStatBadGroups] = 1u;
  } else {
    kc = digits_key((uint64_t)a.cl.kept[c] + 1ull);
    kse = ((uint64_t)a.cl.start[c] << 32) | a.cl.end[c];
    if (a.valid[g]) {
      const uint32_t e = a.cl.entry[c];
      if (e >= a.n_entries) stat[kFeatStatBadCluster] = 1u;
      else kr = min(a.entry_rank[e], kFeatNoRank - 1u);
    }
  }
  key_c[g] = kc;
  key_se[g] = kse;
  key_r[g] = kr;
  vals[g] = g;
}

__global__ __launch_bounds__(kBlock) void feat_gather_keys_kernel(const uint64_t* __restrict__ in, const uint32_t* __restrict__ vals, uint32_t n,
                                                                  uint64_t* __restrict__ out) {
  const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
  if (j >= n) return;
  const uint32_t v = vals[j];
  out[j] = v < n ? in[v] : 0ull;
}

// the first index of keys [0, n) whose low 32 bits are >= r
__device__ __forceinline__ uint32_t first_at_least(const uint64_t* __restrict__ keys, uint32_t n, uint64_t r) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if ((keys[mid] & 0xffffffffull) < r) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

struct Interval {
  int64_t s, e;
  uint32_t strand;
};

__device__ __forceinline__ Interval interval_of(const FeatNeighborArgs& a, uint32_t g) {
  const uint32_t c = min(a.group_cluster[g], a.cl.n - 1u);
  const int32_t* f = a.frame + (uint64_t)g * 4u;
  Interval iv;
  iv.s = (int64_t)a.cl.start[c] + f[2] - f[0];
  iv.e = (int64_t)a.cl.end[c] + 1 + f[3] + f[1];
  iv.strand = a.cl.strand[c] ? 1u : 0u;
  return iv;
}

__global__ __launch_bounds__(kBlock) void feat_neighbors_kernel(FeatNeighborArgs a, const uint64_t* __restrict__ sorted_rank,
                                                                const uint32_t* __restrict__ order, uint32_t* __restrict__ nb_t,
                                                                int64_t* __restrict__ nb_up, int64_t* __restrict__ nb_down,
                                                                uint8_t* __restrict__ nb_flags, uint32_t* __restrict__ stat) {
  const uint32_t j = blockIdx.x * kBlock + threadIdx.x;
  const uint32_t n = a.n_groups;
  if (j == 0u) stat[kFeatStatSorted] = first_at_least(sorted_rank, n, kFeatNoRank);
  if (j >= n) return;
  const uint64_t r = sorted_rank[j] & 0xffffffffull;
  const uint32_t g = order[j];
  if (r == kFeatNoRank || g >= n) return;
  const uint32_t first = first_at_least(sorted_rank, n, r), end = first_at_least(sorted_rank, n, r + 1);
  const Interval me = interval_of(a, g);
  int64_t up_d = 0, down_d = 0;
  bool has_up = false, has_down = false, good = false;
  if (j > first) {
    const uint32_t p = order[j - 1];
    if (p < n) {
      const Interval o = interval_of(a, p);
      has_up = true;
      up_d = me.s - o.e - 1;
      good = good || (up_d >= 9 && up_d <= 44 && o.strand == me.strand);
    }
  }
  if (j + 1 < end) {
    const uint32_t q = order[j + 1];
    if (q < n) {
      const Interval o = interval_of(a, q);
      has_down = true;
      down_d = o.s - me.e - 1;
      good = good || (down_d >= 9 && down_d <= 44 && o.strand == me.strand);
    }
  }
  uint32_t state = 0u;  // Null: alone on its chromosome, or every neighbour beyond 44
  if (has_up || has_down) {
    const bool far = (!has_up || up_d > 44) && (!has_down || down_d > 44);
    state = good ? 1u : far ? 0u : 2u;
  }
  nb_t[g] = j - first;
  nb_up[g] = up_d;
  nb_down[g] = down_d;
  nb_flags[g] = (uint8_t)((has_up ? 0u : kFeatNoUp) | (has_down ? 0u : kFeatNoDown) | (state << kFeatStateShift));
}

}  // namespace

hipError_t feat_mark_launch(const FeatRows& rows, uint32_t n_reads, uint32_t n_clusters, uint32_t* flag32, uint32_t* stat, hipStream_t stream) {
  hipLaunchKernelGGL(feat_mark_kernel, dim3(grid_for((uint64_t)rows.n_rows + 1)), dim3(kBlock), 0, stream, rows, n_reads, n_clusters, flag32, stat);
  return hipGetLastError();
}

hipError_t feat_starts_launch(const FeatRows& rows, const uint32_t* rank, uint32_t* row_group, uint32_t* group_off, uint32_t* group_cluster,
                              hipStream_t stream) {
  if (rows.n_rows == 0) return hipSuccess;
  hipLaunchKernelGGL(feat_starts_kernel, dim3(grid_for(rows.n_rows)), dim3(kBlock), 0, stream, rows, rank, row_group, group_off, group_cluster);
  return hipGetLastError();
}

hipError_t feat_filter_launch(uint32_t n_groups, const uint32_t* group_off, const uint32_t* group_cluster, const FeatRows& rows,
                              const FeatReads& reads, const FeatClusters& cl, uint32_t n_entries, const uint32_t* entry_len,
                              uint64_t* group_sum, uint8_t* group_pass, uint32_t* stat, hipStream_t stream) {
  if (n_groups == 0) return hipSuccess;
  hipLaunchKernelGGL(feat_filter_kernel, dim3((n_groups + kWavesPerBlock - 1) / kWavesPerBlock), dim3(kBlock), 0, stream, n_groups, group_off,
                     group_cluster, rows, reads, cl, n_entries, entry_len, group_sum, group_pass, stat);
  return hipGetLastError();
}

hipError_t feat_pack_launch(const FeatClusters& cl, uint64_t* cl_word, uint8_t* cl_len, uint32_t* stat, hipStream_t stream) {
  if (cl.n == 0) return hipSuccess;
  hipLaunchKernelGGL(feat_pack_kernel, dim3(grid_for(cl.n)), dim3(kBlock), 0, stream, cl, cl_word, cl_len, stat);
  return hipGetLastError();
}

hipError_t feat_align_launch(const FeatAlignArgs& a, hipStream_t stream) {
  if (a.rows.n_rows == 0) return hipSuccess;
  hipLaunchKernelGGL(feat_align_kernel, dim3((a.rows.n_rows + kPairsPerBlock - 1) / kPairsPerBlock), dim3(kBlock), 0, stream, a);
  return hipGetLastError();
}

hipError_t feat_tally_launch(const FeatTallyArgs& a, hipStream_t stream) {
  if (a.n_groups == 0) return hipSuccess;
  hipLaunchKernelGGL(feat_tally_kernel, dim3((a.n_groups + kWavesPerBlock - 1) / kWavesPerBlock), dim3(kBlock), 0, stream, a);
  return hipGetLastError();
}

hipError_t feat_keys_launch(const FeatNeighborArgs& a, uint64_t* key_c, uint64_t* key_se, uint64_t* key_r, uint32_t* vals, uint32_t* stat,
                            hipStream_t stream) {
  if (a.n_groups == 0) return hipSuccess;
  hipLaunchKernelGGL(feat_keys_kernel, dim3(grid_for(a.n_groups)), dim3(kBlock), 0, stream, a, key_c, key_se, key_r, vals, stat);
  return hipGetLastError();
}

hipError_t feat_gather_keys_launch(const uint64_t* in, const uint32_t* vals, uint32_t n, uint64_t* out, hipStream_t stream) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(feat_gather_keys_kernel, dim3(grid_for(n)), dim3(kBlock), 0, stream, in, vals, n, out);
  return hipGetLastError();
}

hipError_t feat_neighbors_launch(const FeatNeighborArgs& a, const uint64_t* sorted_rank, const uint32_t* order, uint32_t* nb_t, int64_t* nb_up,
                                 int64_t* nb_down, uint8_t* nb_flags, uint32_t* stat, hipStream_t stream) {
  if (a.n_groups == 0) return hipSuccess;
  hipLaunchKernelGGL(feat_neighbors_kernel, dim3(grid_for(a.n_groups)), dim3(kBlock), 0, stream, a, sorted_rank, order, nb_t, nb_up, nb_down,
                     nb_flags, stat);
  return hipGetLastError();
}

}  // namespace mrg
