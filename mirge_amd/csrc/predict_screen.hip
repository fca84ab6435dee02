// Predict mode's screening of the folded precursor candidates on the device (mrg_predict_screen_candidates / _prune /
// _features / _select, include/mirge_amd.h).  gfx950, wave64, no atomics, no scratch.
//
// screen_candidates_kernel and screen_select_kernel take one lane per feature line.  screen_prune_kernel and
// screen_features_kernel take one wave per candidate, four waves a workgroup, four characters a lane: the candidate's
// sequence and structure (at most 256 characters), the depth after every character, the pair table and the one or two
// miRNAs live in the wave's 2 KiB of LDS.  The depth is a prefix sum -- four characters in the lane (one aligned dword of the
// structure), then a shuffle scan over the 64 lane sums.  The partner of a `(` at depth d is the first later position of
// depth d - 1: every lane walks forward from its own brackets, so the table costs one pass over LDS per bracket, no stack.
// A wave reads what other lanes of it wrote only behind a __syncthreads(); the four waves of a workgroup run the same
// phases (a wave without a candidate runs them with every lane idle), so the barriers are uniform.
// Every output word has one writer.  The stat words are the exception: every lane that finds what a word names stores the
// same 1 there.
#include "predict_screen.hpp"

#include <limits.h>

namespace mrg {

namespace {

constexpr uint32_t kThreads = 256, kWaves = kThreads / 64;
static_assert(kScreenMaxLen == 256, "four characters a lane");

inline uint32_t grid_for(uint64_t n) { return (uint32_t)((n + kThreads - 1) / kThreads); }
inline uint32_t wave_grid_for(uint64_t n) { return (uint32_t)((n + kWaves - 1) / kWaves); }

__device__ __forceinline__ void set_stat(uint32_t* __restrict__ stat, uint32_t word) { stat[word] = 1u; }

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v = min(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v = max(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

__global__ __launch_bounds__(kThreads) void screen_candidates_kernel(uint32_t n_lines, const uint32_t* __restrict__ line_group, uint32_t n_groups,
                                                                     const uint8_t* __restrict__ nb_flags, const int64_t* __restrict__ nb_up,
                                                                     const int64_t* __restrict__ nb_down, uint8_t* __restrict__ cand_n,
                                                                     uint32_t* __restrict__ cand_rec, uint32_t* __restrict__ cand_mir,
                                                                     uint32_t* __restrict__ stat) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n_lines) return;
  const uint32_t line = (uint32_t)i, g = line_group[i];
  uint32_t n = 0, rec[4] = {kScreenNoIndex, kScreenNoIndex, kScreenNoIndex, kScreenNoIndex};
  uint32_t other[4] = {kScreenNoIndex, kScreenNoIndex, kScreenNoIndex, kScreenNoIndex};
  if (g >= n_groups) {
    set_stat(stat, kScreenStatBadGroup);
  } else {
    const uint32_t flags = nb_flags[g];
    const int64_t up = (flags & 1u) ? kScreenNoNeighbour : nb_up[g], down = (flags & 2u) ? kScreenNoNeighbour : nb_down[g];
    const bool near_up = up >= kScreenClosest && up <= kScreenFarthest, near_down = down >= kScreenClosest && down <= kScreenFarthest;
    if (((flags >> 2) & 3u) != 1u) {  // not Good: the line's own two, its own miRNA
      n = 2;
      rec[0] = 2 * line;
      rec[1] = 2 * line + 1;
    } else if ((near_up && line == 0) || (near_down && line + 1 == n_lines) || !(near_up || near_down)) {
      set_stat(stat, kScreenStatBadLine);
    } else if (!near_up) {
      n = 2;
      rec[0] = 2 * line + 1;
      rec[1] = 2 * line + 2;
      other[0] = other[1] = line + 1;
    } else if (near_down) {
      n = 4;
      rec[0] = 2 * line - 1;
      rec[1] = 2 * line;
      rec[2] = 2 * line + 1;
      rec[3] = 2 * line + 2;
      other[0] = other[1] = line - 1;
      other[2] = other[3] = line + 1;
    } else {
      n = 2;
      rec[0] = 2 * line - 1;
      rec[1] = 2 * line;
      other[0] = other[1] = line - 1;
    }
  }
  cand_n[i] = (uint8_t)n;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    cand_rec[4 * i + k] = rec[k];
    cand_mir[8 * i + 2 * k] = rec[k] == kScreenNoIndex ? kScreenNoIndex : line;
    cand_mir[8 * i + 2 * k + 1] = other[k];
  }
}

__global__ __launch_bounds__(kThreads) void screen_check_offsets_kernel(ScreenBlob b, uint32_t* __restrict__ stat) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i > b.n) return;
  const uint64_t a = b.off[i];
  if (i == 0 && a != 0) set_stat(stat, kScreenStatBadOffsets);
  if (i == b.n) {
    if (a != b.len) set_stat(stat, kScreenStatBadOffsets);
  } else if (a > b.off[i + 1] || b.off[i + 1] > b.len) {
    set_stat(stat, kScreenStatBadOffsets);
  }
}

__global__ __launch_bounds__(kThreads) void screen_check_cands_kernel(uint32_t n_cand, const uint32_t* __restrict__ cand_rec,
                                                                      const uint8_t* __restrict__ status,
                                                                      const uint32_t* __restrict__ cand_mir, uint32_t n_rec, uint32_t n_mir,
                                                                      uint32_t* __restrict__ stat) {
  const uint64_t c = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (c >= n_cand) return;
  if (status && status[c] != kScreenOk) return;
  if (cand_rec) {
    const uint32_t r = cand_rec[c];
    if (r == kScreenNoIndex) return;
    if (r >= n_rec) set_stat(stat, kScreenStatBadCand);
  }
  const uint32_t m0 = cand_mir[2 * c], m1 = cand_mir[2 * c + 1];
  if (m0 >= n_mir || (m1 != kScreenNoIndex && m1 >= n_mir)) set_stat(stat, kScreenStatBadCand);
}

// ---------------------------------------------------------------------------------------------- one wave per candidate
struct alignas(16) WaveLds {
  char seq[kScreenMaxLen];
  char str[kScreenMaxLen];
  int16_t depth[kScreenMaxLen];
  int16_t pt[kScreenMaxLen];
  char mir[2][kScreenMaxLen];
};

struct Candidate {
  bool active;     // wave-uniform: the wave holds a candidate within the limits
  int L, M[2];
  bool two;
  uint64_t text_off, mir_off[2];
};

// the string's and the miRNAs' lengths against the limits: state = kScreenOk (active) or kScreenHost
__device__ __forceinline__ Candidate candidate_of(uint64_t c, const uint32_t* __restrict__ cand_mir, const ScreenBlob& text, uint32_t item,
                                                  const ScreenBlob& mir, uint8_t* state) {
  Candidate cd;
  cd.active = false;
  cd.L = cd.M[0] = cd.M[1] = 0;
  cd.text_off = text.off[item];
  const uint64_t len = text.off[item + 1] - cd.text_off;
  const uint32_t m0 = cand_mir[2 * c], m1 = cand_mir[2 * c + 1];
  cd.two = m1 != kScreenNoIndex;
  cd.mir_off[0] = mir.off[m0];
  cd.mir_off[1] = cd.two ? mir.off[m1] : 0;
  const uint64_t l0 = mir.off[m0 + 1] - cd.mir_off[0], l1 = cd.two ? mir.off[m1 + 1] - cd.mir_off[1] : 0;
  if (len > kScreenMaxLen || l0 > kScreenMaxMir || l1 > kScreenMaxMir) {
    *state = kScreenHost;
  } else {
    *state = kScreenOk;
    cd.active = true;
    cd.L = (int)len;
    cd.M[0] = (int)l0;
    cd.M[1] = (int)l1;
  }
  return cd;
}

// phase 1: the strings into LDS, zero behind their ends; the pair table empty
__device__ __forceinline__ void load_candidate(WaveLds& w, const Candidate& cd, const ScreenBlob& text, const ScreenBlob& mir, int lane) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int p = lane + 64 * k;
    const bool in = cd.active && p < cd.L;
    w.seq[p] = in ? text.text[cd.text_off + p] : (char)0;
    w.str[p] = in ? text.text2[cd.text_off + p] : (char)0;
    w.pt[p] = -1;
    w.mir[0][p] = cd.active && p < cd.M[0] ? mir.text[cd.mir_off[0] + p] : (char)0;
    w.mir[1][p] = cd.active && p < cd.M[1] ? mir.text[cd.mir_off[1] + p] : (char)0;
  }
}

// phase 2: depth[p] = the open brackets after character p.  Returns whether the brackets balance.
__device__ __forceinline__ bool scan_depth(WaveLds& w, int lane) {
  const uint32_t word = *reinterpret_cast<const uint32_t*>(w.str + 4 * lane);
  int d[4], run = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t ch = (word >> (8 * k)) & 0xffu;
    run += (ch == '(') - (ch == ')');
    d[k] = run;
  }
  int incl = run;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(incl, o);
    if (lane >= o) incl += t;
  }
  const int base = incl - run;
  int lowest = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    w.depth[4 * lane + k] = (int16_t)(base + d[k]);
    lowest = min(lowest, base + d[k]);
  }
  return wave_min(lowest) >= 0 && __shfl(incl, 63) == 0;
}

// phase 3: the pair table (the brackets balance)
__device__ __forceinline__ void fill_partners(WaveLds& w, int L, int lane) {
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int p = lane + 64 * k;
    if (p < L && w.str[p] == '(') {
      const int want = w.depth[p] - 1;
      int j = p + 1;
      while (j < L && w.depth[j] != want) ++j;
      if (j < L) {
        w.pt[p] = (int16_t)j;
        w.pt[j] = (int16_t)p;
      }
    }
  }
}

// Python's s[lo:hi] over a string of L characters, as [a, b)
__device__ __forceinline__ void py_slice(int lo, int hi, int L, int* a, int* b) {
  if (lo < 0) lo = max(lo + L, 0);
  if (hi < 0) hi = max(hi + L, 0);
  lo = min(lo, L);
  hi = min(hi, L);
  *a = lo;
  *b = max(hi, lo);
}

struct SliceStats {
  int n_open, n_close, first_open, last_close;
};
__device__ __forceinline__ SliceStats slice_stats(const WaveLds& w, int a, int b, int lane) {
  SliceStats s{0, 0, INT_MAX, -1};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int p = lane + 64 * k;
    if (p >= a && p < b) {
      const char ch = w.str[p];
      if (ch == '(') {
        ++s.n_open;
        s.first_open = min(s.first_open, p);
      } else if (ch == ')') {
        ++s.n_close;
        s.last_close = max(s.last_close, p);
      }
    }
  }
  s.n_open = wave_sum(s.n_open);
  s.n_close = wave_sum(s.n_close);
  s.first_open = wave_min(s.first_open);
  s.last_close = wave_max(s.last_close);
  return s;
}
// checkArm over the miRNA's stretch of the structure
__device__ __forceinline__ int arm_of(const SliceStats& s) {
  if (s.n_open && s.n_close && s.first_open < s.last_close) return kArmLoop;
  if (s.n_open) return s.n_open >= s.n_close ? kArm5 : kArm3;
  return s.n_close ? kArm3 : kArmUnmatched;
}

// str.find: the first position the miRNA stands at, or -1
__device__ __forceinline__ int wave_find(const WaveLds& w, int L, int t, int M, int lane) {
  int best = INT_MAX;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int p = lane + 64 * k;
    if (p + M <= L) {
      int i = 0;
      while (i < M && w.seq[p + i] == w.mir[t][i]) ++i;
      if (i == M) best = min(best, p);
    }
  }
  best = wave_min(best);
  return best == INT_MAX ? -1 : best;
}

__global__ __launch_bounds__(kThreads) void screen_prune_kernel(uint32_t n_cand, const uint32_t* __restrict__ cand_rec,
                                                                const uint32_t* __restrict__ cand_mir, ScreenBlob rec, ScreenBlob mir,
                                                                int32_t pruned_length, uint8_t* __restrict__ status, uint32_t* __restrict__ lo,
                                                                uint32_t* __restrict__ hi, uint32_t* __restrict__ len32,
                                                                uint32_t* __restrict__ stat) {
  __shared__ WaveLds lds[kWaves];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint64_t c = (uint64_t)blockIdx.x * kWaves + wave;
  WaveLds& w = lds[wave];
  Candidate cd;
  cd.active = false;
  cd.L = cd.M[0] = cd.M[1] = 0;
  cd.two = false;
  uint8_t state = kScreenUnused;
  if (c < n_cand) {
    const uint32_t r = cand_rec[c];
    if (r != kScreenNoIndex) cd = candidate_of(c, cand_mir, rec, r, mir, &state);
  }
  load_candidate(w, cd, rec, mir, lane);
  __syncthreads();
  if (cd.active && !scan_depth(w, lane)) {
    cd.active = false;
    state = kScreenRefused;
  }
  __syncthreads();
  if (cd.active) fill_partners(w, cd.L, lane);
  __syncthreads();
  int a = 0, b = 0;
  if (cd.active) {
    const int L = cd.L;
    int sel = 0, pos = wave_find(w, L, 0, cd.M[0], lane);
    if (cd.two && pos != 20) {
      sel = 1;
      pos = wave_find(w, L, 1, cd.M[1], lane);
    }
    const int s = pos, e = pos + (sel ? cd.M[1] : cd.M[0]);  // (constant indices: the struct stays in registers)
    int sa, sb;
    py_slice(s, e, L, &sa, &sb);
    const SliceStats in = slice_stats(w, sa, sb, lane);
    state = kScreenNone;
    if (arm_of(in) == kArm5) {  // (the miRNA was found: an absent one has no `(` in its stretch of a balanced structure)
      const int q = in.first_open, other = q - s, partner = w.pt[q];
      if (partner >= 0) {
        py_slice(s - pruned_length, min(other + partner, L - 1) + 1 + pruned_length, L, &a, &b);
        state = kScreenOk;
      }
    } else if (e - 1 >= L) {  // the reference reads the structure beyond its end and dies
      state = kScreenRefused;
    } else {
      const SliceStats before = slice_stats(w, 0, max(e, 0), lane);
      const int q = before.last_close;
      if (q >= 0 && w.pt[q] >= 0) {
        const int other = e - 1 - q;
        py_slice(max(w.pt[q] - other, 0) - pruned_length, e + pruned_length, L, &a, &b);
        state = kScreenOk;
      }
    }
  }
  if (c < n_cand && lane == 0) {
    if (state == kScreenRefused) set_stat(stat, kScreenStatRefused);
    const bool ok = state == kScreenOk;
    status[c] = state;
    lo[c] = ok ? (uint32_t)a : 0u;
    hi[c] = ok ? (uint32_t)b : 0u;
    len32[c] = ok ? (uint32_t)(b - a) : 0u;
  }
}

__global__ __launch_bounds__(kThreads) void screen_copy_kernel(uint32_t n_cand, const uint32_t* __restrict__ cand_rec, ScreenBlob rec,
                                                               const uint8_t* __restrict__ status, const uint32_t* __restrict__ lo,
                                                               const uint32_t* __restrict__ hi, const uint64_t* __restrict__ pruned_off,
                                                               char* __restrict__ pruned) {
  const uint64_t c = ((uint64_t)blockIdx.x * kThreads + threadIdx.x) >> 6;
  const uint32_t lane = threadIdx.x & 63;
  if (c >= n_cand || status[c] != kScreenOk) return;
  const uint64_t src = rec.off[cand_rec[c]] + lo[c], dst = pruned_off[c];
  const uint32_t n = hi[c] - lo[c];  // (at most kScreenMaxLen: the prune kernel's)
  for (uint32_t i = lane; i < n; i += 64) pruned[dst + i] = rec.text[src + i];
}

// The overlap of the miRNA's positions s .. e with a hairpin's r0 .. r1, and the distance to it by the arm.
__device__ __forceinline__ int overlap_of(int s, int e, int r0, int r1) { return max(0, min(e, r1) - max(s, r0) + 1); }
__device__ __forceinline__ int distance_of(int arm, int s, int e, int r0, int r1) { return arm == kArm5 ? r0 - 1 - e : s - r1 - 1; }

__global__ __launch_bounds__(kThreads) void screen_features_kernel(uint32_t n_cand, const uint8_t* __restrict__ status,
                                                                   const uint32_t* __restrict__ cand_mir, ScreenBlob text, ScreenBlob mir,
                                                                   int32_t* __restrict__ feat, uint32_t* __restrict__ stat) {
  __shared__ WaveLds lds[kWaves];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint64_t c = (uint64_t)blockIdx.x * kWaves + wave;
  WaveLds& w = lds[wave];
  Candidate cd;
  cd.active = false;
  cd.L = cd.M[0] = cd.M[1] = 0;
  cd.two = false;
  uint8_t state = kScreenNone;
  if (c < n_cand && status[c] == kScreenOk) cd = candidate_of(c, cand_mir, text, (uint32_t)c, mir, &state);
  load_candidate(w, cd, text, mir, lane);
  __syncthreads();
  if (cd.active && !scan_depth(w, lane)) {
    cd.active = false;
    state = kScreenRefused;
  }
  __syncthreads();
  if (cd.active) fill_partners(w, cd.L, lane);
  __syncthreads();
  int out[kScreenFeatWords];
#pragma unroll
  for (int k = 0; k < kScreenFeatWords; ++k) out[k] = 0;
  out[kSfArm2] = -1;
  if (cd.active) {
    const int L = cd.L;
    const SliceStats all = slice_stats(w, 0, L, lane);
    if (all.n_open == 0 || all.n_close == 0) {
      state = kScreenNone;
    } else {
      // the one or two miRNAs: first and last position (s may be -1), arm; the first one's stretch of the structure
      int s[2] = {0, 0}, e[2] = {0, 0}, arm[2] = {0, 0};
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        if (t == 1 && !cd.two) break;
        s[t] = wave_find(w, L, t, cd.M[t], lane);
        e[t] = s[t] + cd.M[t] - 1;
        int sa, sb;
        py_slice(s[t], s[t] + cd.M[t], L, &sa, &sb);
        const SliceStats in = slice_stats(w, sa, sb, lane);
        arm[t] = arm_of(in);
        if (t == 0) {
          out[kSfBound] = in.n_open + in.n_close;
          out[kSfMirLen] = sb - sa;
        }
      }
      // every lane's own brackets: the hairpins they close, interior loops, stems
      int hairpins = 0, interior = 0, stems = 0, apical = 0, ugu = 0, bad = 0, r0[4], r1[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int p = lane + 64 * k;
        r0[k] = r1[k] = -1;
        if (p < L && w.str[p] == '(') {
          const int j = w.pt[p];
          int q = p + 1;
          while (q < L && w.str[q] == '.') ++q;
          if (q >= L) {
            bad = 1;
          } else if (q == j) {
            if (j - p - 1 < 3) bad = 1;
            ++hairpins;
            r0[k] = p + 1;
            r1[k] = j - 1;
            apical = max(apical, j - p - 1);
            for (int x = p + 1; x + 2 <= j - 2; ++x)  // seq[r0:r1] leaves the loop's last base out
              if (w.seq[x] == 'U' && w.seq[x + 1] == 'G' && w.seq[x + 2] == 'U') ugu = 1;
          } else if (w.str[q] == '(') {
            const int l = w.pt[q];
            int m = l + 1;
            while (m < L && w.str[m] == '.') ++m;
            if (m == j && (q > p + 1 || l < j - 1)) ++interior;
          }
          if (!(p > 0 && w.str[p - 1] == '(' && w.pt[p - 1] == j + 1)) ++stems;
        }
      }
      hairpins = wave_sum(hairpins);
      interior = wave_sum(interior);
      stems = wave_sum(stems);
      apical = wave_max(apical);
      ugu = wave_max(ugu);
      bad = wave_max(bad);
      int over[2] = {0, 0}, dist[2] = {0, 0};
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        if (t == 1 && !cd.two) break;
        int best = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (r0[k] >= 0) best = max(best, overlap_of(s[t], e[t], r0[k], r1[k]));
        best = wave_max(best);
        // overlap 0: the nearest hairpin; otherwise the first hairpin along the sequence with that overlap
        int first = INT_MAX;
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (r0[k] >= 0 && overlap_of(s[t], e[t], r0[k], r1[k]) == best) first = min(first, r0[k]);
        first = wave_min(first);
        int d = INT_MAX;
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (r0[k] >= 0 && (best == 0 || r0[k] == first)) d = min(d, distance_of(arm[t], s[t], e[t], r0[k], r1[k]));
        d = wave_min(d);
        over[t] = best;
        dist[t] = d == INT_MAX ? 0 : d;
      }
      state = bad ? kScreenRefused : (stems >= kScreenMaxElements || hairpins >= kScreenMaxElements) ? kScreenHost : kScreenOk;
      out[kSfHairpins] = hairpins;
      out[kSfBindings] = max(all.n_open, all.n_close);
      out[kSfInterior] = interior;
      out[kSfArm1] = arm[0];
      out[kSfApical] = apical;
      out[kSfOver1] = over[0];
      out[kSfDist1] = dist[0];
      out[kSfArm2] = cd.two ? arm[1] : -1;
      out[kSfOver2] = over[1];
      out[kSfDist2] = dist[1];
      out[kSfStemLen] = all.n_open;  // fewer than ten stems: every stem its own key, the sum of the stems' lengths
      out[kSfUgu] = ugu;
      out[kSfStems] = stems;
    }
  }
  out[kSfState] = state;
  if (c < n_cand) {
    if (lane == 0 && state == kScreenRefused) set_stat(stat, kScreenStatRefused);
    if (lane < (int)kScreenFeatWords) {
      int v = 0;
#pragma unroll
      for (int k = 0; k < kScreenFeatWords; ++k)
        if (lane == k) v = out[k];
      feat[c * kScreenFeatWords + lane] = v;
    }
  }
}

__device__ __forceinline__ bool retained(const int32_t* __restrict__ f, int32_t threshold) {
  const double percent = f[kSfMirLen] > 0 ? (double)f[kSfBound] / (double)f[kSfMirLen] : 0.0;
  if (!(f[kSfHairpins] > 0 && f[kSfBindings] >= threshold && percent >= 0.6)) return false;
  int over5 = -1, over3 = -1;  // armTypeOverlenDic: the second miRNA's entry replaces the first's under the same arm
  if (f[kSfArm1] == kArm5) over5 = f[kSfOver1];
  if (f[kSfArm1] == kArm3) over3 = f[kSfOver1];
  if (f[kSfArm2] == kArm5) over5 = f[kSfOver2];
  if (f[kSfArm2] == kArm3) over3 = f[kSfOver2];
  if (over5 >= 0 && over3 >= 0) return over5 <= 5 && over3 == 0;
  if (over5 >= 0) return over5 <= 5;
  return over3 == 0;
}

__global__ __launch_bounds__(kThreads) void screen_select_kernel(uint32_t n_lines, const uint8_t* __restrict__ cand_n,
                                                                 const uint32_t* __restrict__ cand_rec, uint32_t n_rec,
                                                                 const double* __restrict__ rec_mfe, const int32_t* __restrict__ feat,
                                                                 int32_t threshold, int32_t* __restrict__ best, uint32_t* __restrict__ stat) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n_lines) return;
  const uint32_t n = cand_n[i];
  int chosen = -1;
  bool chosen_kept = false;
  double chosen_mfe = 0.0;
  if (n != 2 && n != 4) set_stat(stat, kScreenStatBadLine);
  for (uint32_t k = 0; k < 4; ++k) {
    if (k >= n || (n != 2 && n != 4)) break;
    const int32_t* f = feat + (4 * i + k) * kScreenFeatWords;
    const uint32_t r = cand_rec[4 * i + k];
    if (r >= n_rec || (f[kSfState] != kScreenOk && f[kSfState] != kScreenNone)) {  // (a host row not patched in counts too)
      set_stat(stat, kScreenStatBadCand);
      continue;
    }
    if (f[kSfState] != kScreenOk) continue;
    const bool kept = retained(f, threshold);
    const double mfe = rec_mfe[r];
    if (chosen < 0 || (kept && !chosen_kept) || (kept == chosen_kept && mfe < chosen_mfe)) {
      chosen = (int)k;
      chosen_kept = kept;
      chosen_mfe = mfe;
    }
  }
  best[i] = chosen;
}

}  // namespace

hipError_t screen_candidates_launch(uint32_t n_lines, const uint32_t* line_group, uint32_t n_groups, const uint8_t* nb_flags,
                                    const int64_t* nb_up, const int64_t* nb_down, uint8_t* cand_n, uint32_t* cand_rec, uint32_t* cand_mir,
                                    uint32_t* stat, hipStream_t stream) {
  if (n_lines == 0) return hipSuccess;
  hipLaunchKernelGGL(screen_candidates_kernel, dim3(grid_for(n_lines)), dim3(kThreads), 0, stream, n_lines, line_group, n_groups, nb_flags, nb_up,
                     nb_down, cand_n, cand_rec, cand_mir, stat);
  return hipGetLastError();
}

hipError_t screen_check_offsets_launch(const ScreenBlob& b, uint32_t* stat, hipStream_t stream) {
  hipLaunchKernelGGL(screen_check_offsets_kernel, dim3(grid_for((uint64_t)b.n + 1)), dim3(kThreads), 0, stream, b, stat);
  return hipGetLastError();
}

hipError_t screen_check_cands_launch(uint32_t n_cand, const uint32_t* cand_rec, const uint8_t* status, const uint32_t* cand_mir, uint32_t n_rec,
                                     uint32_t n_mir, uint32_t* stat, hipStream_t stream) {
  if (n_cand == 0) return hipSuccess;
  hipLaunchKernelGGL(screen_check_cands_kernel, dim3(grid_for(n_cand)), dim3(kThreads), 0, stream, n_cand, cand_rec, status, cand_mir, n_rec, n_mir,
                     stat);
  return hipGetLastError();
}

hipError_t screen_prune_launch(uint32_t n_cand, const uint32_t* cand_rec, const uint32_t* cand_mir, const ScreenBlob& rec, const ScreenBlob& mir,
                               int32_t pruned_length, uint8_t* status, uint32_t* lo, uint32_t* hi, uint32_t* len32, uint32_t* stat,
                               hipStream_t stream) {
  if (n_cand == 0) return hipSuccess;
  hipLaunchKernelGGL(screen_prune_kernel, dim3(wave_grid_for(n_cand)), dim3(kThreads), 0, stream, n_cand, cand_rec, cand_mir, rec, mir,
                     pruned_length, status, lo, hi, len32, stat);
  return hipGetLastError();
}

hipError_t screen_copy_launch(uint32_t n_cand, const uint32_t* cand_rec, const ScreenBlob& rec, const uint8_t* status, const uint32_t* lo,
                              const uint32_t* hi, const uint64_t* pruned_off, char* pruned, hipStream_t stream) {
  if (n_cand == 0) return hipSuccess;
  hipLaunchKernelGGL(screen_copy_kernel, dim3(wave_grid_for(n_cand)), dim3(kThreads), 0, stream, n_cand, cand_rec, rec, status, lo, hi,
                     pruned_off, pruned);
  return hipGetLastError();
}

hipError_t screen_features_launch(uint32_t n_cand, const uint8_t* status, const uint32_t* cand_mir, const ScreenBlob& pruned, const ScreenBlob& mir,
                                  int32_t* feat, uint32_t* stat, hipStream_t stream) {
  if (n_cand == 0) return hipSuccess;
  hipLaunchKernelGGL(screen_features_kernel, dim3(wave_grid_for(n_cand)), dim3(kThreads), 0, stream, n_cand, status, cand_mir, pruned, mir, feat,
                     stat);
  return hipGetLastError();
}

hipError_t screen_select_launch(uint32_t n_lines, const uint8_t* cand_n, const uint32_t* cand_rec, uint32_t n_rec, const double* rec_mfe,
                                const int32_t* feat, int32_t threshold, int32_t* best, uint32_t* stat, hipStream_t stream) {
  if (n_lines == 0) return hipSuccess;
  hipLaunchKernelGGL(screen_select_kernel, dim3(grid_for(n_lines)), dim3(kThreads), 0, stream, n_lines, cand_n, cand_rec, n_rec, rec_mfe, feat,
                     threshold, best, stat);
  return hipGetLastError();
}

}  // namespace mrg
