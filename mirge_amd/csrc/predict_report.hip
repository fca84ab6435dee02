// Predict mode's report on the device (mrg_predict_report_correct / _entries / _profile, include/mirge_amd.h).  gfx950,
// wave64, no atomics.
//
// report_correct_kernel: one wave (one workgroup) per table line.  Which pair of strings a line ends up with is a function
// of the line and its two neighbours, so every wave works out src on its own; the corrected precursor and structure (at most
// 256 characters), the line's clusterSeq and stableClusterSeq (at most 255, T read as U) sit in 1 KiB of LDS.  str.find runs
// with one start offset a lane, 64 at a time, and a ballot names the first; the first `(` and the last `)` of the stretch
// come from ballots too.
// The entry pass sorts the lines by their interned group (the project's radix sort, stable: file order inside a group),
// lets every group's first position write its chunks' keys (the first listed member's rank), sorts the chunks by that key
// and numbers the entries with the project's prefix sum.
// report_profile_kernel: one wave per entry.  The precursor sits in LDS; the entry's read rows pass through LDS 64 at a time
// (one row a lane: dashes in front, where its bases start in the text, length, dashes behind, count); lanes own precursor
// positions p = 64 r + lane, r < 4, and add the rows' counts in row order into uint64 registers.
// Every output word has one writer.
#include "predict_report.hpp"

#include "prims.hpp"

namespace mrg {

namespace {

constexpr uint32_t kWave = 64, kThreads = 256;
static_assert(kReportMaxPrec == 4 * kWave, "a lane owns four precursor positions");
static_assert(kReportTile == kWave, "one staged row a lane");

inline uint32_t grid_for(uint64_t n) { return (uint32_t)((n + kThreads - 1) / kThreads); }

__device__ __forceinline__ uint32_t arm_of(uint8_t flags) { return (flags >> kRepArmShift) & 3u; }
__device__ __forceinline__ bool distance_ok(int64_t v) { return v != kReportNone && v != kReportBad; }

// s.find(t) over LDS, all 64 lanes: -1 where t is not in s
__device__ int wave_find(const char* s, int ls, const char* t, int lt) {
  if (lt == 0) return 0;
  if (lt > ls) return -1;
  const int lane = (int)threadIdx.x;
  for (int base = 0; base + lt <= ls; base += (int)kWave) {
    const int o = base + lane;
    bool ok = o + lt <= ls;
    for (int k = 0; ok && k < lt; ++k) ok = s[o + k] == t[k];
    const unsigned long long m = __ballot(ok);
    if (m) return base + (int)__ffsll((long long)m) - 1;
  }
  return -1;
}

// offsets 4 i .. 4 i + 4 of line i ascend inside the text
__device__ __forceinline__ bool offsets_ok(const ReportLines& in, uint32_t i) {
  const uint64_t* o = in.t_off + 4ull * i;
  return o[0] <= o[1] && o[1] <= o[2] && o[2] <= o[3] && o[3] <= o[4] && o[4] <= in.text_len;
}

__global__ __launch_bounds__(kWave) void report_correct_kernel(ReportLines in, ReportLineOut out) {
  __shared__ char s_seq[kReportMaxPrec], s_str[kReportMaxPrec], s_cs[kReportMaxPrec], s_st[kReportMaxPrec];
  const uint32_t j = blockIdx.x, n = in.n, lane = threadIdx.x;
  const uint8_t f = in.flags[j];
  // the offers (every lane works out the same)
  auto qualifies = [&](uint32_t i) {
    const uint8_t fi = in.flags[i];
    return (fi & kRepListed) && (fi & kRepPairYes) && in.up[i] != kReportNone;
  };
  auto takes_from = [&](uint32_t i) { return (f & kRepPairYes) && arm_of(f) <= kRepArm3 && arm_of(f) != arm_of(in.flags[i]); };
  bool from_prev = false, from_next = false;
  if (j > 0 && qualifies(j - 1)) {
    const int64_t up = in.up[j - 1], down = in.down[j - 1];
    from_prev = up != kReportBad && up > 44 && distance_ok(down) && down <= 44;
  }
  if (j + 1 < n && qualifies(j + 1)) {
    const int64_t up = in.up[j + 1];
    from_next = up != kReportBad && up <= 44;
  }
  uint8_t err = 0;
  if (qualifies(j)) {
    const int64_t up = in.up[j], down = in.down[j];
    if (up == kReportBad) err = kRepErrUp;
    else if (up > 44 && !distance_ok(down)) err = kRepErrDown;
    else if (up > 44 && down <= 44 && j + 1 == n) err = kRepErrLast;
  }
  uint32_t src = j;
  if (from_prev && takes_from(j - 1)) src = j - 1;
  if (from_next && takes_from(j + 1)) src = j + 1;   // applied later in file order: it stands
  const bool none = (in.flags[src] & kRepPrecNone) != 0;
  if (!err && (f & kRepListed) && none) err = kRepErrListedNone;

  bool host = false, loop = false;
  int stable = -1;
  if (!offsets_ok(in, j) || !offsets_ok(in, src)) {
    err = kRepErrOffsets;
  } else {
    const uint64_t *os = in.t_off + 4ull * src, *oj = in.t_off + 4ull * j;
    const uint64_t l_seq = os[1] - os[0], l_str = os[2] - os[1], l_cs = oj[3] - oj[2], l_st = oj[4] - oj[3];
    host = l_seq > kReportMaxPrec || l_str > kReportMaxPrec || l_cs > kReportMaxSeq || l_st > kReportMaxSeq;
    if (!host) {
      for (uint32_t p = lane; p < l_seq; p += kWave) s_seq[p] = in.text[os[0] + p];
      for (uint32_t p = lane; p < l_str; p += kWave) s_str[p] = in.text[os[1] + p];
      for (uint32_t p = lane; p < l_cs; p += kWave) {
        const char c = in.text[oj[2] + p];
        s_cs[p] = c == 'T' ? 'U' : c;
      }
      for (uint32_t p = lane; p < l_st; p += kWave) {
        const char c = in.text[oj[3] + p];
        s_st[p] = c == 'T' ? 'U' : c;
      }
      __syncthreads();
      const int start = wave_find(s_seq, (int)l_seq, s_cs, (int)l_cs);
      // the stretch str[start : start + len]; an absent clusterSeq leaves at most one character: no pair of brackets
      if (start >= 0) {
        const int lo = start, hi = min(start + (int)l_cs, (int)l_str);
        int first_open = -1, last_close = -1;
        for (int base = lo; base < hi; base += (int)kWave) {
          const int p = base + (int)lane;
          const unsigned long long mo = __ballot(p < hi && s_str[p] == '('), mc = __ballot(p < hi && s_str[p] == ')');
          if (mo && first_open < 0) first_open = base + (int)__ffsll((long long)mo) - 1;
          if (mc) last_close = base + 63 - (int)__clzll((long long)mc);
        }
        loop = first_open >= 0 && last_close > first_open;
      }
      stable = wave_find(s_seq, (int)l_seq, s_st, (int)l_st);
    }
  }
  if (lane != 0) return;
  const uint32_t arm = arm_of(f);
  const bool retyped = loop && arm != kRepLoop;
  const uint32_t arm_new = retyped ? (uint32_t)kRepLoop : arm;
  out.src[j] = src;
  out.state[j] = (uint8_t)(((from_prev || from_next) ? kRepTouched : 0) | (retyped ? kRepRetyped : 0) | (host ? kRepHost : 0) |
                           (none ? kRepNone : 0) | (arm_new << kRepStateArmShift));
  out.err[j] = err;
  const int32_t *a = in.adj + 4ull * j;
  const int64_t s0 = in.pos[2ull * j], e0 = in.pos[2ull * j + 1];
  const bool minus = (f & kRepMinus) != 0;
  out.pos_adj[2ull * j] = minus ? s0 - a[1] + a[3] : s0 - a[0] + a[2];
  out.pos_adj[2ull * j + 1] = minus ? e0 + a[0] - a[2] : e0 + a[1] - a[3];
  out.stable_idx[j] = stable;
  out.gid[j] = none ? kReportNoGroup : in.gid3[3ull * j + (src + 1 - j)];
}

// ------------------------------------------------------------------------------------------------ the entry pass
__global__ __launch_bounds__(kThreads) void report_keys_kernel(uint32_t n, const uint32_t* __restrict__ gid, uint32_t* __restrict__ key,
                                                               uint32_t* __restrict__ val, uint32_t* __restrict__ cval) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  key[i] = gid[i];
  val[i] = (uint32_t)i;
  cval[i] = (uint32_t)i;
}

// the first position of every group: the first listed member's rank into the key of each of the group's chunks (ckey is
// filled with 0xff before)
__global__ __launch_bounds__(kThreads) void report_groups_kernel(uint32_t n, const uint32_t* __restrict__ key, const uint32_t* __restrict__ val,
                                                                 const uint8_t* __restrict__ flags, const uint32_t* __restrict__ rank,
                                                                 uint32_t* __restrict__ ckey) {
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const uint32_t k = key[i];
  if (k == kReportNoGroup || (i > 0 && key[i - 1] == k)) return;
  uint32_t best = 0xffffffffu;
  uint64_t e = i;
  for (; e < n && key[e] == k; ++e) {
    const uint32_t line = val[e];
    if (flags[line] & kRepListed) best = min(best, rank[line]);
  }
  if (best == 0xffffffffu) return;   // no listed member: never visited
  for (uint64_t c = i; c < e; c += 2) ckey[c] = best;
}

__global__ __launch_bounds__(kThreads) void report_chunks_kernel(uint32_t n, const uint32_t* __restrict__ ckey, const uint32_t* __restrict__ cval,
                                                                 const uint32_t* __restrict__ key, const uint32_t* __restrict__ val,
                                                                 ReportLines in, ReportLineOut lines, const uint8_t* __restrict__ blk,
                                                                 uint32_t* __restrict__ cm, int32_t* __restrict__ cp, uint32_t* __restrict__ emit,
                                                                 uint8_t* __restrict__ chunk_err, uint32_t* __restrict__ chunk_line) {
  const uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (k >= n) return;
  uint32_t m = 0, e = 0;
  int32_t p = -1;
  uint8_t err = 0;
  if (ckey[k] != 0xffffffffu) {
    const uint32_t at = cval[k], a = val[at];
    m = a;
    if (at + 1 < n && key[at + 1] == key[at]) {
      const uint32_t b = val[at + 1];
      const bool la = (in.flags[a] & kRepListed) != 0, lb = (in.flags[b] & kRepListed) != 0;
      bool first;   // the first member is the mature one
      if (la && lb) first = in.reads[a] >= in.reads[b];
      else first = la && !lb;
      m = first ? a : b;
      p = (int32_t)(first ? b : a);
      if (((lines.state[p] >> kRepStateArmShift) & 3u) == kRepLoop) p = -1;
    }
    e = ((lines.state[m] >> kRepStateArmShift) & 3u) != kRepLoop;
    // padClusteredList runs before the arm is looked at: its .index() and the blocks it reads
    if (blk[m] != 1 || (p >= 0 && blk[p] != 1)) err = kRepErrBlock;
    else if (lines.stable_idx[m] < 0 || (p >= 0 && lines.stable_idx[p] < 0)) err = kRepErrAbsent;
    else if (e && !(in.flags[m] & kRepListed)) err = kRepErrUnlisted;
  }
  cm[k] = m;
  cp[k] = p;
  emit[k] = e;
  chunk_err[k] = err;
  chunk_line[k] = m;
}

__global__ __launch_bounds__(kThreads) void report_entries_kernel(uint32_t n, const uint32_t* __restrict__ cm, const int32_t* __restrict__ cp,
                                                                  const uint32_t* __restrict__ emit, const uint32_t* __restrict__ num,
                                                                  ReportLines in, const uint32_t* __restrict__ src, const uint64_t* __restrict__ r_off,
                                                                  uint32_t* __restrict__ ent_m, int32_t* __restrict__ ent_p,
                                                                  uint32_t* __restrict__ rows32, uint32_t* __restrict__ len32,
                                                                  uint32_t* __restrict__ n_entries) {
  const uint64_t k = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (k >= n) return;
  if (k + 1 == n) *n_entries = num[k] + emit[k];
  if (!emit[k]) return;
  const uint32_t e = num[k], m = cm[k];
  const int32_t p = cp[k];
  ent_m[e] = m;
  ent_p[e] = p;
  uint64_t rows = r_off[m + 1] - r_off[m];
  if (p >= 0) rows += r_off[p + 1] - r_off[p];
  rows32[e] = (uint32_t)min(rows, (uint64_t)0xffffffffu);
  const uint64_t* o = in.t_off + 4ull * src[m];
  len32[e] = (uint32_t)(o[1] - o[0]);
}

// ------------------------------------------------------------------------------------------------ the profiles
__global__ __launch_bounds__(kWave) void report_profile_kernel(ReportLines in, ReportLineOut lines, ReportRows rows, uint32_t n_entries,
                                                               const uint32_t* __restrict__ ent_m, const int32_t* __restrict__ ent_p,
                                                               const uint64_t* __restrict__ row_off, const uint64_t* __restrict__ prof_off,
                                                               ReportProfileOut out) {
  __shared__ char s_prec[kReportMaxPrec];
  __shared__ int32_t s_lead[kReportTile], s_len[kReportTile], s_trail[kReportTile];
  __shared__ uint64_t s_at[kReportTile], s_count[kReportTile];
  const uint32_t e = blockIdx.x, lane = threadIdx.x;
  const uint32_t m = ent_m[e];
  const int32_t p = ent_p[e];
  // what the kernel checks before it reads through an index: the lines exist, the precursor lies inside the text, the rows
  // named lie inside the row arrays, the entry's slices are the sizes the entry pass gave
  bool bad = m >= in.n || (p >= 0 && (uint32_t)p >= in.n);
  if (!bad) bad = lines.src[m] >= in.n;
  uint64_t L64 = 0, n_m = 0, n_p = 0;
  const uint64_t* o = in.t_off;
  if (!bad) {
    o = in.t_off + 4ull * lines.src[m];
    bad = o[0] > o[1] || o[1] > in.text_len;
  }
  if (!bad) {
    L64 = o[1] - o[0];
    bad = rows.r_off[m + 1] > rows.n_rows || rows.r_off[m] > rows.r_off[m + 1] || lines.stable_idx[m] < 0;
    if (!bad && p >= 0) bad = rows.r_off[p + 1] > rows.n_rows || rows.r_off[p] > rows.r_off[p + 1] || lines.stable_idx[p] < 0;
  }
  if (!bad) {
    n_m = rows.r_off[m + 1] - rows.r_off[m];
    n_p = p >= 0 ? rows.r_off[p + 1] - rows.r_off[p] : 0;
    bad = row_off[e + 1] - row_off[e] != n_m + n_p || prof_off[e + 1] - prof_off[e] != L64;
  }
  if (bad || L64 > kReportMaxPrec) {
    if (lane == 0) {
      out.flag[e] = bad ? kRepEntryBad : kRepEntryHost;
      out.total[e] = 0;
    }
    return;
  }
  const int L = (int)L64;
  for (int q = (int)lane; q < L; q += (int)kWave) s_prec[q] = in.text[o[0] + q];
  uint64_t acc[4] = {0, 0, 0, 0}, total = 0;
  bool ragged = false, host = false;
  const uint64_t n_all = n_m + n_p;
  for (uint64_t t0 = 0; t0 < n_all; t0 += kReportTile) {
    __syncthreads();   // (the tile before is read to its end; the first round: s_prec is written)
    const uint64_t r = t0 + lane;
    int lead = 0, trail = 0, len = 0;
    if (r < n_all) {
      const uint32_t x = r < n_m ? m : (uint32_t)p;   // the cluster the row belongs to
      const uint64_t row = r < n_m ? rows.r_off[m] + r : rows.r_off[p] + (r - n_m);
      const uint64_t a0 = rows.s_off[row], a1 = rows.s_off[row + 1];
      if (a0 > a1 || a1 > rows.text_len || a1 - a0 > kReportMaxSeq) {
        host = true;
      } else {
        const uint64_t* ox = in.t_off + 4ull * x;
        const int64_t head_len = lines.stable_idx[x], tail_len = (int64_t)L - head_len - (int64_t)(ox[4] - ox[3]);
        const bool minus = (in.flags[x] & kRepMinus) != 0;
        const int64_t p_head = lines.pos_adj[2ull * x] - (minus ? tail_len : head_len);
        const int64_t p_tail = lines.pos_adj[2ull * x + 1] + (minus ? head_len : tail_len);
        const int64_t before = rows.start[row] - p_head, behind = p_tail - rows.end[row];
        const int64_t ld = max((int64_t)0, minus ? behind : before), tr = max((int64_t)0, minus ? before : behind);
        if (ld > kReportMaxPad || tr > kReportMaxPad) host = true;
        lead = (int)min(ld, kReportMaxPad);
        trail = (int)min(tr, kReportMaxPad);
        len = (int)(a1 - a0);
        s_at[lane] = a0;
        s_count[lane] = (uint64_t)rows.count[row];
        total += (uint64_t)rows.count[row];
        ragged = ragged || lead + len + trail != L;
        out.lead[row_off[e] + r] = lead;
        out.trail[row_off[e] + r] = trail;
      }
    }
    s_lead[lane] = lead;
    s_len[lane] = len;
    s_trail[lane] = trail;
    if (__ballot(host)) break;   // (uniform: every lane leaves)
    __syncthreads();
    const int live = (int)min((uint64_t)kReportTile, n_all - t0);
    for (int i = 0; i < live; ++i) {
      const int ld = s_lead[i], ln = s_len[i], end = ld + ln + s_trail[i];
      const uint64_t at = s_at[i], cnt = s_count[i];
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int q = rr * (int)kWave + (int)lane;
        if (q < L && q < end) {
          const char c = (q < ld || q >= ld + ln) ? '-' : rows.text[at + (uint64_t)(q - ld)];   // (the rows' text is RNA already)
          if (c == s_prec[q]) acc[rr] += cnt;
        }
      }
    }
  }
  const bool any_host = __ballot(host) != 0, any_ragged = __ballot(ragged) != 0;
#pragma unroll
  for (int w = 32; w; w >>= 1) total += __shfl_xor(total, w);
  if (!any_host) {
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int q = rr * (int)kWave + (int)lane;
      if (q < L) out.prof[prof_off[e] + q] = acc[rr];
    }
  }
  if (lane == 0) {
    out.flag[e] = any_host ? kRepEntryHost : (any_ragged ? kRepRagged : 0);
    out.total[e] = any_host ? 0 : total;
  }
}

}  // namespace

hipError_t report_correct_launch(const ReportLines& in, const ReportLineOut& out, hipStream_t stream) {
  if (in.n == 0) return hipSuccess;
  hipLaunchKernelGGL(report_correct_kernel, dim3(in.n), dim3(kWave), 0, stream, in, out);
  return hipGetLastError();
}

hipError_t report_entries_launch(const ReportLines& in, const ReportLineOut& lines, const uint8_t* blk, const uint64_t* r_off,
                                 const ReportEntryScratch& sc, const ReportEntryOut& out, hipStream_t stream) {
  const uint32_t n = in.n;
  hipError_t e;
  // the offsets' sums run over n + 1 words: an entry slot that stays unused counts nothing
  if ((e = hipMemsetAsync(sc.rows32, 0, (n + 1ull) * sizeof(uint32_t), stream)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(sc.len32, 0, (n + 1ull) * sizeof(uint32_t), stream)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(out.n_entries, 0, sizeof(uint32_t), stream)) != hipSuccess) return e;
  if (n) {
    hipLaunchKernelGGL(report_keys_kernel, dim3(grid_for(n)), dim3(kThreads), 0, stream, n, lines.gid, sc.key0, sc.val0, sc.cval0);
    bool second = false;
    if ((e = prims::radix_sort_pairs_u32(sc.key0, sc.key1, sc.val0, sc.val1, n, 32, sc.sort_tmp, stream, &second)) != hipSuccess) return e;
    const uint32_t *key = second ? sc.key1 : sc.key0, *val = second ? sc.val1 : sc.val0;
    if ((e = hipMemsetAsync(sc.ckey0, 0xff, (size_t)n * sizeof(uint32_t), stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(report_groups_kernel, dim3(grid_for(n)), dim3(kThreads), 0, stream, n, key, val, in.flags, in.rank, sc.ckey0);
    bool csecond = false;
    if ((e = prims::radix_sort_pairs_u32(sc.ckey0, sc.ckey1, sc.cval0, sc.cval1, n, 32, sc.sort_tmp, stream, &csecond)) != hipSuccess) return e;
    const uint32_t *ckey = csecond ? sc.ckey1 : sc.ckey0, *cval = csecond ? sc.cval1 : sc.cval0;
    hipLaunchKernelGGL(report_chunks_kernel, dim3(grid_for(n)), dim3(kThreads), 0, stream, n, ckey, cval, key, val, in, lines, blk, sc.cm, sc.cp,
                       sc.emit, out.chunk_err, out.chunk_line);
    if ((e = prims::exclusive_sum_u32(sc.emit, sc.num, n, sc.scan_tmp, stream)) != hipSuccess) return e;
    hipLaunchKernelGGL(report_entries_kernel, dim3(grid_for(n)), dim3(kThreads), 0, stream, n, sc.cm, sc.cp, sc.emit, sc.num, in, lines.src, r_off,
                       out.ent_m, out.ent_p, sc.rows32, sc.len32, out.n_entries);
  }
  if ((e = prims::exclusive_sum_u32_to_u64(sc.rows32, out.row_off, n + 1ull, sc.scan_tmp, stream)) != hipSuccess) return e;
  if ((e = prims::exclusive_sum_u32_to_u64(sc.len32, out.prof_off, n + 1ull, sc.scan_tmp, stream)) != hipSuccess) return e;
  return hipGetLastError();
}

hipError_t report_profile_launch(const ReportLines& in, const ReportLineOut& lines, const ReportRows& rows, uint32_t n_entries,
                                 const uint32_t* ent_m, const int32_t* ent_p, const uint64_t* row_off, const uint64_t* prof_off,
                                 const ReportProfileOut& out, hipStream_t stream) {
  if (n_entries == 0) return hipSuccess;
  hipLaunchKernelGGL(report_profile_kernel, dim3(n_entries), dim3(kWave), 0, stream, in, lines, rows, n_entries, ent_m, ent_p, row_off, prof_off, out);
  return hipGetLastError();
}

}  // namespace mrg
