// `-ai` on the device (mrg_a2i_align, include/mirge_amd.h): every miRNA read aligned to the canonical sequence of its
// (merged) miRNA, as far as `pairwise2.align.localms(target, read, 2, -1, -20, -20)` (mirge_amd.a2i.local_pair) lands on
// one ungapped diagonal, and the few questions the -ai report asks of that frame.
//
// 32 lanes per pair, two pairs per wave: lane c holds column c (read base c) of the score tables and the rows (target
// bases) are walked one after the other.  A cell needs its upper-left neighbour (one shuffle up by one lane), the cells
// above it (this lane's own registers) and the cells to its left in the same row; since a gap base costs 20 and no score
// passes 64, a path with more than three gap bases scores below zero, so "to its left" is three more shuffles and not a
// scan.  Nothing is indexed in registers, so nothing can land in scratch, and the two pairs of a wave never look at each
// other's lanes (every shuffle has width 32).
//
//   U[r][c]  = max(0, U[r-1][c-1] + s)                       the ungapped local score; m = max U, ends = #{U == m}
//   Hg[r][c] = max(Hg, E, F)[r-1][c-1] + s                   best path ending in a pair here with an interior gap
//   E[r][c]  = max_k max(U, Hg)[r][c-k] - 20 k,  F[r][c] = max_k max(U, Hg)[r-k][c] - 20 k     (k = 1..3)
//   g = max Hg;  simple  <=>  m > 0, ends == 1, g < m        
//
// Only g < m is reported, never g, so the paths the truncation (and the missing zero column / row) drops, all of which
// score below m, change nothing.
//
// mrg_a2i_settle walks the pairs of status 1 (ends > 1) once more in the same layout and, where g < m, names the diagonal
// that localms lists first among the tied ones (a2i_settle_kernel, status 5).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "a2i_align.hpp"

namespace mrg {

namespace {

constexpr uint32_t kBlock = 256;
constexpr uint32_t kPairsPerBlock = kBlock / 32;
constexpr uint64_t kEven = 0x5555555555555555ull;
constexpr int32_t kNeg = -1000;   // "no such path"; 32 rows of -1 keep it far below every score

__device__ __forceinline__ bool a2i_selected(int32_t p, const uint8_t* __restrict__ keep, uint64_t i, int32_t canon_pass,
                                             int32_t isomir_pass) {
  return (p == canon_pass || p == isomir_pass) && (!keep || keep[i]);
}

__global__ __launch_bounds__(kBlock) void a2i_flags_kernel(const int8_t* __restrict__ pass_id, const uint8_t* __restrict__ keep,
                                                           uint64_t n, int32_t canon_pass, int32_t isomir_pass,
                                                           uint32_t* __restrict__ flags) {
  const uint64_t step = (uint64_t)gridDim.x * kBlock;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += step)
    flags[i] = a2i_selected(pass_id[i], keep, i, canon_pass, isomir_pass) ? 1u : 0u;
  if (blockIdx.x == 0 && threadIdx.x == 0) flags[n] = 0u;
}

__global__ __launch_bounds__(kBlock) void a2i_scatter_kernel(const int8_t* __restrict__ pass_id, const uint8_t* __restrict__ keep,
                                                             uint64_t n, int32_t canon_pass, int32_t isomir_pass,
                                                             const uint32_t* __restrict__ off, uint64_t cap,
                                                             uint32_t* __restrict__ idx) {
  const uint64_t step = (uint64_t)gridDim.x * kBlock;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += step) {
    if (!a2i_selected(pass_id[i], keep, i, canon_pass, isomir_pass)) continue;
    const uint64_t o = off[i];
    if (o < cap) idx[o] = (uint32_t)i;
  }
}

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

// x moved by d bases towards the high end (d < 0: towards the low end), |d| <= 31
__device__ __forceinline__ uint64_t shift_bases(uint64_t x, int32_t d) { return d >= 0 ? x << (2 * d) : x >> (2 * -d); }

// even bit 2i set: base i of x is not `code`
__device__ __forceinline__ uint64_t differs_from(uint64_t x, uint32_t code) {
  const uint64_t z = x ^ (kEven * (uint64_t)code);
  return (z | (z >> 1)) & kEven;
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

// What the report asks of the ungapped frame of diagonal d (target coordinates: the read covers [d, d + lb)); rw holds 0
// where rn marks an N.
__device__ __forceinline__ void frame_answers(uint64_t tw, uint64_t rw, uint64_t rn, int32_t la, int32_t lb, int32_t d,
                                              uint32_t from_base, uint32_t to_base, uint32_t& verdict, uint32_t& substring,
                                              uint32_t& edit) {
  const uint64_t rs = shift_bases(rw, d), ns = shift_bases(rn, d);
  const uint32_t cover = bit_range(max(0, d), min(la, d + lb));
  const uint64_t x = tw ^ rs;
  const uint32_t eq = ~squeeze_even((x | (x >> 1)) | ns) & cover;
  // judge_align: the window ends 3 nt before the end of the PADDED target (a trailing dash of the target counts as a
  // mismatch), measured from the padded start
  const int32_t lo = max(0, d);
  const int32_t hi = min(max(la, d + lb) - max(0, -d) - 4, d + lb - 1);
  const int32_t cells = max(0, hi - lo + 1);
  const int32_t mat = __popc(eq & bit_range(lo, hi + 1));
  const int32_t need = la - 4 - (d == 1 ? 1 : 0);
  verdict = (d <= 1 && !(cells - mat > 1 || mat < need)) ? 1u : 0u;
  substring = (d >= 0 && d + lb <= la && __popc(eq) == lb) ? 1u : 0u;
  edit = ~squeeze_even(differs_from(tw, from_base) | differs_from(rs, to_base) | ns) & cover & bit_range(0, la - 5);
}

__global__ __launch_bounds__(kBlock) void a2i_align_kernel(const A2iAlignParams p) {
  const uint32_t lane = threadIdx.x & 31u;
  const uint32_t wanted = blockIdx.x * kPairsPerBlock + (threadIdx.x >> 5);
  const uint32_t row = min(wanted, p.rows - 1u);   // (a group past the end repeats the last pair and stores nothing)
  const uint32_t read = p.idx[row];
  const int32_t pass = p.pass_id[read];
  const int32_t e = p.ref_id[read];
  int32_t target = -1;
  if (pass == p.canon_pass) {
    if (e >= 0 && (uint32_t)e < p.n_canon) target = p.canon_target[e];
  } else if (e >= 0 && (uint32_t)e < p.n_isomir) {
    target = p.isomir_target[e];
  }
  if (target < 0 || (uint32_t)target >= p.n_targets) target = -1;
  const int32_t la = target >= 0 ? (int32_t)p.target_lens[target] : 0;
  const int32_t lb = p.lens[read];
  const bool usable = la >= 1 && la <= 32 && lb >= 1 && lb <= 32;
  const uint64_t tw = usable ? p.target_words[target] : 0ull;
  const uint64_t rn = (usable && p.nmask) ? (p.nmask[read] & kEven) : 0ull;
  const uint64_t rw = usable ? (p.reads[read] & ~(rn * 3ull)) : 0ull;

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
  const int32_t d = group_sum((best == m && ends == 1) ? r_best - (int32_t)lane : 0);

  uint32_t status = kA2iSimple;
  if (!usable) status = kA2iUnsupported;
  else if (m <= 0) status = kA2iNoScore;
  else if (ends != 1) status = kA2iEnds;
  else if (gmax >= m) status = kA2iGapped;

  // ---- what the report asks of the frame of diagonal d
  uint32_t verdict = 0u, substring = 0u, edit = 0u;
  int32_t diag = 0;
  if (status == kA2iSimple) {
    diag = d;
    frame_answers(tw, rw, rn, la, lb, d, p.from_base, p.to_base, verdict, substring, edit);
  }
  if (lane == 0u && wanted < p.rows) {
    const uint32_t score = (status == kA2iUnsupported || m < 0) ? 0u : (uint32_t)m;
    int4 out;
    out.x = (int32_t)(status | (verdict << 8) | (substring << 9) | (score << 16));
    out.y = diag;
    out.z = (int32_t)edit;
    out.w = target;
    *reinterpret_cast<int4*>(p.rec + (uint64_t)row * kA2iRecInts) = out;
  }
}

// The rows mrg_a2i_settle examines: flags[i] = row i has status 1, flags[k] = 0; then sel[off[i]] = i.
__global__ __launch_bounds__(kBlock) void a2i_tied_flags_kernel(const int32_t* __restrict__ rec, uint64_t k, uint32_t* __restrict__ flags) {
  const uint64_t step = (uint64_t)gridDim.x * kBlock;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < k; i += step)
    flags[i] = ((uint32_t)rec[i * kA2iRecInts + kA2iRecFlags] & 0xFFu) == kA2iEnds ? 1u : 0u;
  if (blockIdx.x == 0 && threadIdx.x == 0) flags[k] = 0u;
}

__global__ __launch_bounds__(kBlock) void a2i_tied_scatter_kernel(const int32_t* __restrict__ rec, uint64_t k,
                                                                  const uint32_t* __restrict__ off, uint32_t* __restrict__ sel) {
  const uint64_t step = (uint64_t)gridDim.x * kBlock;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < k; i += step)
    if (((uint32_t)rec[i * kA2iRecInts + kA2iRecFlags] & 0xFFu) == kA2iEnds) sel[off[i]] = (uint32_t)i;
}

// A pair whose best ungapped score m ends in several cells (status 1), in a2i_align_kernel's layout.  Where every gapped
// path scores below m, pairwise2 lists first the diagonal of one of those cells, and which one follows from U alone
// ("ties"): a best cell is eligible iff no cell above it in the positive run of its diagonal holds m (one
// bit that travels with U in the shuffle); the best score is passed along the last row and the last column, and the
// listing stops at the first passed-along cell X whose upper-left neighbour is a best cell; the answer is the last
// eligible cell before X in row order.  Each lane keeps the rows of its best and of its eligible cells as two bit masks,
// so X is found after the loop from two columns and two rows of those masks.
__global__ __launch_bounds__(kBlock) void a2i_settle_kernel(const A2iSettleParams p) {
  const uint32_t lane = threadIdx.x & 31u;
  const uint32_t half = threadIdx.x & 32u;          // where this pair's lanes sit in the wave's ballot
  const uint32_t wanted = blockIdx.x * kPairsPerBlock + (threadIdx.x >> 5);
  const uint32_t row = p.sel[min(wanted, p.n_sel - 1u)];   // (a group past the end repeats the last pair and stores nothing)
  const int4 in = *reinterpret_cast<const int4*>(p.rec + (uint64_t)row * kA2iRecInts);
  const uint32_t read = p.idx[row];
  const int32_t m = (int32_t)(((uint32_t)in.x >> 16) & 0xFFFFu);
  const int32_t target = in.w;
  const bool known = wanted < p.n_sel && ((uint32_t)in.x & 0xFFu) == kA2iEnds && m > 0 && target >= 0 &&
                     (uint32_t)target < p.n_targets && (uint64_t)read < p.n_reads;
  const int32_t la = known ? (int32_t)p.target_lens[target] : 0;
  const int32_t lb = known ? (int32_t)p.lens[read] : 0;
  const bool usable = la >= 1 && la <= 32 && lb >= 1 && lb <= 32;
  const uint64_t tw = usable ? p.target_words[target] : 0ull;
  const uint64_t rn = (usable && p.nmask) ? (p.nmask[read] & kEven) : 0ull;
  const uint64_t rw = usable ? (p.reads[read] & ~(rn * 3ull)) : 0ull;

  const bool col = (int32_t)lane < lb;
  const uint32_t my_base = (uint32_t)(rw >> (2u * lane)) & 3u;
  const bool my_n = ((rn >> (2u * lane)) & 1ull) != 0ull || !col;
  int32_t UT = 0, X = kNeg, H1 = kNeg, H2 = kNeg, H3 = kNeg, g = kNeg;   // UT = U << 1 | "this run already holds a top"
  uint32_t tops = 0u, elig = 0u;                                       // bit r: U[r][lane] == m / and eligible
  for (int32_t r = 0; r < 32; ++r) {
    const uint32_t t_base = (uint32_t)(tw >> (2u * r)) & 3u;
    const int32_t s = (!my_n && t_base == my_base) ? 2 : -1;
    const int32_t ul = up(UT, 1u, lane, 0);
    const int32_t Un = max(0, (ul >> 1) + s);
    const int32_t Hg = up(X, 1u, lane, kNeg) + s;
    const int32_t H = max(Un, Hg);
    const int32_t E = max(max(up(H, 1u, lane, kNeg) - 20, up(H, 2u, lane, kNeg) - 40), up(H, 3u, lane, kNeg) - 60);
    const int32_t F = max(max(H1 - 20, H2 - 40), H3 - 60);
    const bool top = Un == m;
    if (col && r < la) {
      if (top) {
        tops |= 1u << r;
        if (!(ul & 1)) elig |= 1u << r;
      }
      g = max(g, Hg);
    }
    X = max(max(Hg, E), max(F, kNeg));
    H3 = H2;
    H2 = H1;
    H1 = H;
    UT = (Un << 1) | ((Un > 0 && ((ul & 1) || top)) ? 1 : 0);
  }
  const int32_t gmax = group_max(g);

  // X in the last column: the first row after a best cell of the last column whose upper-left neighbour is a best cell
  const uint32_t last_col = (uint32_t)__shfl((int32_t)tops, max(lb - 1, 0), 32);
  const uint32_t prev_col = lb >= 2 ? (uint32_t)__shfl((int32_t)tops, max(lb - 2, 0), 32) : 0u;
  int32_t row_cut = 32;                                                  // rows beyond row_cut come after X
  if (last_col) {
    const uint32_t from = prev_col & ~((1u << (__ffs(last_col) - 1)) - 1u);
    if (from) row_cut = __ffs(from);
  }
  // X in the last row: the same question of the lanes
  const uint32_t last_row = (uint32_t)(__ballot(la >= 1 && ((tops >> max(la - 1, 0)) & 1u)) >> half);
  const uint32_t prev_row = (uint32_t)(__ballot(la >= 2 && ((tops >> max(la - 2, 0)) & 1u)) >> half);
  uint32_t lane_cut = 32u;                                               // in the last row, lanes beyond lane_cut come after X
  if (last_row) {
    const uint32_t from = (prev_row << 1) & ~((2u << (__ffs(last_row) - 1)) - 1u) & bit_range(0, lb);
    if (from) lane_cut = (uint32_t)__ffs(from) - 1u;
  }
  uint32_t e = elig & bit_range(0, row_cut + 1);
  if (lane > lane_cut) e &= ~(1u << max(la - 1, 0));
  const int32_t key = group_max(e ? (((31 - __clz(e)) << 6) | (int32_t)lane) : -1);   // the largest (row, column)

  if (usable && gmax < m && key >= 0) {
    const int32_t d = (key >> 6) - (key & 63);
    uint32_t verdict, substring, edit;
    frame_answers(tw, rw, rn, la, lb, d, p.from_base, p.to_base, verdict, substring, edit);
    if (lane == 0u) {
      int4 out;
      out.x = (int32_t)(kA2iTied | (verdict << 8) | (substring << 9) | ((uint32_t)in.x & 0xFFFF0000u));
      out.y = d;
      out.z = (int32_t)edit;
      out.w = target;
      *reinterpret_cast<int4*>(p.rec + (uint64_t)row * kA2iRecInts) = out;
      atomicAdd(p.settled, 1u);
    }
  }
}

uint32_t grid_for(uint64_t n) { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((n + kBlock - 1) / kBlock, 1), 1u << 16); }

}  // namespace

hipError_t a2i_flags_launch(const int8_t* pass_id, const uint8_t* keep, uint64_t n, int32_t canon_pass, int32_t isomir_pass,
                            uint32_t* flags, hipStream_t stream) {
  hipLaunchKernelGGL(a2i_flags_kernel, dim3(grid_for(n)), dim3(kBlock), 0, stream, pass_id, keep, n, canon_pass, isomir_pass, flags);
  return hipGetLastError();
}

hipError_t a2i_scatter_launch(const int8_t* pass_id, const uint8_t* keep, uint64_t n, int32_t canon_pass, int32_t isomir_pass,
                              const uint32_t* off, uint64_t cap, uint32_t* idx, hipStream_t stream) {
  if (n == 0 || cap == 0) return hipSuccess;
  hipLaunchKernelGGL(a2i_scatter_kernel, dim3(grid_for(n)), dim3(kBlock), 0, stream, pass_id, keep, n, canon_pass, isomir_pass, off,
                     cap, idx);
  return hipGetLastError();
}

hipError_t a2i_align_launch(const A2iAlignParams& p, hipStream_t stream) {
  if (p.rows == 0) return hipSuccess;
  hipLaunchKernelGGL(a2i_align_kernel, dim3((p.rows + kPairsPerBlock - 1) / kPairsPerBlock), dim3(kBlock), 0, stream, p);
  return hipGetLastError();
}

hipError_t a2i_tied_select_launch(const int32_t* rec, uint64_t k, uint32_t* flags, hipStream_t stream) {
  hipLaunchKernelGGL(a2i_tied_flags_kernel, dim3(grid_for(k)), dim3(kBlock), 0, stream, rec, k, flags);
  return hipGetLastError();
}

hipError_t a2i_tied_scatter_launch(const int32_t* rec, uint64_t k, const uint32_t* off, uint32_t* sel, hipStream_t stream) {
  if (k == 0) return hipSuccess;
  hipLaunchKernelGGL(a2i_tied_scatter_kernel, dim3(grid_for(k)), dim3(kBlock), 0, stream, rec, k, off, sel);
  return hipGetLastError();
}

hipError_t a2i_settle_launch(const A2iSettleParams& p, hipStream_t stream) {
  if (p.n_sel == 0) return hipSuccess;
  hipLaunchKernelGGL(a2i_settle_kernel, dim3((p.n_sel + kPairsPerBlock - 1) / kPairsPerBlock), dim3(kBlock), 0, stream, p);
  return hipGetLastError();
}

}  // namespace mrg
