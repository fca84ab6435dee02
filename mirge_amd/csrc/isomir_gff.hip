// `-gff` on the device (mrg_isomir_classify, include/mirge_amd.h): which reads the GFF files list, in which order, and
// what each of them is.
//
// Replaces the per-read Python of updateIsomiRDic / updateIsomiRDic2 (runAnnotationPipeline.py:382-446) with its
// fillTerminal + analyzeAlignment (RAP:86-172, :237-339): mirge_amd/isomir.py restates those in coordinates on the
// precursor's axis, and classify_kernel restates isomir.classify_alignment, one lane per read.
//
// Everything the classification asks is a question about ONE bit mask, D: bit i set = read base i differs from the
// precursor's base at r0 + i (a position outside the precursor equals nothing).  The mature sequence sits in the
// precursor at [m0, m1), so "differs from mature" inside the overlap is D too, and the 5' / 3' extension tests are "any
// bit of D in front of m0 / behind m1".  D comes out of the packed words: the precursor's window at r0 is cut out of its
// 2-bit words by shifts, XORed with the read word, the bit pairs folded, the N planes added (read N = precursor N, N
// differs from every base) and the even bits squeezed into 32.  No per-base loop, nothing indexed in registers.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "isomir_gff.hpp"

namespace mrg {

namespace {

constexpr uint32_t kBlock = 256;
constexpr uint64_t kEven = 0x5555555555555555ull;

__global__ __launch_bounds__(kBlock) void iso_flags_kernel(const int8_t* __restrict__ pass_id, uint64_t n, int32_t canon_pass,
                                                           int32_t isomir_pass, uint32_t* __restrict__ flags) {
  const uint64_t step = (uint64_t)gridDim.x * kBlock;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += step) {
    const int32_t p = pass_id[i];
    flags[i] = p == canon_pass ? 1u : 0u;
    flags[n + i] = p == isomir_pass ? 1u : 0u;
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) flags[2 * n] = 0u;
}

__global__ __launch_bounds__(kBlock) void iso_scatter_kernel(const int8_t* __restrict__ pass_id, uint64_t n, int32_t canon_pass,
                                                             int32_t isomir_pass, const uint32_t* __restrict__ off, uint64_t cap,
                                                             uint32_t* __restrict__ idx) {
  const uint64_t step = (uint64_t)gridDim.x * kBlock;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += step) {
    const int32_t p = pass_id[i];
    if (p != canon_pass && p != isomir_pass) continue;
    const uint64_t o = off[p == canon_pass ? i : n + i];
    if (o < cap) idx[o] = (uint32_t)i;
  }
}

// bases x .. x + 31 of a packed text of nw words (zero outside it); x may be negative
__device__ __forceinline__ uint64_t window32(const uint64_t* __restrict__ t, int32_t nw, int32_t x) {
  const int32_t q = x >> 5;
  const uint32_t s = (uint32_t)(x & 31) * 2u;
  const uint64_t lo = (q >= 0 && q < nw) ? t[q] : 0ull;
  const uint64_t hi = (q + 1 >= 0 && q + 1 < nw) ? t[q + 1] : 0ull;
  return s ? (lo >> s) | (hi << (64u - s)) : lo;
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

__device__ __forceinline__ uint32_t snp_class(int32_t i) {
  if (i >= 1 && i <= 6) return 2u;
  if (i == 7) return 3u;
  if (i >= 8 && i <= 11) return 4u;
  if (i >= 12 && i <= 16) return 5u;
  return 1u;
}

__global__ __launch_bounds__(kBlock) void classify_kernel(const IsoClassifyParams p) {
  const uint32_t row = blockIdx.x * kBlock + threadIdx.x;
  if (row >= p.rows) return;
  const uint32_t read = p.idx[row];
  const bool canon = row < p.n_canon;
  const int32_t e = p.ref_id[read];
  const int32_t at = p.pos[read];
  const int32_t L = p.lens[read];
  int32_t* rec = p.rec + (uint64_t)row * kIsoRecInts;
  uint32_t* mask = p.mask + (uint64_t)row * 2u * p.mask_words;
  for (uint32_t w = 0; w < 2u * p.mask_words; ++w) mask[w] = 0u;
  int32_t pre_start = 0, pre_end = 0, iso5 = 0, iso3 = 0;
  uint32_t kind = kIsoBadEntry, snp = 0u, add = 0u, lead = 0u, trail = 0u;
  const bool usable = e >= 0 && (uint32_t)e < p.n_entries && at > -(1 << 24) && at < (1 << 24) && (uint32_t)L <= 32u * p.W;
  if (usable) {
    const int32_t* d = p.desc + (uint64_t)e * kIsoDescInts;
    const int32_t status = d[kIsoDescStatus];
    kind = status == 0 ? kIsoIsomir : status == 1 ? kIsoDropped : kIsoUnresolvable;
    if (status == 0) {
      const int32_t plen = d[kIsoDescLen], m0 = d[kIsoDescM0], m1 = m0 + d[kIsoDescMat];
      const int32_t nw = (plen + 31) >> 5;
      const uint64_t* text = p.text + (uint32_t)d[kIsoDescOff];
      const uint64_t* npl = p.nplane + (uint32_t)d[kIsoDescOff];
      const int32_t e0 = m0 - 2;
      const int32_t r0 = e0 + at - (canon ? 0 : 1), r1 = r0 + L;
      const int32_t frame0 = canon ? min(0, e0) : min(min(0, e0), r0);
      const int32_t ov_lo = max(m0, r0) - r0, ov_hi = min(m1, r1) - r0;        // read n mature
      const int32_t x5 = r0 < m0 ? min(m0 - r0, L) : 0;                        // 5' extension: [0, x5)
      const int32_t y3 = r1 > m1 ? max(m1 - r0, 0) : L;                        // 3' extension: [y3, L)
      uint32_t any = 0u, any5 = 0u, any3 = 0u;
      int32_t first = -1;
      for (int32_t w = 0; 32 * w < L; ++w) {
        const uint64_t at_w = (uint64_t)w * p.stride + read;
        const uint64_t rn = p.nmask ? (p.nmask[at_w] & kEven) : 0ull;
        const uint64_t R = p.reads[at_w] & ~(rn * 3ull);
        const uint64_t P = window32(text, nw, r0 + 32 * w);
        const uint64_t pn = window32(npl, nw, r0 + 32 * w);
        uint64_t dd = R ^ P;
        dd = (dd | (dd >> 1)) | (rn ^ pn);
        const uint32_t inside = bit_range(-r0 - 32 * w, plen - r0 - 32 * w);
        const uint32_t m = ((squeeze_even(dd) & inside) | ~inside) & bit_range(0, L - 32 * w);
        mask[w] = m;
        any |= m;
        const uint32_t ov = m & bit_range(ov_lo - 32 * w, ov_hi - 32 * w);
        if (first < 0 && ov) first = 32 * w + (int32_t)__builtin_ctz(ov);
        any5 |= m & bit_range(-32 * w, x5 - 32 * w);
        any3 |= m & bit_range(y3 - 32 * w, L - 32 * w);
      }
      pre_start = r0 + 1;
      pre_end = r1;
      lead = (uint32_t)min(max(-r0, 0), L);
      trail = (uint32_t)min(max(r1 - plen, 0), L - (int32_t)lead);
      if (r0 == m0 && r1 == m1 && !any) {
        kind = kIsoRef;
      } else {
        if (first >= 0) snp = snp_class(r0 + first - frame0);
        if (r0 != m0) iso5 = m0 - r0;
        // (a read that ends in front of mature leaves precursor bases of the extension uncovered: they differ too)
        if (r0 < m0 && (any5 || max(r1, 0) < m0)) snp = 1u;
        if (r1 != m1) iso3 = r1 - m1;
        if (r1 > m1 && (any3 || (r0 > m1 && m1 < min(r0, plen)))) add = 1u;
      }
    }
  }
  rec[kIsoRecStart] = pre_start;
  rec[kIsoRecEnd] = pre_end;
  rec[kIsoRec5p] = iso5;
  rec[kIsoRec3p] = iso3;
  rec[kIsoRecFlags] = (int32_t)(kind | (snp << 8) | (add << 16));
  rec[kIsoRecEnds] = (int32_t)(lead | (trail << 16));
  rec[kIsoRecEntry] = e;
  rec[7] = 0;
}

uint32_t grid_for(uint64_t n) { return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((n + kBlock - 1) / kBlock, 1), 1u << 16); }

}  // namespace

hipError_t iso_flags_launch(const int8_t* pass_id, uint64_t n, int32_t canon_pass, int32_t isomir_pass, uint32_t* flags,
                            hipStream_t stream) {
  hipLaunchKernelGGL(iso_flags_kernel, dim3(grid_for(n)), dim3(kBlock), 0, stream, pass_id, n, canon_pass, isomir_pass, flags);
  return hipGetLastError();
}

hipError_t iso_scatter_launch(const int8_t* pass_id, uint64_t n, int32_t canon_pass, int32_t isomir_pass, const uint32_t* off,
                              uint64_t cap, uint32_t* idx, hipStream_t stream) {
  if (n == 0 || cap == 0) return hipSuccess;
  hipLaunchKernelGGL(iso_scatter_kernel, dim3(grid_for(n)), dim3(kBlock), 0, stream, pass_id, n, canon_pass, isomir_pass, off, cap,
                     idx);
  return hipGetLastError();
}

hipError_t iso_classify_launch(const IsoClassifyParams& p, hipStream_t stream) {
  if (p.rows == 0) return hipSuccess;
  hipLaunchKernelGGL(classify_kernel, dim3((p.rows + kBlock - 1) / kBlock), dim3(kBlock), 0, stream, p);
  return hipGetLastError();
}

}  // namespace mrg
