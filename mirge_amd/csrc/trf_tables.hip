// `-trf` on the device (mrg_trf_classify, include/mirge_amd.h): which reads the tRF tables list, what each of their
// alignments is (trfTypes, runAnnotationPipeline.py:448-474), which tRNA a read is counted for and which predefined tRF
// it is nearest to (assign_cluster / getDistance2, writeDataToCSV.py:373-392, :546-564).  mirge_amd/trf.py holds the
// Python these kernels restate; capi.hip strings them together with the listing (mrg_list_best_*) and the sort.
//
// trf_assign_kernel never builds a dashed string.  add_dash_new(read, length, start + 1, end + 1) is `start` dashes, the
// read and max(length - end - 1, 0) dashes, so its coordinate() is (start + 1, start + len(read)) whatever the T tail of a
// trailer read does to `end`; the substitutions are the read's bases that differ from the predefined string at start + i,
// a dash of that string equal to everything and a position behind its end equal to nothing.  The predefined strings are
// packed whole, dashes included (a dash plane beside the N plane), so one window cut out of two adjacent words by shifts,
// XORed with the read word, folded and masked gives 32 positions at once; __popcll counts them.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "trf_tables.hpp"

namespace mrg {

namespace {

constexpr uint32_t kBlock = 256;
constexpr uint64_t kEven = 0x5555555555555555ull;

__device__ __forceinline__ uint64_t low_pairs(int32_t bases) {  // the bit pairs of bases [0, bases), bases anywhere
  return bases <= 0 ? 0ull : bases >= 32 ? ~0ull : (1ull << (2 * bases)) - 1ull;
}

// bases x .. x + 31 of a packed text of nw words (zero outside it); x >= 0
__device__ __forceinline__ uint64_t window32(const uint64_t* __restrict__ t, int32_t nw, int32_t x) {
  const int32_t q = x >> 5;
  const uint32_t s = (uint32_t)(x & 31) * 2u;
  const uint64_t lo = q < nw ? t[q] : 0ull;
  const uint64_t hi = q + 1 < nw ? t[q + 1] : 0ull;
  return s ? (lo >> s) | (hi << (64u - s)) : lo;
}

__global__ __launch_bounds__(kBlock) void trf_gather_kernel(const TrfGatherParams p) {
  const uint32_t row = blockIdx.x * kBlock + threadIdx.x;
  if (row >= p.k) return;
  const uint32_t read = p.idx[row];
  const int32_t L = min((int32_t)p.lens[read], 32 * (int32_t)p.W);
  const bool trailer = row >= p.n_mature;
  int32_t tail = 0;
  if (trailer) {
    // trailing T's: from the last word down, the highest base that is no T (code 3, and no N) ends the run
    bool open = true;
    for (int32_t w = (int32_t)p.W - 1; w >= 0; --w) {
      const int32_t c = min(L - 32 * w, 32);
      if (c <= 0 || !open) continue;
      const uint64_t at = (uint64_t)w * p.stride + read;
      uint64_t x = ~p.reads[at];
      x = (x | (x >> 1)) & kEven;                     // a base that is not T
      if (p.nmask) x |= p.nmask[at] & kEven;          // (N is stored as code 0 under its mask bit)
      x &= low_pairs(c);
      if (x) {
        tail += c - 1 - ((63 - __clzll((long long)x)) >> 1);
        open = false;
      } else {
        tail += c;
      }
    }
  }
  // strip_poly_t: at least 3 T's cut off and at least 11 nt left, else the read has no stripped sequence
  const bool ok = !trailer || (tail >= 3 && L - tail >= 11);
  const int32_t sub = ok ? L - tail : 0;
  p.sub_len[row] = (uint8_t)sub;
  p.tail[row] = (uint8_t)tail;
  const uint32_t n_b = p.k - p.n_mature;
  const uint64_t out_stride = trailer ? n_b : p.n_mature;
  const uint64_t out_row = trailer ? row - p.n_mature : row;
  uint64_t* words = trailer ? p.words_b : p.words_a;
  uint64_t* nm = trailer ? p.nmask_b : p.nmask_a;
  for (uint32_t w = 0; w < p.W; ++w) {
    const uint64_t at = (uint64_t)w * p.stride + read;
    const uint64_t keep = low_pairs(sub - 32 * (int32_t)w);
    words[(uint64_t)w * out_stride + out_row] = p.reads[at] & keep;
    if (p.nmask) nm[(uint64_t)w * out_stride + out_row] = p.nmask[at] & keep;
  }
}

__global__ __launch_bounds__(kBlock) void trf_keys_kernel(const uint64_t* __restrict__ off, const int32_t* __restrict__ ref,
                                                          const int32_t* __restrict__ pos, uint32_t n_rows, uint32_t row0, uint32_t entry0,
                                                          uint32_t entry_bits, uint32_t pos_bits, uint64_t out0, uint64_t* __restrict__ keys) {
  const uint32_t r = blockIdx.x * kBlock + threadIdx.x;
  if (r >= n_rows) return;
  const uint64_t emask = (1ull << entry_bits) - 1ull, pmask = (1ull << pos_bits) - 1ull;
  const uint64_t owner = (uint64_t)(row0 + r) << (entry_bits + pos_bits);
  // (a value that does not fit its field saturates it: trf_type_kernel reports such a row as out of range)
  for (uint64_t j = off[r]; j < off[r + 1]; ++j) {
    const int64_t e = (int64_t)ref[j] + (ref[j] < 0 ? 0 : (int64_t)entry0), at = pos[j];
    const uint64_t ef = e < 0 || (uint64_t)e > emask ? emask : (uint64_t)e;
    const uint64_t pf = at < 0 || (uint64_t)at > pmask ? pmask : (uint64_t)at;
    keys[out0 + j] = owner | (ef << pos_bits) | pf;
  }
}

__global__ __launch_bounds__(kBlock) void trf_heads_kernel(const uint64_t* __restrict__ keys, uint32_t n, uint32_t pos_bits,
                                                           uint32_t* __restrict__ head) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i > n) return;
  head[i] = i == n ? 0u : (i == 0 || (keys[i] >> pos_bits) != (keys[i - 1] >> pos_bits)) ? 1u : 0u;
}

// One lane per alignment of the sorted listing; the lanes of kept alignments (the lowest offset of an (owner, entry) run)
// write.  trfTypes in integer comparisons.
__global__ __launch_bounds__(kBlock) void trf_type_kernel(const TrfTypeParams p) {
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= p.n_keys) return;
  const uint32_t slot = p.slot[i];
  const bool head = p.slot[i + 1] != slot;
  const uint64_t key = p.keys[i];
  const uint32_t owner = (uint32_t)(key >> (p.entry_bits + p.pos_bits));
  if (owner >= p.k) return;
  const uint32_t next_owner = i + 1 < p.n_keys ? (uint32_t)(p.keys[i + 1] >> (p.entry_bits + p.pos_bits)) : 0xFFFFFFFFu;
  const uint32_t prev_owner = i ? (uint32_t)(p.keys[i - 1] >> (p.entry_bits + p.pos_bits)) : 0xFFFFFFFFu;
  if (prev_owner != owner) p.hit0[owner] = slot;                      // (the first alignment of an owner is a head)
  if (next_owner != owner) p.hit1[owner] = slot + (head ? 1u : 0u);   // (one past the owner's last kept alignment)
  if (!head) return;
  const uint32_t e = (uint32_t)(key >> p.pos_bits) & ((1u << p.entry_bits) - 1u);
  const int32_t start = (int32_t)(key & ((1ull << p.pos_bits) - 1ull));
  const int32_t L = p.lens[p.idx[owner]], tail = p.tail[owner];
  uint32_t type = kTrfTypeRange;
  if (e < p.n_entries && start < (1 << 24) && (uint64_t)start != (1ull << p.pos_bits) - 1ull) {
    const int32_t* d = p.desc + (uint64_t)e * kTrfDescInts;
    const int32_t flags = d[kTrfDescFlags];
    if (flags & 2) {
      type = kTrfTypeUnresolvable;
    } else if (flags & 1) {
      type = kTrfType1;
    } else {
      const int32_t n = d[kTrfDescTypeLen], anticodon = d[kTrfDescAnticodon], last = start + L - 1;
      if (start == 0)
        type = L == n ? kTrfTypeWhole : (anticodon - 2 <= last && last <= anticodon + 1) ? kTrfType5Half : kTrfType5;
      else if (n - 3 <= last && last <= n - 1)
        type = (anticodon - 1 <= start && start <= anticodon + 2) ? kTrfType3Half : kTrfType3;
      else
        type = kTrfTypeI;
    }
  }
  int32_t* out = p.hits + (uint64_t)slot * kTrfHitInts;
  out[0] = (int32_t)e;
  out[1] = start;
  out[2] = start + L - 1 - tail;
  out[3] = (int32_t)type;
}

// One lane per selected read: the tRNA it is counted for (the smallest de-duplicated name among its alignments) and
// assign_cluster against that tRNA's predefined tRFs.
__global__ __launch_bounds__(kBlock) void trf_assign_kernel(const TrfAssignParams p) {
  const uint32_t row = blockIdx.x * kBlock + threadIdx.x;
  if (row >= p.k) return;
  const uint32_t read = p.idx[row];
  const int32_t L = p.lens[read];
  const uint32_t h0 = p.hit0[row], h1 = p.hit1[row];
  int32_t sel = -1, start = 0, end = 0, type = 0, cluster = -1, distance = 0;
  uint32_t kind = kTrfNoCandidate;
  if (row >= p.n_mature && p.sub_len[row] == 0) kind = kTrfRange;   // (the Python route fails on strip_poly_t's None)
  if ((uint32_t)L > 32u * p.W) kind = kTrfRange;
  if (kind == kTrfNoCandidate && h1 > h0) {
    // selected = min(unique): the smallest rank of a de-duplicated name, then that name's own alignment
    int32_t best_rank = 0x7FFFFFFF;
    bool bad_type = false, bad_range = false;
    for (uint32_t h = h0; h < h1; ++h) {
      const int32_t* hit = p.hits + (uint64_t)h * kTrfHitInts;
      bad_range |= hit[3] == (int32_t)kTrfTypeRange;
      bad_type |= hit[3] == (int32_t)kTrfTypeUnresolvable;
      if (hit[3] >= (int32_t)kTrfTypeUnresolvable) continue;
      const int32_t* d = p.desc + (uint64_t)hit[0] * kTrfDescInts;
      if (d[kTrfDescRank] < best_rank) {
        best_rank = d[kTrfDescRank];
        sel = d[kTrfDescRep];
      }
    }
    bool found = false;
    for (uint32_t h = h0; h < h1; ++h) {
      const int32_t* hit = p.hits + (uint64_t)h * kTrfHitInts;
      if (hit[0] == sel && hit[3] < (int32_t)kTrfTypeUnresolvable) {
        found = true;
        start = hit[1];
        end = hit[2];
        type = hit[3];
      }
    }
    if (!found) sel = -1;   // (the de-duplicated name is no alignment of this read: `rec[selected]` fails)
    const int32_t* d = found && (uint32_t)sel < p.n_entries ? p.desc + (uint64_t)sel * kTrfDescInts : nullptr;
    if (bad_range) {
      kind = kTrfRange;
    } else if (bad_type || !d || d[kTrfDescTemplate] < 0) {
      kind = kTrfUnresolvable;   // (the representative is no alignment of this read, or a table lacks the name)
    } else if (d[kTrfDescCount] == 0) {
      kind = kTrfDele;
      distance = 100;
    } else {
      // get_distance2 against every predefined tRF of the tRNA; the minimum by (distance, name rank)
      const int32_t c1_first = start + 1, c1_last = start + L;
      int32_t best_d = 0x7FFFFFFF, best_r = 0x7FFFFFFF;
      const uint32_t t0 = (uint32_t)d[kTrfDescFirst], t1 = t0 + (uint32_t)d[kTrfDescCount];
      for (uint32_t t = t0; t < t1 && t < p.n_clusters; ++t) {
        const int32_t* c = p.clusters + (uint64_t)t * kTrfClusterInts;
        const int32_t tl = c[kTrfClusterLen], nw = (tl + 31) >> 5;
        const uint64_t* text = p.text + (uint32_t)c[kTrfClusterWord];
        const uint64_t* plane = p.plane + (uint32_t)c[kTrfClusterWord];
        int32_t dist = abs(c1_first - c[kTrfClusterFirst]) + abs(c1_last - c[kTrfClusterLast]);
        for (int32_t w = 0; 32 * w < L; ++w) {
          const uint64_t at_w = (uint64_t)w * p.stride + read;
          const uint64_t rn = p.nmask ? (p.nmask[at_w] & kEven) : 0ull;
          const uint64_t R = p.reads[at_w] & ~(rn * 3ull);
          const int32_t x = start + 32 * w;
          const uint64_t P = window32(text, nw, x), pl = window32(plane, nw, x);
          uint64_t dd = R ^ P;
          dd = ((dd | (dd >> 1)) | (rn ^ pl)) & kEven & ~(pl >> 1);   // differs, and the predefined string has no dash there
          const uint64_t inside = low_pairs(tl - x);                   // a base behind the predefined string counts as one
          dist += __popcll(((dd & inside) | (~inside & kEven)) & low_pairs(L - 32 * w));
        }
        const int32_t r = c[kTrfClusterRank];
        if (dist < best_d || (dist == best_d && r < best_r)) {
          best_d = dist;
          best_r = r;
          cluster = (int32_t)t;
        }
      }
      distance = best_d;
      kind = best_d <= 8 ? kTrfAssigned : kTrfUndef;
    }
  }
  int32_t* rec = p.rec + (uint64_t)row * kTrfRecInts;
  rec[kTrfRecRead] = (int32_t)read;
  rec[kTrfRecEntry] = sel;
  rec[kTrfRecStart] = start;
  rec[kTrfRecEnd] = end;
  rec[kTrfRecType] = type;
  rec[kTrfRecCluster] = cluster;
  rec[kTrfRecDistance] = distance;
  rec[kTrfRecKind] = (int32_t)kind;
  rec[kTrfRecHit0] = (int32_t)h0;
  rec[kTrfRecHits] = (int32_t)(h1 - h0);
  rec[kTrfRecTail] = p.tail[row];
  rec[11] = 0;
}

dim3 grid_for(uint64_t n) { return dim3((uint32_t)((n + kBlock - 1) / kBlock)); }

}  // namespace

hipError_t trf_gather_launch(const TrfGatherParams& p, hipStream_t stream) {
  if (p.k == 0) return hipSuccess;
  hipLaunchKernelGGL(trf_gather_kernel, grid_for(p.k), dim3(kBlock), 0, stream, p);
  return hipGetLastError();
}

hipError_t trf_keys_launch(const uint64_t* off, const int32_t* ref, const int32_t* pos, uint32_t n_rows, uint32_t row0, uint32_t entry0,
                           uint32_t entry_bits, uint32_t pos_bits, uint64_t out0, uint64_t* keys, hipStream_t stream) {
  if (n_rows == 0) return hipSuccess;
  hipLaunchKernelGGL(trf_keys_kernel, grid_for(n_rows), dim3(kBlock), 0, stream, off, ref, pos, n_rows, row0, entry0, entry_bits,
                     pos_bits, out0, keys);
  return hipGetLastError();
}

hipError_t trf_heads_launch(const uint64_t* keys, uint32_t n, uint32_t pos_bits, uint32_t* head, hipStream_t stream) {
  hipLaunchKernelGGL(trf_heads_kernel, grid_for((uint64_t)n + 1), dim3(kBlock), 0, stream, keys, n, pos_bits, head);
  return hipGetLastError();
}

hipError_t trf_type_launch(const TrfTypeParams& p, hipStream_t stream) {
  if (p.n_keys == 0) return hipSuccess;
  hipLaunchKernelGGL(trf_type_kernel, grid_for(p.n_keys), dim3(kBlock), 0, stream, p);
  return hipGetLastError();
}

hipError_t trf_assign_launch(const TrfAssignParams& p, hipStream_t stream) {
  if (p.k == 0) return hipSuccess;
  hipLaunchKernelGGL(trf_assign_kernel, grid_for(p.k), dim3(kBlock), 0, stream, p);
  return hipGetLastError();
}

}  // namespace mrg
