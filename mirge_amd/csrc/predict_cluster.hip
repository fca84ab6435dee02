// Predict mode's location clusters (reference utils/cluster_basedon_location.py) from the genome listing's rows, which
// stay on the device: gfx950, wave64.
//
// The reference walks a coordinate-sorted SAM file: per chromosome and strand, an alignment [s, e] joins the cluster in
// front of it iff it starts inside it with at least t bases of overlap, and then extends the cluster's sequence by its
// own tail.  With the rows of an (entry, strand) list in position order that is
//     joins  <=>  P - s + 1 >= t        P = the largest e of ALL earlier rows of the list,
// and a joining row extends the sequence iff e > P, by SEQ[P - s + 1 :].  (A cluster that ends before P can only be a
// single row: a row that started within t bases of P's end would have joined P's own cluster.)  So, per run:
//   cluster_keys_kernel    (entry, strand, position) keys of the rows of every part; prims::radix_sort_pairs_u64 sorts;
//   cluster_rows_kernel    e of every sorted row, the list heads, the rows' reads;
//   prims::segmented_inclusive_max_u32 of e over the lists;
//   cluster_heads_kernel   the rows that open a cluster; prims::inclusive_sum_u32 numbers the clusters;
//   cluster_bounds_kernel  entry, strand, start, end, first row and length of every cluster;
//   cluster_assemble_kernel  every row writes the bases it contributes -- each base of a cluster's sequence has exactly
//                          one writer -- and adds its read's count to its cluster's sum.
// Rows of an entry the caller masks out (names without "chr") get an entry number behind all others: they sort to the
// end and never enter a list.
#include "predict_cluster.hpp"

namespace mrg {

namespace {

constexpr uint32_t kThreads = 256u;

__device__ __forceinline__ uint32_t key_entry(uint64_t k, uint32_t pos_bits) { return (uint32_t)(k >> (pos_bits + 1u)); }
__device__ __forceinline__ uint32_t key_pos(uint64_t k, uint32_t pos_bits) { return (uint32_t)(k & ((1ull << pos_bits) - 1ull)); }
__device__ __forceinline__ uint32_t key_strand(uint64_t k, uint32_t pos_bits) { return (uint32_t)(k >> pos_bits) & 1u; }

__global__ void __launch_bounds__(kThreads) cluster_keys_kernel(ClusterKeysArgs a) {
  const uint32_t k = blockIdx.x * kThreads + threadIdx.x;
  if (k >= a.rows) return;
  // the read r with offsets[r] <= k < offsets[r + 1]
  uint64_t lo = 0, hi = a.n_reads;
  while (hi - lo > 1) {
    const uint64_t mid = (lo + hi) >> 1;
    if (a.offsets[mid] <= k) lo = mid;
    else hi = mid;
  }
  uint64_t e = (uint64_t)a.entry_base + (uint32_t)a.ref[k];
  if (e >= a.n_entries || (a.entry_keep && !a.entry_keep[e])) e = a.n_entries;
  const uint64_t p = (uint32_t)a.pos[k] & ((1ull << a.pos_bits) - 1ull), s = a.strand[k] ? 1ull : 0ull;
  const uint64_t at = (uint64_t)a.row_base + k;
  a.keys[at] = a.order == kSamOrder ? (e << (a.pos_bits + 1u)) | (p << 1) | s : (e << (a.pos_bits + 1u)) | (s << a.pos_bits) | p;
  a.vals[at] = (uint32_t)at;
  a.owner[at] = (uint32_t)lo;
}

__global__ void __launch_bounds__(kThreads) cluster_rows_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                                uint32_t rows, const uint32_t* __restrict__ owner,
                                                                const uint8_t* __restrict__ lens, uint32_t n_entries, uint32_t pos_bits,
                                                                ClusterWork w, uint32_t* __restrict__ member) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= rows) return;
  const uint64_t k = keys[i];
  const uint32_t r = owner[vals[i]];
  member[i] = r;
  w.end[i] = key_pos(k, pos_bits) + (uint32_t)lens[r];  // 0-based start + length = 1-based inclusive end
  const bool valid = key_entry(k, pos_bits) < n_entries;
  bool prev_valid = true, head = true;
  if (i) {
    const uint64_t kp = keys[i - 1];
    prev_valid = key_entry(kp, pos_bits) < n_entries;
    head = (kp >> pos_bits) != (k >> pos_bits);
  }
  w.lhead[i] = head ? 1 : 0;
  if (!valid && prev_valid) *w.n_valid = i;
  if (valid && i == rows - 1u) *w.n_valid = rows;
}

__global__ void __launch_bounds__(kThreads) cluster_heads_kernel(const uint64_t* __restrict__ keys, uint32_t rows, uint32_t n_entries,
                                                                 uint32_t pos_bits, int32_t t, ClusterWork w) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= rows) return;
  const uint64_t k = keys[i];
  uint32_t h = 0;
  if (key_entry(k, pos_bits) < n_entries) {
    h = 1;
    if (!w.lhead[i]) {
      const int64_t P = w.runmax[i - 1], s = (int64_t)key_pos(k, pos_bits) + 1;
      if (s <= P && P - s + 1 >= (int64_t)t) h = 0;
    }
  }
  w.chead[i] = h;
}

__global__ void __launch_bounds__(kThreads) cluster_bounds_kernel(const uint64_t* __restrict__ keys, uint32_t pos_bits, ClusterWork w,
                                                                  ClusterTable c) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i == 0) {
    c.member_off[c.n_clusters] = c.n_valid;
    c.len[c.n_clusters] = 0u;
  }
  if (i >= c.n_valid || !w.chead[i]) return;
  const uint32_t id = w.cinc[i] - 1u;
  if (id >= c.n_clusters) return;
  // the cluster's rows are [i, j): j = the next cluster head
  uint32_t j = i + 1u;
  while (j < c.n_valid && !w.chead[j]) ++j;
  const uint64_t k = keys[i];
  const uint32_t start = key_pos(k, pos_bits) + 1u;
  const uint32_t end = j - i == 1u ? w.end[i] : w.runmax[j - 1u];
  c.entry[id] = key_entry(k, pos_bits);
  c.strand[id] = (uint8_t)key_strand(k, pos_bits);
  c.start[id] = start;
  c.end[id] = end;
  c.member_off[id] = i;
  c.len[id] = end - start + 1u;
}

__global__ void __launch_bounds__(kThreads) cluster_assemble_kernel(ClusterAssembleArgs a, ClusterWork w, ClusterTable c) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= c.n_valid) return;
  const uint32_t id = w.cinc[i] - 1u;
  if (id >= c.n_clusters) return;
  const uint32_t r = a.member[i];
  if (r >= a.n_reads) return;
  atomicAdd(&a.sum[id], (unsigned long long)a.counts[r]);
  const uint64_t k = a.keys[i];
  const uint32_t s = key_pos(k, a.pos_bits) + 1u, L = a.lens[r], e = w.end[i];
  uint32_t from = 0, dst = 0;  // SEQ[from:] goes to the cluster's sequence at dst
  if (!w.chead[i]) {
    const uint32_t P = w.runmax[i - 1u];
    if (e <= P) return;
    from = P - s + 1u;
    dst = P - c.start[id] + 1u;
  }
  const uint64_t base = a.seq_off[id];
  const uint32_t room = (uint32_t)(a.seq_off[id + 1u] - base);
  const bool minus = key_strand(k, a.pos_bits) != 0u;
  uint32_t have = ~0u;  // the word in `word` / `nm`
  uint64_t word = 0, nm = 0;
  for (uint32_t j = from; j < L && dst < room; ++j, ++dst) {
    const uint32_t q = minus ? L - 1u - j : j;  // SEQ is the reverse complement of the read on the - strand
    if ((q >> 5) != have) {
      have = q >> 5;
      if (have >= a.words) return;
      word = a.reads[(uint64_t)have * a.n_reads + r];
      nm = a.nmask ? a.nmask[(uint64_t)have * a.n_reads + r] : 0ull;
    }
    const uint32_t sh = (q & 31u) * 2u;
    uint32_t code = (uint32_t)(word >> sh) & 3u;
    if (minus) code = 3u - code;
    a.seq[base + dst] = ((nm >> sh) & 1ull) ? 'N' : (char)((0x54474341u >> (code * 8u)) & 0xffu);  // "ACGT"
  }
}

__global__ void __launch_bounds__(kThreads) cluster_gather_kernel(const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                                  uint32_t rows, uint32_t pos_bits, int32_t order,
                                                                  const uint32_t* __restrict__ owner, const uint8_t* __restrict__ mm,
                                                                  uint32_t* __restrict__ out_read, int32_t* __restrict__ out_entry,
                                                                  int32_t* __restrict__ out_pos, uint8_t* __restrict__ out_strand,
                                                                  uint8_t* __restrict__ out_mm) {
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= rows) return;
  const uint64_t k = keys[i];
  const uint32_t row = vals[i];
  out_read[i] = owner[row];
  out_entry[i] = (int32_t)key_entry(k, pos_bits);
  if (order == kSamOrder) {
    out_pos[i] = (int32_t)((k >> 1) & ((1ull << pos_bits) - 1ull));
    out_strand[i] = (uint8_t)(k & 1ull);
  } else {
    out_pos[i] = (int32_t)key_pos(k, pos_bits);
    out_strand[i] = (uint8_t)key_strand(k, pos_bits);
  }
  out_mm[i] = mm[row];
}

inline uint32_t blocks_for(uint32_t n) { return (n + kThreads - 1u) / kThreads; }

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

size_t cluster_work_bytes(uint64_t rows) { return 4 * align256(rows * 4) + align256(rows) + 256; }

ClusterWork cluster_work(void* buf, uint64_t rows) {
  char* p = (char*)buf;
  const size_t a4 = align256(rows * 4);
  ClusterWork w;
  w.end = (uint32_t*)p;
  w.runmax = (uint32_t*)(p + a4);
  w.chead = (uint32_t*)(p + 2 * a4);
  w.cinc = (uint32_t*)(p + 3 * a4);
  w.lhead = (uint8_t*)(p + 4 * a4);
  w.n_valid = (uint64_t*)(p + 4 * a4 + align256(rows));
  return w;
}

hipError_t cluster_keys_launch(const ClusterKeysArgs& a, hipStream_t stream) {
  if (!a.rows) return hipSuccess;
  hipLaunchKernelGGL(cluster_keys_kernel, dim3(blocks_for(a.rows)), dim3(kThreads), 0, stream, a);
  return hipGetLastError();
}

hipError_t cluster_rows_launch(const uint64_t* keys, const uint32_t* vals, uint32_t rows, const uint32_t* owner, const uint8_t* lens,
                               uint32_t n_entries, uint32_t pos_bits, const ClusterWork& w, uint32_t* member, hipStream_t stream) {
  if (!rows) return hipSuccess;
  hipLaunchKernelGGL(cluster_rows_kernel, dim3(blocks_for(rows)), dim3(kThreads), 0, stream, keys, vals, rows, owner, lens, n_entries,
                     pos_bits, w, member);
  return hipGetLastError();
}

hipError_t cluster_heads_launch(const uint64_t* keys, uint32_t rows, uint32_t n_entries, uint32_t pos_bits, int32_t t, const ClusterWork& w,
                                hipStream_t stream) {
  if (!rows) return hipSuccess;
  hipLaunchKernelGGL(cluster_heads_kernel, dim3(blocks_for(rows)), dim3(kThreads), 0, stream, keys, rows, n_entries, pos_bits, t, w);
  return hipGetLastError();
}

hipError_t cluster_bounds_launch(const uint64_t* keys, uint32_t pos_bits, const ClusterWork& w, const ClusterTable& c, hipStream_t stream) {
  hipLaunchKernelGGL(cluster_bounds_kernel, dim3(blocks_for(c.n_valid ? c.n_valid : 1u)), dim3(kThreads), 0, stream, keys, pos_bits, w, c);
  return hipGetLastError();
}

hipError_t cluster_assemble_launch(const ClusterAssembleArgs& a, const ClusterWork& w, const ClusterTable& c, hipStream_t stream) {
  if (!c.n_valid) return hipSuccess;
  hipLaunchKernelGGL(cluster_assemble_kernel, dim3(blocks_for(c.n_valid)), dim3(kThreads), 0, stream, a, w, c);
  return hipGetLastError();
}

hipError_t cluster_gather_launch(const uint64_t* keys, const uint32_t* vals, uint32_t rows, uint32_t pos_bits, int32_t order,
                                 const uint32_t* owner, const uint8_t* mm, uint32_t* out_read, int32_t* out_entry, int32_t* out_pos,
                                 uint8_t* out_strand, uint8_t* out_mm, hipStream_t stream) {
  if (!rows) return hipSuccess;
  hipLaunchKernelGGL(cluster_gather_kernel, dim3(blocks_for(rows)), dim3(kThreads), 0, stream, keys, vals, rows, pos_bits, order, owner, mm,
                     out_read, out_entry, out_pos, out_strand, out_mm);
  return hipGetLastError();
}

}  // namespace mrg
