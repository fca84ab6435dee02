// C-ABI of include/mirge_amd.h: handle management, HBM residency of the
// libraries, the cascade driver (one match launch per bowtie command line of
// RAP:577-599 / RAP:688, survivor lists kept on device) and the tally launch.
#include <hip/hip_runtime.h>

#include <dlfcn.h>
#include <rccl/rccl.h>  // types and enums only: the library is bound at run time (see RcclApi)

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/mirge_amd.h"
#include "dict_index.hpp"
#include "pgzip.hpp"
#include "fastq.hpp"
#include "fm_index.hpp"
#include "a2i_align.hpp"
#include "collapsed_order.hpp"
#include "predict_remap.hpp"
#include "predict_trim.hpp"
#include "isomir_gff.hpp"
#include "kernels.hpp"
#include "predict_cluster.hpp"
#include "predict_features.hpp"
#include "predict_precursors.hpp"
#include "predict_reads.hpp"
#include "predict_report.hpp"
#include "predict_screen.hpp"
#include "predict_svm.hpp"
#include "prims.hpp"
#include "sa_build.hpp"
#include "tables.hpp"
#include "trf_groups.hpp"
#include "trf_labels.hpp"
#include "trf_peaks.hpp"
#include "trf_tables.hpp"

struct mrg_index {
  mutable mrg::FmIndex ix;
  // A large library's jump tables and row context are built when somebody needs them on the HOST (mrg_index_get_view, a
  // context without `device_tables`): fm_index.hpp, derive_tables.
  mutable std::mutex derive_mutex;
  const mrg::FmIndex& derived() const {
    std::lock_guard<std::mutex> g(derive_mutex);
    mrg::derive_tables(ix);
    return ix;
  }
  // exact-match dictionaries by key length, built on first request (mrg_index_get_dict,
  // mrg_ctx_add_library) and kept for the life of the index
  mutable std::map<uint32_t, mrg::ExactDict> dicts;
  mutable std::mutex dict_mutex;
  const mrg::ExactDict& dict(uint32_t key_bases) const {
    std::lock_guard<std::mutex> g(dict_mutex);
    auto it = dicts.find(key_bases);
    if (it == dicts.end()) {
      mrg::ExactDict d;
      mrg::build_exact_dict(ix, key_bases, d);
      it = dicts.emplace(key_bases, std::move(d)).first;
    }
    return it->second;
  }
  void drop_dict(uint32_t key_bases) const {  // (a large library's slot array is gigabytes: not kept on the host once uploaded)
    std::lock_guard<std::mutex> g(dict_mutex);
    dicts.erase(key_bases);
  }
};
struct mrg_fastq {
  mrg::FastqData d;
};
struct mrg_gz {
  std::unique_ptr<mrg::GzipReader> rd;
};

namespace {

thread_local std::string g_err;
thread_local uint32_t g_device_build_rounds = 0;  // mrg_index_build_device_rounds

int fail(int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIP_TRY(expr)                                                              \
  do {                                                                             \
    hipError_t e_ = (expr);                                                        \
    if (e_ != hipSuccess)                                                          \
      return fail(MRG_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                  __FILE__, __LINE__);                                             \
  } while (0)

// ---- a stage's scratch: one buffer, carved in a fixed order into typed pieces ----
// A piece of a layout: where it starts, and of what.  at(base) is the only way to a pointer.
template <class T>
struct Piece {
  size_t off = 0;
  T* at(void* base) const { return reinterpret_cast<T*>(static_cast<char*>(base) + off); }
};
// Hands out the pieces of one layout in order.  A piece takes max(bytes, least) rounded up to `align` -- the one
// rounding rule.  Carver(8): the predict stages (an empty piece takes nothing); Carver(256, 1): -trf, -tcf and the
// candidate reads (every piece has a slot of its own).
class Carver {
 public:
  explicit Carver(size_t align, size_t least = 0) : align_(align), least_(least) {}
  template <class T>
  Piece<T> take(uint64_t count) {
    const Piece<T> p{used_};
    used_ += (std::max((size_t)count * sizeof(T), least_) + align_ - 1) & ~(align_ - 1);
    return p;
  }
  size_t total() const { return used_; }

 private:
  size_t align_, least_, used_ = 0;
};
// the layout of a call that uses the stat words alone (the first piece of its stage's 8-byte layouts)
size_t stat_only_bytes(uint32_t words) {
  Carver c(8);
  c.take<uint32_t>(words);
  return c.total();
}

// the size-and-alignment check of a call that takes caller scratch; `sizer` is the call that reports `need`
int scratch_ok(const char* fn, const void* d_tmp, uint64_t tmp_bytes, uint64_t need, const char* sizer) {
  if (tmp_bytes < need || ((uintptr_t)d_tmp & 7)) return fail(MRG_ERR_ARG, "%s: scratch smaller than %s, or unaligned", fn, sizer);
  return MRG_OK;
}

// n stat words back to the host on the stream, and the stream synchronised (whatever else was queued rides along)
int read_stat(const uint32_t* stat, uint32_t* h_stat, size_t n, hipStream_t st) {
  HIP_TRY(hipMemcpyAsync(h_stat, stat, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return MRG_OK;
}

// a writer's body with what it throws mapped to a code: invalid_argument is the caller's data, anything else the file's
template <class F>
auto guarded(const char* fn, F&& body) -> decltype(body()) {
  try {
    return body();
  } catch (const std::invalid_argument& e) {
    return fail(MRG_ERR_ARG, "%s: %s", fn, e.what());
  } catch (const std::exception& e) {
    return fail(MRG_ERR_IO, "%s: %s", fn, e.what());
  }
}

struct DevLib {
  uint32_t *blocks = nullptr, *super = nullptr, *text = nullptr, *seg_start = nullptr,
           *seg_ref = nullptr, *seg_off = nullptr, *chunk_seg = nullptr;
  uint64_t* sa = nullptr;
  uint32_t* ctx = nullptr;
  uint32_t* sa16 = nullptr;  // wide rows of a large library (fm_index.hpp: fill_wide_rows)
  bool tables_on_device = false;  // jump tables / row context / wide rows / buckets were filled by libtables.hip
  uint32_t* buckets = nullptr;  // seed buckets (fm_index.hpp: fill_seed_buckets), 128 B per k-mer of bucket_k bases
  uint32_t bucket_k = 0;
  uint32_t* pos_rows = nullptr;  // position lists of the k-mers whose bucket overflows (fm_index.hpp: seed_pos_lists), 16-byte rows
  uint64_t pos_rows_n = 0;
  // pair tables of a small library (fm_index.hpp: PairTables), for 2-mismatch passes
  uint32_t* pair_jump = nullptr;
  uint64_t* pair_rows = nullptr;
  uint32_t pair_row_off[3] = {0, 0, 0};
  uint32_t pair_anchor = 0;
  uint32_t* pair_jump_s = nullptr;        // second set: anchors of pair_anchor - 1 bases
  uint32_t pair_row_off_s[3] = {0, 0, 0};  // (its row lists follow the first set's in pair_rows)
  // pair tables of a large library (pairs.hip), built on the device the first time a one-mismatch
  // sub-pass of a fused launch meets reads with short seed regions: three anchors, gaps A and 2A
  uint32_t* bpair_jump = nullptr;
  uint64_t* bpair_rows = nullptr;
  uint32_t bpair_row_off[3] = {0, 0, 0};
  uint32_t bpair_anchor = 0;
  bool bpair_failed = false;  // not enough free HBM: the pigeonhole pieces stay
  // exact-match dictionary (dict_index.hpp) of a library of at most dict_max_bases bases
  mrg::DictSlot* dict_slots = nullptr;
  uint32_t dict_log2 = 0, dict_key = 0;
  uint64_t dict_n_keys = 0, dict_n_overflow = 0;  // positions stored / left to the FM index (their home's chain overflowed)
  uint32_t* kbits = nullptr;
  std::vector<uint32_t> kbits_host;  // host copy (32 KB): the per-round interleaved tables are built from it
  std::vector<std::string> host_seqs;  // entries of a library of at most kDictSmallBases bases (for seed units over several libraries)
  uint32_t* ftab = nullptr;
  mrg::JumpTables tabs = {{0, 0, 0, 0}, {0, 0, 0, 0}};
  uint32_t n = 0, nblk = 0, nsup = 0, primary = 0, text_words = 0, n_seg = 0, n_ref = 0;
  uint32_t max_ref_len = 0;
  bool simple = false;  // every entry is exactly one N-free segment: segment id == entry id, offset 0
  uint32_t* first_seg = nullptr;  // [n_ref + 1] the segments of entry e are [first_seg[e], first_seg[e + 1]) (mrg_predict_precursor_bases, on first use)
};

template <class T>
int upload(T** dst, const std::vector<T>& v, size_t pad_to_multiple = 1) {
  size_t n = v.size();
  size_t n_alloc = ((n + pad_to_multiple - 1) / pad_to_multiple) * pad_to_multiple;
  if (n_alloc == 0) n_alloc = pad_to_multiple;
  HIP_TRY(hipMalloc((void**)dst, n_alloc * sizeof(T)));
  HIP_TRY(hipMemset(*dst, 0, n_alloc * sizeof(T)));
  if (n) HIP_TRY(hipMemcpy(*dst, v.data(), n * sizeof(T), hipMemcpyHostToDevice));
  return MRG_OK;
}

constexpr uint32_t kStatsPerPass = 5;
constexpr uint32_t kWalkCap = 256;  // wave_seed_kernel: records a wave may leave behind its stream (in the cascade workspace)

void free_dev_lib(DevLib& l);

// What a seed_kernel unit searches: one library, or several small ones searched with the same
// policy as ONE index of their concatenation (entries of member j start at entry_lo[j]).  Built
// the first time a cascade plans such a unit, kept for the life of the context.
struct SeedLib {
  std::string key;     // member library ids, e.g. "2,4,5"
  DevLib lib;          // FM arrays (with 16-byte rows)
  bool owned = false;  // false: `lib` is a copy of the pointers of a library of the context
  std::vector<uint32_t> entry_lo;
  uint32_t* kbits = nullptr;  // presence bitmaps of the 8-, 9-, 10- and 11-mers (owned units of small libraries)
};

}  // namespace

namespace {
// RCCL is resolved with dlopen/dlsym at the first mrg_comm_* call: a process whose host side is
// PyTorch has torch's own librccl loaded already (that copy is reused, one RCCL per process), a
// torch-less host gets the system library.  Nothing links against it, so single-GPU users need no
// RCCL at all.
struct RcclApi {
  void* handle = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
  std::string error;
};

RcclApi* rccl_api() {
  static RcclApi api;
  static bool tried = false;
  if (tried) return &api;
  tried = true;
  const char* names[] = {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"};
  for (const char* n : names)  // a copy that is already mapped (torch's) wins
    if ((api.handle = dlopen(n, RTLD_NOW | RTLD_NOLOAD))) break;
  for (size_t i = 0; !api.handle && i < sizeof names / sizeof *names; ++i) api.handle = dlopen(names[i], RTLD_NOW | RTLD_GLOBAL);
  if (!api.handle) {
    api.error = std::string("librccl.so not found: ") + (dlerror() ? dlerror() : "?");
    return &api;
  }
  api.GetUniqueId = (decltype(api.GetUniqueId))dlsym(api.handle, "ncclGetUniqueId");
  api.CommInitRank = (decltype(api.CommInitRank))dlsym(api.handle, "ncclCommInitRank");
  api.AllReduce = (decltype(api.AllReduce))dlsym(api.handle, "ncclAllReduce");
  api.CommDestroy = (decltype(api.CommDestroy))dlsym(api.handle, "ncclCommDestroy");
  api.GetErrorString = (decltype(api.GetErrorString))dlsym(api.handle, "ncclGetErrorString");
  if (!api.GetUniqueId || !api.CommInitRank || !api.AllReduce || !api.CommDestroy) {
    api.error = "librccl.so lacks ncclGetUniqueId / ncclCommInitRank / ncclAllReduce / ncclCommDestroy";
    api.handle = nullptr;
  }
  return &api;
}
}  // namespace

struct mrg_ctx {
  int device = 0;
  ncclComm_t comm = nullptr;
  int comm_rank = 0, comm_world = 1;
  int n_cu = 0;
  uint64_t hbm_bytes = 0;
  std::string arch;
  int64_t lds_budget = 160 * 1024;
  int64_t wstop = 8;
  int64_t use_ftab = 1;
  int64_t force_lds_mode = -1;
  int64_t wide_rows = 64;
  int64_t hint_min_len = 0, hint_max_len = 255;  // length range of the reads of the NEXT run only
  uint64_t run_id = 0;
  // interleaved 9-mer tables of fused rounds, keyed by "lib ids | log2 | bits" (built on first use)
  std::vector<std::pair<std::string, uint32_t*>> round_tables;
  void* scratch = nullptr;  // context-owned device scratch (grown on demand; mrg_list_best_count)
  uint64_t scratch_bytes = 0;
  int64_t kmer_filter = 1;
  int64_t ctx_wide_rows = 32;
  int64_t prefer_two_blocks = 1;
  // 0 = one launch per pass; 1 = consecutive passes with at most one seed mismatch share a launch,
  // small (bitmap-filtered) and large libraries in separate groups; 2 = one group regardless of
  // library size; 3 = only the small-library runs are fused
  int64_t fuse = 1;
  int64_t round_large = 0;
  int64_t split_strata = 1;
  int64_t pair_big = 5;      // anchor length of the pair tables of large libraries (one-mismatch sub-passes of fused launches, reads with 3A..4A-1 seed bases); 0 = off
  int64_t pair_seeds = 1;    // 2-mismatch passes on small libraries search through anchor pairs (set before add_library)
  int64_t stratum_rows = 0;  // (measured slower than match_kernel: 2.43 vs 2.28 ms) 1: the last stratum of a split 2-mismatch pass runs stratum_kernel; 2: every strata launch does
  int64_t wide_rows_16 = 1;  // libraries of >= 2^20 bases get 16-byte rows with 32 bases of context
  int64_t dict = 1;          // one-word batches without N run the dictionary kernels (dict.hip) where a pass can
  int64_t dict_key = 16;     // key length of the exact-match dictionaries (set before add_library)
  // libraries up to this size get an exact-match dictionary (set before add_library).  The default covers the
  // small libraries; a host that will run passes WITHOUT seed mismatch on a large one (mRNA `-n 0`) raises it
  // for that library (16 B x 2..4 slots per base of HBM), as mirge_amd/engine.py does
  int64_t dict_max_bases = (int64_t)mrg::kDictSmallBases;
  int64_t split_mixed = 1;    // a batch with long reads / reads with N: its one-word N-free reads take the dictionary kernels
  int64_t split_min_len = 16;  // ... and so do not reads shorter than this (the reference's own minimum length, trim_file.py:33; shorter seed regions than 15 bases have no pair tables)
  int64_t stratum0_unit = 0;  // (measured slower, default off) the exact stratum of a 2-mismatch pass behind a seed launch rides in that launch
  int64_t walk_diag = 0;
  int64_t count_variants = 1;  // mrg_count_best, one seed mismatch: the jump-table variants kernel in front of the pigeonhole kernel (2: and no pigeonhole kernel behind it)
  int64_t long_lane = 0;   // round 6: 1 = the reads of 33..63 nt of a split batch ride the dictionary kernels too (their LONG instantiations; measured no faster than the FM kernels: off)
  int64_t walk_cap = 256;  // records a wave may leave behind its stream (<= 256; tests shrink it: beyond it a seed is verified row by row)
  int64_t pos_scan = 1;   // 0 at run time: the seed launches verify a wide interval row by row as before round 6
  int64_t pos_lists = 1;  // overflowing seed buckets get their rows in text order too (set before add_library)
  int64_t seed_buckets = 1;  // large libraries get seed buckets where they pay (set before add_library); 0 at run time: not used
  int64_t seed_wgs = 0;      // seed_kernel workgroups (256 threads) per CU; 0 = what the launch's instantiation keeps resident
  int64_t seed_units = 1;    // ... and their runs of passes with at most one seed mismatch go through seed_kernel
  int64_t pair_impl = 1;   // 1 = pair_wave_kernel for the anchor-pair search of one-word batches, 0 = stratum_kernel
  int64_t grid_pct = 100;  // share of the workgroups every cascade launch gets (see scale_grid)
  // "fused_step": a caller that follows EVERY cascade with a tally on the same stream (bench.py's step, the command line):
  // no per-pass events are recorded (mrg_pass_stats.ms = 0) and d_pass_counts is written by the tally launch
  int64_t fused_step = 0;
  uint64_t* pending_export_out = nullptr;
  hipStream_t pending_export_stream = nullptr;
  uint32_t last_tally_launch[2][4] = {{0}};  // mrg_ctx_last_tally_launch: [tally, edit tally] x (flags, grid, LDS bytes, 0)
  int64_t device_tables = 1;  // mrg_ctx_add_library: a large library's derived tables (dictionary, wide rows, seed buckets) are filled on the device
  mrg::CollapseInfo last_collapse;  // mrg_ctx_last_collapse: what the last mrg_collapse_run that succeeded did
  int64_t collapse_fast = 1;  // mrg_collapse_run: batches that fit it take the duplication-aware path (0: always the general sort)
  int64_t seed_impl = -1;  // -1 = per launch (launch_seed), 0 = seed_kernel (tiles), 1 = wave_seed_kernel, 2 = the same with more registers
  std::vector<DevLib> libs;
  std::vector<std::unique_ptr<SeedLib>> seed_libs;
  // last run
  hipStream_t last_stream = nullptr;
  uint64_t* last_stats_dev = nullptr;
  uint32_t last_n_pass = 0;
  uint32_t last_lds[MRG_MAX_PASSES] = {0};
  uint32_t last_mode[MRG_MAX_PASSES] = {0};
  uint32_t last_group[MRG_MAX_PASSES] = {0};
  uint32_t last_launches[MRG_MAX_PASSES] = {0};
  uint32_t last_split = 0;  // the last run split its batch into one-word reads and the rest
  uint32_t last_kbits_log2[MRG_MAX_PASSES] = {0};
  uint32_t last_pair_anchor[MRG_MAX_PASSES] = {0};
  uint32_t last_variant[MRG_MAX_PASSES] = {0};
  hipEvent_t ev[MRG_MAX_PASSES + 1] = {nullptr};
  hipEvent_t ev0[MRG_MAX_PASSES + 1] = {nullptr};  // the first cascade of a split batch
  // which event holds the time of pass boundary i: a boundary with no launch since the one before shares its event
  // (an event record costs ~5 us of an idle GPU: five of them less per step)
  uint8_t ev_ix[MRG_MAX_PASSES + 1] = {0}, ev0_ix[MRG_MAX_PASSES + 1] = {0};
  bool ev_ready = false;
  bool last_timed = true;  // the last run recorded its per-pass events
};

extern "C" {

int mrg_version(void) { return 100; }
const char* mrg_last_error(void) { return g_err.c_str(); }

// ----------------------------------------------------------------- index
int mrg_index_build(const char* const* names, const char* const* seqs, uint32_t n_ref,
                    mrg_index** out) {
  if (!out || (n_ref && (!names || !seqs))) return fail(MRG_ERR_ARG, "mrg_index_build: null argument");
  try {
    std::vector<std::string> nv(n_ref), sv(n_ref);
    for (uint32_t i = 0; i < n_ref; ++i) {
      nv[i] = names[i];
      sv[i] = seqs[i];
    }
    auto h = std::make_unique<mrg_index>();
    mrg::build_index(nv, sv, h->ix);
    *out = h.release();
    return MRG_OK;
  } catch (const std::bad_alloc&) {
    return fail(MRG_ERR_NOMEM, "mrg_index_build: out of memory");
  } catch (const std::exception& e) {
    return fail(MRG_ERR_FORMAT, "mrg_index_build: %s", e.what());
  }
}

int mrg_index_build_fasta(const char* fasta_path, mrg_index** out) {
  if (!fasta_path || !out) return fail(MRG_ERR_ARG, "mrg_index_build_fasta: null argument");
  try {
    std::vector<std::string> nv, sv;
    mrg::read_fasta(fasta_path, nv, sv);
    auto h = std::make_unique<mrg_index>();
    mrg::build_index(nv, sv, h->ix);
    *out = h.release();
    return MRG_OK;
  } catch (const std::bad_alloc&) {
    return fail(MRG_ERR_NOMEM, "mrg_index_build_fasta: out of memory");
  } catch (const std::exception& e) {
    return fail(MRG_ERR_IO, "mrg_index_build_fasta: %s", e.what());
  }
}

// the device route: same host code, the suffix array and what is made from it by sa_build.hip on `device`
static int build_on_device(const char* who, int device, bool from_fasta, const char* fasta_path, const char* const* names,
                           const char* const* seqs, uint32_t n_ref, mrg_index** out) {
  g_device_build_rounds = 0;
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0)
    return fail(MRG_ERR_NO_DEVICE, "%s: no HIP device visible (%s); the device route has no host fallback", who,
                e != hipSuccess ? hipGetErrorString(e) : "device count 0");
  if (device < 0 || device >= count) return fail(MRG_ERR_NO_DEVICE, "%s: device %d not in [0,%d)", who, device, count);
  // the calling thread's current device is the caller's: put it back on every way out
  struct DeviceScope {
    int prev = -1;
    ~DeviceScope() {
      if (prev >= 0) (void)hipSetDevice(prev);
    }
  } scope;
  HIP_TRY(hipGetDevice(&scope.prev));
  HIP_TRY(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0)
    return fail(MRG_ERR_NO_DEVICE, "%s: device %d is %s; kernels are built for gfx950 only", who, device, prop.gcnArchName);
  try {
    std::vector<std::string> nv, sv;
    if (from_fasta) {
      mrg::read_fasta(fasta_path, nv, sv);
    } else {
      nv.resize(n_ref);
      sv.resize(n_ref);
      for (uint32_t i = 0; i < n_ref; ++i) {
        if (!names[i] || !seqs[i]) return fail(MRG_ERR_ARG, "%s: entry %u is null", who, i);
        nv[i] = names[i];
        sv[i] = seqs[i];
      }
    }
    auto h = std::make_unique<mrg_index>();
    uint32_t rounds = 0;
    const mrg::RowBuilder rows = [&rounds](mrg::FmIndex& ix) { mrg::build_rows_device(ix, &rounds); };
    mrg::build_index(nv, sv, h->ix, &rows);
    g_device_build_rounds = rounds;
    *out = h.release();
    return MRG_OK;
  } catch (const std::bad_alloc&) {
    return fail(MRG_ERR_NOMEM, "%s: out of memory", who);
  } catch (const mrg::SaBuildError& e) {
    return fail(e.no_memory ? MRG_ERR_NOMEM : MRG_ERR_HIP, "%s: %s", who, e.what());
  } catch (const std::exception& e) {
    return fail(from_fasta ? MRG_ERR_IO : MRG_ERR_FORMAT, "%s: %s", who, e.what());
  }
}

int mrg_index_build_device(int device, const char* const* names, const char* const* seqs, uint32_t n_ref, mrg_index** out) {
  if (!out || (n_ref && (!names || !seqs))) return fail(MRG_ERR_ARG, "mrg_index_build_device: null argument");
  return build_on_device("mrg_index_build_device", device, false, nullptr, names, seqs, n_ref, out);
}

int mrg_index_build_fasta_device(int device, const char* fasta_path, mrg_index** out) {
  if (!fasta_path || !out) return fail(MRG_ERR_ARG, "mrg_index_build_fasta_device: null argument");
  return build_on_device("mrg_index_build_fasta_device", device, true, fasta_path, nullptr, nullptr, 0, out);
}

uint32_t mrg_index_build_device_rounds(void) { return g_device_build_rounds; }

int mrg_index_build_ebwt(const char* prefix, mrg_index** out) {
  if (!prefix || !out) return fail(MRG_ERR_ARG, "mrg_index_build_ebwt: null argument");
  try {
    std::vector<std::string> nv, sv;
    mrg::read_ebwt(prefix, nv, sv);
    auto h = std::make_unique<mrg_index>();
    mrg::build_index(nv, sv, h->ix);
    *out = h.release();
    return MRG_OK;
  } catch (const std::bad_alloc&) {
    return fail(MRG_ERR_NOMEM, "mrg_index_build_ebwt: out of memory");
  } catch (const std::exception& e) {
    return fail(MRG_ERR_IO, "mrg_index_build_ebwt: %s", e.what());
  }
}

int mrg_index_save(const mrg_index* ix, const char* path) {
  if (!ix || !path) return fail(MRG_ERR_ARG, "mrg_index_save: null argument");
  try {
    mrg::save_index(ix->ix, path);
    return MRG_OK;
  } catch (const std::exception& e) {
    return fail(MRG_ERR_IO, "mrg_index_save: %s", e.what());
  }
}

int mrg_index_load(const char* path, mrg_index** out) {
  if (!path || !out) return fail(MRG_ERR_ARG, "mrg_index_load: null argument");
  try {
    auto h = std::make_unique<mrg_index>();
    mrg::load_index(path, h->ix);
    *out = h.release();
    return MRG_OK;
  } catch (const std::exception& e) {
    return fail(MRG_ERR_IO, "mrg_index_load: %s", e.what());
  }
}

void mrg_index_free(mrg_index* ix) { delete ix; }

int mrg_index_get_info(const mrg_index* h, mrg_index_info* info) {
  if (!h || !info) return fail(MRG_ERR_ARG, "mrg_index_get_info: null argument");
  const mrg::FmIndex& ix = h->ix;
  info->n_ref = (uint32_t)ix.names.size();
  info->n_seg = (uint32_t)ix.seg_ref.size();
  info->n_bases = ix.n;
  info->n_blocks = (uint32_t)ix.blocks.size();
  info->n_super = (uint32_t)(ix.super.size() / 4);
  info->primary = ix.primary;
  info->text_words = (uint32_t)ix.text.size();
  for (int t = 0; t < 4; ++t) info->ftab_ks[t] = ix.ftab_ks[t];
  for (int c = 0; c < 4; ++c) info->C[c] = ix.C[c];
  info->bytes_fm = (uint64_t)ix.blocks.size() * 16 + (uint64_t)ix.super.size() * 4;
  info->bytes_sa = (uint64_t)ix.sa.size() * 8;
  return MRG_OK;
}

int mrg_index_name(const mrg_index* h, uint32_t i, const char** name) {
  if (!h || !name) return fail(MRG_ERR_ARG, "mrg_index_name: null argument");
  if (i >= h->ix.names.size()) return fail(MRG_ERR_ARG, "mrg_index_name: entry %u out of range", i);
  *name = h->ix.names[i].c_str();
  return MRG_OK;
}

int mrg_index_seq(const mrg_index* h, uint32_t i, char* buf, uint32_t cap, uint32_t* len) {
  if (!h || !len) return fail(MRG_ERR_ARG, "mrg_index_seq: null argument");
  if (i >= h->ix.names.size()) return fail(MRG_ERR_ARG, "mrg_index_seq: entry %u out of range", i);
  *len = h->ix.ref_len[i];
  if (!buf) return MRG_OK;
  if (cap < *len + 1) return fail(MRG_ERR_ARG, "mrg_index_seq: buffer too small (%u < %u)", cap, *len + 1);
  std::string s = mrg::entry_sequence(h->ix, i);
  std::memcpy(buf, s.c_str(), s.size() + 1);
  return MRG_OK;
}

int mrg_index_get_view(const mrg_index* h, mrg_index_view* v) {
  if (!h || !v) return fail(MRG_ERR_ARG, "mrg_index_get_view: null argument");
  const mrg::FmIndex& ix = h->derived();
  v->blocks = reinterpret_cast<const uint32_t*>(ix.blocks.data());
  v->super = ix.super.data();
  v->text = ix.text.data();
  v->sa = ix.sa.data();
  v->ftab = ix.ftab.data();
  v->ctx = ix.ctx.empty() ? nullptr : ix.ctx.data();
  v->kbits = ix.kbits.empty() ? nullptr : ix.kbits.data();
  v->seg_start = ix.seg_start.data();
  v->seg_ref = ix.seg_ref.data();
  v->seg_off = ix.seg_off.data();
  v->chunk_seg = ix.chunk_seg.data();
  return MRG_OK;
}

int mrg_index_get_dict(const mrg_index* h, uint32_t key_bases, mrg_dict_view* v) {
  if (!h || !v) return fail(MRG_ERR_ARG, "mrg_index_get_dict: null argument");
  try {
    const mrg::ExactDict& d = h->dict(key_bases);
    v->slots = reinterpret_cast<const uint64_t*>(d.slots.data());
    v->log2_slots = d.log2_slots;
    v->key_bases = d.key_bases;
    v->n_keys = d.n_keys;
    v->n_overflow = d.n_overflow;
    return MRG_OK;
  } catch (const std::bad_alloc&) {
    return fail(MRG_ERR_NOMEM, "mrg_index_get_dict: out of memory");
  } catch (const std::exception& e) {
    return fail(MRG_ERR_ARG, "mrg_index_get_dict: %s", e.what());
  }
}

// --------------------------------------------------------------- context
int mrg_ctx_create(int device, mrg_ctx** out) {
  if (!out) return fail(MRG_ERR_ARG, "mrg_ctx_create: null argument");
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0)
    return fail(MRG_ERR_NO_DEVICE,
                "mrg_ctx_create: no HIP device visible (%s); this engine has no CPU fallback",
                e != hipSuccess ? hipGetErrorString(e) : "device count 0");
  if (device < 0 || device >= count)
    return fail(MRG_ERR_NO_DEVICE, "mrg_ctx_create: device %d not in [0,%d)", device, count);
  HIP_TRY(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  auto ctx = std::make_unique<mrg_ctx>();
  ctx->device = device;
  ctx->n_cu = prop.multiProcessorCount;
  ctx->hbm_bytes = prop.totalGlobalMem;
  ctx->arch = prop.gcnArchName;
  if (ctx->arch.rfind("gfx950", 0) != 0)
    return fail(MRG_ERR_NO_DEVICE, "mrg_ctx_create: device %d is %s; kernels are built for gfx950 only",
                device, ctx->arch.c_str());
  ctx->lds_budget = (int64_t)prop.sharedMemPerBlock;  // 160 KiB on gfx950
  if (ctx->lds_budget > 160 * 1024) ctx->lds_budget = 160 * 1024;
  *out = ctx.release();
  return MRG_OK;
}

void mrg_ctx_destroy(mrg_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  for (DevLib& l : ctx->libs) free_dev_lib(l);
  for (auto& sl : ctx->seed_libs) {
    if (sl->owned) free_dev_lib(sl->lib);
    (void)hipFree(sl->kbits);
  }
  if (ctx->ev_ready)
  {
    for (auto& e : ctx->ev) (void)hipEventDestroy(e);
    for (auto& e : ctx->ev0) (void)hipEventDestroy(e);
  }
  if (ctx->comm) (void)rccl_api()->CommDestroy(ctx->comm);
  (void)hipFree(ctx->scratch);
  for (auto& kv : ctx->round_tables) (void)hipFree(kv.second);
  delete ctx;
}

namespace {
void free_dev_lib(DevLib& l) {
  void* ptrs[] = {l.blocks, l.super, l.text, l.sa, l.ftab, l.ctx, l.sa16, l.buckets, l.pos_rows, l.kbits, l.pair_jump, l.pair_jump_s, l.pair_rows, l.dict_slots,
                  l.bpair_jump, l.bpair_rows, l.seg_start, l.seg_ref, l.seg_off, l.chunk_seg, l.first_seg};
  for (void* p : ptrs) (void)hipFree(p);
}

// The FM arrays of one index into HBM.  wide_rows: also the 16-byte rows; pair_tables: also the
// anchor-pair tables of 2-mismatch passes.
int upload_index(mrg_ctx* ctx, const mrg::FmIndex& ix, DevLib& l, bool wide_rows, bool pair_tables) {
  mrg::StageTimer tm("upload_index");
  int rc;
  l.n = ix.n;
  l.nblk = (uint32_t)ix.blocks.size();
  l.primary = ix.primary;
  l.n_seg = (uint32_t)ix.seg_ref.size();
  l.n_ref = (uint32_t)ix.names.size();
  l.nsup = (uint32_t)(ix.super.size() / 4);
  // (not just "as many segments as entries": an all-N entry and one with an inner N run would
  // also give equal counts)
  l.simple = l.n_seg == l.n_ref;
  for (uint32_t sg = 0; l.simple && sg < l.n_seg; ++sg) l.simple = ix.seg_ref[sg] == sg && ix.seg_off[sg] == 0;
  for (uint32_t v : ix.ref_len) l.max_ref_len = std::max(l.max_ref_len, v);
  std::vector<uint32_t> blk(reinterpret_cast<const uint32_t*>(ix.blocks.data()),
                            reinterpret_cast<const uint32_t*>(ix.blocks.data()) + ix.blocks.size() * 4);
  if ((rc = upload(&l.blocks, blk, 4))) return rc;
  if ((rc = upload(&l.super, ix.super, 4))) return rc;
  // text is staged into LDS 16 B at a time: round its word count up to 4
  l.text_words = (uint32_t)((ix.text.size() + 3) / 4 * 4);
  if ((rc = upload(&l.text, ix.text, 4))) return rc;
  if ((rc = upload(&l.sa, ix.sa))) return rc;
  {
    // ascending k for the kernels; ix.ftab_ks is in storage order (largest first, 0 = absent)
    uint32_t off = 0, offs[4];
    for (int t = 0; t < 4; ++t) {
      offs[t] = off;
      if (ix.ftab_ks[t]) off += (1u << (2 * ix.ftab_ks[t])) + 1u;
    }
    for (int i = 0; i < 4; ++i) {
      int t = 3 - i;
      if (!ix.ftab_ks[t]) t = 1;  // no big table: the main one again
      l.tabs.k[i] = ix.ftab_ks[t];
      l.tabs.off[i] = offs[t];
    }
  }
  const bool on_device = ctx->device_tables && ix.n >= mrg::kLazyDeriveBases;
  if (!on_device && !ix.derived)
    return fail(MRG_ERR_ARG, "upload_index: the index's jump tables are not derived (derive_tables before the upload)");
  if (on_device) {
    // jump tables, row context and wide rows from the rows and the text just uploaded (libtables.hip)
    size_t total = 0;
    for (int t = 0; t < 4; ++t)
      if (ix.ftab_ks[t]) total += ((size_t)1 << (2 * ix.ftab_ks[t])) + 1;
    tm.lap("blocks, text, sa");
    void* tmp = nullptr;
    HIP_TRY(hipMalloc((void**)&l.ftab, total * 4));
    HIP_TRY(hipMalloc(&tmp, mrg::jump_tables_device_temp_bytes(ix.n + 1u)));
    hipError_t e = mrg::build_jump_tables_device(l.text, l.text_words, reinterpret_cast<const uint64_t*>(l.sa), ix.n, ix.ftab_ks, l.ftab, tmp, nullptr);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    (void)hipFree(tmp);
    if (e != hipSuccess) return fail(MRG_ERR_HIP, "mrg_ctx_add_library: jump tables on the device: %s", hipGetErrorString(e));
    HIP_TRY(hipMalloc((void**)&l.ctx, (size_t)(ix.n + 1u) * 4));
    HIP_TRY(mrg::build_row_context_device(l.text, l.text_words, reinterpret_cast<const uint64_t*>(l.sa), ix.n, l.ctx, nullptr));
    if (wide_rows) {
      HIP_TRY(hipMalloc((void**)&l.sa16, (size_t)(ix.n + 1u) * 16));
      HIP_TRY(mrg::build_wide_rows_device(l.text, l.text_words, reinterpret_cast<const uint64_t*>(l.sa), ix.n, l.sa16, nullptr));
    }
    HIP_TRY(hipStreamSynchronize(nullptr));
    l.tables_on_device = true;
    tm.lap("jump tables, row context, wide rows (device)");
  } else {
    if ((rc = upload(&l.ftab, ix.ftab))) return rc;
    if (!ix.ctx.empty() && (rc = upload(&l.ctx, ix.ctx))) return rc;
    tm.lap("blocks, text, sa, jump tables, ctx");
  }
  if (wide_rows && !on_device) {
    // 16-byte rows for the fused launches: filled on the host in chunks, never kept there
    const size_t n_rows = ix.sa.size(), chunk = 1u << 24;
    HIP_TRY(hipMalloc((void**)&l.sa16, n_rows * 16));
    std::vector<uint32_t> buf;
    for (size_t lo = 0; lo < n_rows; lo += chunk) {
      const size_t hi = std::min(n_rows, lo + chunk);
      buf.resize((hi - lo) * 4);
      mrg::fill_wide_rows(ix, lo, hi, buf.data());
      HIP_TRY(hipMemcpy(l.sa16 + lo * 4, buf.data(), (hi - lo) * 16, hipMemcpyHostToDevice));
    }
  }
  tm.lap("wide rows");
  if (pair_tables && ix.n <= mrg::kPairMaxBases && ix.n >= 4u * mrg::kPairAnchor) {
    mrg::PairTables pt, pt_s;
    try {
      mrg::build_pair_tables(ix, mrg::kPairAnchor, pt);
      mrg::build_pair_tables(ix, mrg::kPairAnchor - 1u, pt_s);
    } catch (const std::exception& e) {
      return fail(MRG_ERR_ARG, "mrg_ctx_add_library: %s", e.what());
    }
    if ((rc = upload(&l.pair_jump, pt.jump))) return rc;
    if ((rc = upload(&l.pair_jump_s, pt_s.jump))) return rc;
    for (int t = 0; t < 3; ++t) {
      l.pair_row_off[t] = pt.row_off[t];
      l.pair_row_off_s[t] = pt.row_off[3] + pt_s.row_off[t];
    }
    pt.rows.insert(pt.rows.end(), pt_s.rows.begin(), pt_s.rows.end());
    if ((rc = upload(&l.pair_rows, pt.rows))) return rc;
    l.pair_anchor = pt.anchor;
  }
  tm.lap("pair tables");
  if (!ix.kbits.empty() && (rc = upload(&l.kbits, ix.kbits))) return rc;
  l.kbits_host = ix.kbits;  // the interleaved tables of fused rounds are built from it
  if ((rc = upload(&l.seg_start, ix.seg_start))) return rc;
  if ((rc = upload(&l.seg_ref, ix.seg_ref))) return rc;
  if ((rc = upload(&l.seg_off, ix.seg_off))) return rc;
  if ((rc = upload(&l.chunk_seg, ix.chunk_seg))) return rc;
  return MRG_OK;
}
}  // namespace

int mrg_ctx_add_library(mrg_ctx* ctx, const mrg_index* h, int32_t* lib_id) {
  if (!ctx || !h || !lib_id) return fail(MRG_ERR_ARG, "mrg_ctx_add_library: null argument");
  HIP_TRY(hipSetDevice(ctx->device));
  const bool tables_dev = ctx->device_tables && h->ix.n >= mrg::kLazyDeriveBases;
  const mrg::FmIndex& ix = tables_dev ? h->ix : h->derived();
  DevLib l;
  struct Guard {  // a failed upload must not leak the arrays uploaded before it
    DevLib* l;
    ~Guard() {
      if (l) free_dev_lib(*l);
    }
  } guard{&l};
  mrg::StageTimer tm("add_library");
  int rc = upload_index(ctx, ix, l, ix.n >= mrg::kWideRowMinBases && ctx->wide_rows_16, ctx->pair_seeds != 0);
  if (rc) return rc;
  tm.lap("index arrays + wide rows + pair tables");
  // Exact-match dictionary: every library of at most dict_max_bases bases whose slot array (16 B x 2..4
  // slots per base: 8.6 GB for the 137 Mbp mRNA library) leaves 8 GB of this GPU's HBM free.  A pass
  // without seed mismatch on it -- mRNA `-n 0`, RAP:584/598 -- is then ONE 16-byte gather per read
  // instead of a jump-table line and a wide-row line.
  bool want_dict = ctx->dict && ix.n <= (uint64_t)ctx->dict_max_bases && ix.n <= mrg::kDictMaxBases && ix.n >= (uint32_t)ctx->dict_key;
  if (want_dict && ix.n > mrg::kDictSmallBases) {
    const uint64_t need = mrg::exact_dict_bytes(ix, (uint32_t)ctx->dict_key);
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    want_dict = need != 0 && free_b > need + (8ull << 30);
  }
  if (want_dict && ctx->device_tables && ix.n > mrg::kDictSmallBases) {
    // a large library's dictionary is filled on the device, from the text and segment tables uploaded above
    // (dictbuild.hip): no host build, no 8.6 GB upload
    const uint64_t bytes = mrg::exact_dict_bytes(ix, (uint32_t)ctx->dict_key);
    uint32_t l2 = 0;
    while (bytes && (16ull << l2) < bytes) ++l2;
    if (bytes && mrg::exact_dict_device_ok(ix.n, (uint32_t)ctx->dict_key, l2)) {
      void* tmp = nullptr;
      HIP_TRY(hipMalloc((void**)&l.dict_slots, bytes));
      hipError_t e = hipMalloc(&tmp, mrg::exact_dict_device_temp_bytes(ix.n));
      uint64_t counts[2] = {0, 0};
      if (e == hipSuccess)
        e = mrg::build_exact_dict_device(l.text, ix.n, l.seg_start, l.seg_ref, l.seg_off, l.chunk_seg, (uint32_t)ctx->dict_key, l2, l.dict_slots, tmp,
                                         counts, nullptr);
      (void)hipFree(tmp);
      if (e != hipSuccess) return fail(MRG_ERR_HIP, "mrg_ctx_add_library: dictionary build on the device: %s", hipGetErrorString(e));
      l.dict_log2 = l2;
      l.dict_key = (uint32_t)ctx->dict_key;
      l.dict_n_keys = counts[0];
      l.dict_n_overflow = counts[1];
      want_dict = false;
    }
  }
  if (want_dict) {
    const mrg::ExactDict* ed = nullptr;
    try {
      ed = &h->dict((uint32_t)ctx->dict_key);
    } catch (const std::exception&) {
      ed = nullptr;  // entries too long for the slot format: the FM kernels serve this library
    }
    if (ed) {
      if ((rc = upload(&l.dict_slots, ed->slots))) return rc;
      l.dict_log2 = ed->log2_slots;
      l.dict_key = ed->key_bases;
      l.dict_n_keys = ed->n_keys;
      l.dict_n_overflow = ed->n_overflow;
      if (ix.n > mrg::kDictSmallBases) h->drop_dict((uint32_t)ctx->dict_key);
    }
  }
  tm.lap("dictionary");
  if (ctx->dict && ctx->seed_buckets && l.sa16) {
    // large library where a seed of 11 bases has a few rows: those rows in one line per seed
    const uint32_t bk = mrg::seed_bucket_k(ix);
    if (bk) {
      const uint64_t n_codes = 1ull << (2 * bk), chunk = 1ull << 18;
      size_t free_b = 0, total_b = 0;
      HIP_TRY(hipMemGetInfo(&free_b, &total_b));
      if (l.tables_on_device && free_b > n_codes * 128ull + (4ull << 30) && hipMalloc((void**)&l.buckets, n_codes * 128ull) == hipSuccess) {
        size_t tab_base = 0;
        for (int t = 0; t < 4 && ix.ftab_ks[t] != bk; ++t)
          if (ix.ftab_ks[t]) tab_base += ((size_t)1 << (2 * ix.ftab_ks[t])) + 1;
        HIP_TRY(mrg::build_seed_buckets_device(l.text, l.text_words, reinterpret_cast<const uint64_t*>(l.sa), ix.n, l.ftab + tab_base, bk, l.buckets, nullptr));
        HIP_TRY(hipStreamSynchronize(nullptr));
        l.bucket_k = bk;
      } else if (!l.tables_on_device && free_b > n_codes * 128ull + (4ull << 30) && hipMalloc((void**)&l.buckets, n_codes * 128ull) == hipSuccess) {
        std::vector<uint32_t> buf(chunk * 32);
        for (uint64_t lo = 0; lo < n_codes; lo += chunk) {
          const uint64_t hi = std::min(n_codes, lo + chunk);
          mrg::fill_seed_buckets(ix, bk, lo, hi, buf.data());
          HIP_TRY(hipMemcpy(l.buckets + lo * 32, buf.data(), (hi - lo) * 128, hipMemcpyHostToDevice));
        }
        l.bucket_k = bk;
      } else {
        (void)hipGetLastError();
        l.buckets = nullptr;
      }
      if (l.buckets && l.bucket_k && ctx->pos_lists) {
        // the k-mers whose bucket overflows (repeats, poly-A, tandem motifs): their rows in text order (round 6)
        size_t tab_base = 0;
        for (int t = 0; t < 4 && ix.ftab_ks[t] != bk; ++t)
          if (ix.ftab_ks[t]) tab_base += ((size_t)1 << (2 * ix.ftab_ks[t])) + 1;
        hipError_t e = mrg::build_seed_pos_lists_device(l.text, l.text_words, reinterpret_cast<const uint64_t*>(l.sa), ix.n, l.ftab + tab_base, bk,
                                                        l.buckets, &l.pos_rows, &l.pos_rows_n, nullptr);
        if (e != hipSuccess) return fail(MRG_ERR_HIP, "mrg_ctx_add_library: position lists of the seed buckets: %s", hipGetErrorString(e));
      }
    }
  }
  // small libraries keep their entries on the host: passes that search several of them with one
  // policy get one index of their concatenation (seed_kernel units), built when a cascade first asks
  if (ctx->dict && ix.n <= mrg::kDictSmallBases) {
    l.host_seqs.resize(ix.names.size());
    for (uint32_t i = 0; i < l.host_seqs.size(); ++i) l.host_seqs[i] = mrg::entry_sequence(ix, i);
  }
  tm.lap("seed buckets + host entries");
  ctx->libs.push_back(l);
  guard.l = nullptr;
  *lib_id = (int32_t)ctx->libs.size() - 1;
  return MRG_OK;
}

int mrg_ctx_set_option(mrg_ctx* ctx, const char* key, int64_t value) {
  if (!ctx || !key) return fail(MRG_ERR_ARG, "mrg_ctx_set_option: null argument");
  std::string k(key);
  if (k == "lds_budget") {
    if (value < 0 || value > 160 * 1024) return fail(MRG_ERR_ARG, "lds_budget must be in [0,163840]");
    ctx->lds_budget = value;
  } else if (k == "wstop") {
    if (value < 0) return fail(MRG_ERR_ARG, "wstop must be >= 0");
    ctx->wstop = value;
  } else if (k == "ctx_wide_rows") {
    if (value < 1) return fail(MRG_ERR_ARG, "ctx_wide_rows must be >= 1");
    ctx->ctx_wide_rows = value;
  } else if (k == "kmer_filter") {
    ctx->kmer_filter = value != 0;
  } else if (k == "hint_min_len") {
    ctx->hint_min_len = value;
  } else if (k == "hint_max_len") {
    ctx->hint_max_len = value;
  } else if (k == "wide_rows") {
    if (value < 1) return fail(MRG_ERR_ARG, "wide_rows must be >= 1");
    ctx->wide_rows = value;
  } else if (k == "prefer_two_blocks") {
    ctx->prefer_two_blocks = value != 0;
  } else if (k == "force_lds_mode") {
    if (value < -1 || value > 3) return fail(MRG_ERR_ARG, "force_lds_mode must be in [-1,3]");
    ctx->force_lds_mode = value;
  } else if (k == "ftab") {
    ctx->use_ftab = value != 0;
  } else if (k == "split_strata") {
    ctx->split_strata = value != 0;
  } else if (k == "pair_big") {
    if (value != 0 && (value < 4 || value > 7)) return fail(MRG_ERR_ARG, "pair_big must be 0 or in [4,7]");
    ctx->pair_big = value;
  } else if (k == "pair_seeds") {
    ctx->pair_seeds = value != 0;
  } else if (k == "stratum_rows") {
    if (value < 0 || value > 2) return fail(MRG_ERR_ARG, "stratum_rows must be in [0,2]");
    ctx->stratum_rows = value;
  } else if (k == "round_large") {
    ctx->round_large = value != 0;
  } else if (k == "wide_rows_16") {
    ctx->wide_rows_16 = value != 0;  // takes effect for libraries added afterwards
  } else if (k == "dict") {
    ctx->dict = value != 0;  // (the dictionaries themselves are built by mrg_ctx_add_library while this is 1)
  } else if (k == "split_mixed") {
    ctx->split_mixed = value != 0;
  } else if (k == "split_min_len") {
    if (value < 0 || value > 32) return fail(MRG_ERR_ARG, "mrg_ctx_set_option: split_min_len must be in [0,32]");
    ctx->split_min_len = value;
  } else if (k == "stratum0_unit") {
    ctx->stratum0_unit = value != 0;
  } else if (k == "seed_buckets") {
    ctx->seed_buckets = value != 0;
  } else if (k == "pos_lists") {
    ctx->pos_lists = value != 0;
  } else if (k == "pos_scan") {
    ctx->pos_scan = value != 0;
  } else if (k == "count_variants") {
    if (value < 0 || value > 2) return fail(MRG_ERR_ARG, "count_variants must be 0, 1 or 2");
    ctx->count_variants = value;
  } else if (k == "walk_cap") {
    if (value < 0 || value > (int64_t)kWalkCap) return fail(MRG_ERR_ARG, "walk_cap must be in [0,256]");
    ctx->walk_cap = value;
  } else if (k == "walk_diag") {
    ctx->walk_diag = value;
  } else if (k == "long_lane") {
    ctx->long_lane = value != 0;
  } else if (k == "seed_wgs") {
    ctx->seed_wgs = value;
  } else if (k == "pair_impl") {
    ctx->pair_impl = value != 0;
  } else if (k == "grid_pct") {
    if (value < 1 || value > 100) return fail(MRG_ERR_ARG, "grid_pct must be in [1,100]");
    ctx->grid_pct = value;
  } else if (k == "seed_impl") {
    if (value < -1 || value > 2) return fail(MRG_ERR_ARG, "seed_impl must be in [-1,2]");
    ctx->seed_impl = value;
  } else if (k == "seed_units") {
    ctx->seed_units = value != 0;
  } else if (k == "fused_step") {
    ctx->fused_step = value != 0;
  } else if (k == "collapse_fast") {
    ctx->collapse_fast = value != 0;
  } else if (k == "device_tables") {
    ctx->device_tables = value != 0;  // takes effect for libraries added afterwards
  } else if (k == "dict_max_bases") {
    if (value < 0) return fail(MRG_ERR_ARG, "dict_max_bases must be >= 0");
    ctx->dict_max_bases = value;  // takes effect for libraries added afterwards
  } else if (k == "dict_key") {
    if (value < 8 || value > 16) return fail(MRG_ERR_ARG, "dict_key must be in [8,16]");
    ctx->dict_key = value;
  } else if (k == "fuse") {
    if (value < 0 || value > 3) return fail(MRG_ERR_ARG, "fuse must be in [0,3]");
    ctx->fuse = value;
  } else {
    return fail(MRG_ERR_ARG, "mrg_ctx_set_option: unknown key '%s'", key);
  }
  return MRG_OK;
}

int mrg_ctx_device_info(const mrg_ctx* ctx, int32_t* n_cu, uint64_t* hbm_bytes, char* arch,
                        uint32_t arch_cap) {
  if (!ctx) return fail(MRG_ERR_ARG, "mrg_ctx_device_info: null argument");
  if (n_cu) *n_cu = ctx->n_cu;
  if (hbm_bytes) *hbm_bytes = ctx->hbm_bytes;
  if (arch && arch_cap) {
    std::snprintf(arch, arch_cap, "%s", ctx->arch.c_str());
  }
  return MRG_OK;
}

int mrg_ctx_library_stats(const mrg_ctx* ctx, int32_t lib, uint64_t* out4) {
  if (!ctx || !out4) return fail(MRG_ERR_ARG, "mrg_ctx_library_stats: null argument");
  if (lib < 0 || (size_t)lib >= ctx->libs.size()) return fail(MRG_ERR_ARG, "mrg_ctx_library_stats: unknown library %d", lib);
  const DevLib& l = ctx->libs[lib];
  out4[0] = l.dict_n_keys;
  out4[1] = l.dict_n_overflow;
  out4[2] = l.dict_slots ? l.dict_log2 : 0;
  out4[3] = l.buckets ? l.bucket_k : 0;
  return MRG_OK;
}

int mrg_ctx_library_check_tables(mrg_ctx* ctx, int32_t lib, const mrg_index* index, uint64_t* mismatches4) {
  if (!ctx || !index || !mismatches4) return fail(MRG_ERR_ARG, "mrg_ctx_library_check_tables: null argument");
  if (lib < 0 || (size_t)lib >= ctx->libs.size()) return fail(MRG_ERR_ARG, "mrg_ctx_library_check_tables: unknown library %d", lib);
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipDeviceSynchronize());
  const DevLib& l = ctx->libs[lib];
  try {
    const mrg::FmIndex& ix = index->derived();
    if (ix.n != l.n) return fail(MRG_ERR_ARG, "mrg_ctx_library_check_tables: not the index this library was made from");
    for (int t = 0; t < 4; ++t) mismatches4[t] = ~0ull;
    std::vector<uint32_t> got, want;
    auto compare = [&](const uint32_t* dev, const uint32_t* host, size_t words) -> uint64_t {
      uint64_t bad = 0;
      const size_t chunk = (size_t)1 << 24;
      for (size_t lo = 0; lo < words; lo += chunk) {
        const size_t m = std::min(chunk, words - lo);
        got.resize(m);
        if (hipMemcpy(got.data(), dev + lo, m * 4, hipMemcpyDeviceToHost) != hipSuccess) return ~0ull - 1;
        for (size_t i = 0; i < m; ++i) bad += got[i] != host[lo + i];
      }
      return bad;
    };
    if (l.ftab) mismatches4[0] = compare(l.ftab, ix.ftab.data(), ix.ftab.size());
    if (l.ctx && !ix.ctx.empty()) mismatches4[1] = compare(l.ctx, ix.ctx.data(), ix.ctx.size());
    if (l.sa16) {
      uint64_t bad = 0;
      const size_t n_rows = ix.sa.size(), chunk = (size_t)1 << 22;
      for (size_t lo = 0; lo < n_rows; lo += chunk) {
        const size_t hi = std::min(n_rows, lo + chunk);
        want.resize((hi - lo) * 4);
        mrg::fill_wide_rows(ix, lo, hi, want.data());
        bad += compare(l.sa16 + lo * 4, want.data(), want.size());
      }
      mismatches4[2] = bad;
    }
    if (l.buckets && l.bucket_k) {
      uint64_t bad = 0;
      const uint64_t n_codes = 1ull << (2 * l.bucket_k), chunk = 1ull << 18;
      std::vector<uint32_t> over_start, over_pos;
      mrg::seed_pos_lists(ix, l.bucket_k, over_start, over_pos);
      if (!l.pos_rows && ctx->pos_lists && !over_pos.empty()) bad += 1;
      for (uint64_t lo = 0; lo < n_codes; lo += chunk) {
        const uint64_t hi = std::min(n_codes, lo + chunk);
        want.resize((hi - lo) * 32);
        mrg::fill_seed_buckets(ix, l.bucket_k, lo, hi, want.data(), l.pos_rows ? over_start.data() : nullptr);
        bad += compare(l.buckets + lo * 32, want.data(), want.size());
      }
      if (l.pos_rows) {  // the position lists themselves: every row = the wide row of the position the host lists there
        if (l.pos_rows_n != over_pos.size()) {
          bad += 1;
        } else {
          std::vector<uint64_t> row_of(ix.n + 1u);
          for (size_t i = 0; i < ix.sa.size(); ++i) row_of[(uint32_t)ix.sa[i]] = ix.sa[i];
          const size_t chunk_rows = (size_t)1 << 20;
          for (size_t r0 = 0; r0 < over_pos.size(); r0 += chunk_rows) {
            const size_t r1 = std::min(over_pos.size(), r0 + chunk_rows);
            want.resize((r1 - r0) * 4);
            for (size_t r = r0; r < r1; ++r) mrg::wide_row_of_row(ix, row_of[over_pos[r]], want.data() + 4 * (r - r0));
            bad += compare(l.pos_rows + r0 * 4, want.data(), want.size());
          }
        }
      }
      mismatches4[3] = bad;
    }
  } catch (const std::exception& e) {
    return fail(MRG_ERR_NOMEM, "mrg_ctx_library_check_tables: %s", e.what());
  }
  return MRG_OK;
}

int mrg_ctx_release_scratch(mrg_ctx* ctx) {
  if (!ctx) return fail(MRG_ERR_ARG, "mrg_ctx_release_scratch: null argument");
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipDeviceSynchronize());
  if (ctx->scratch) HIP_TRY(hipFree(ctx->scratch));
  ctx->scratch = nullptr;
  ctx->scratch_bytes = 0;
  return MRG_OK;
}

// --------------------------------------------------------------- cascade
// workspace: [idx A][idx B][idx C]  (each n + kListSlack u32: segmented survivor lists; a producer
//            workgroup's segment holds every read of its chunks, 256, 1024 or 4096 reads each; C parks
//            the one-word reads of a split batch while the other reads run their cascade)
//            [segment counts A, B, C: kMaxSegments u32 each][stats: MRG_MAX_PASSES * 5 u64]
// (16 bytes per entry: the seed launches of a one-word batch write lists that carry their reads -- index, length, read --;
// exact_dict_kernel and the FM kernels keep 4-byte index lists in the same buffers)
static uint64_t ws_idx_bytes(uint64_t n) {
  return (((n + mrg::kListSlack) * 16 + 255) / 256) * 256;
}
static const uint64_t kWsCountsBytes = 3 * mrg::kMaxSegments * 4;
static const uint64_t kWsStatsBytes = MRG_MAX_PASSES * kStatsPerPass * 8;
// round 6: the records of the reads a wave of wave_seed_kernel answers behind its stream (dict.hip; 32 bytes each, kWalkCap per
// wave of the largest grid) -- in the caller's workspace, not in the context: cascades of one context on several streams
// (the e2e leg's chunks) must not share them
static const uint64_t kWsWalkBytes = (uint64_t)mrg::kMaxSegments * (mrg::kSeedThreads / 64u) * kWalkCap * 32ull;

int mrg_cascade_workspace_bytes(uint64_t n, uint64_t* bytes) {
  if (!bytes) return fail(MRG_ERR_ARG, "mrg_cascade_workspace_bytes: null argument");
  *bytes = 3 * ws_idx_bytes(n) + kWsCountsBytes + kWsStatsBytes + kWsWalkBytes;
  return MRG_OK;
}

namespace {
// The index a seed unit searches (SeedLib): cached by member list.
int get_seed_lib(mrg_ctx* ctx, const std::vector<int32_t>& lib_ids, SeedLib** out) {
  std::string key;
  for (int32_t id : lib_ids) key += std::to_string(id) + ",";
  for (auto& sl : ctx->seed_libs)
    if (sl->key == key) {
      *out = sl.get();
      return MRG_OK;
    }
  auto sl = std::make_unique<SeedLib>();
  sl->key = key;
  const DevLib& first = ctx->libs[lib_ids[0]];
  if (lib_ids.size() == 1 && first.host_seqs.empty()) {
    // a large library: its own arrays (the caller made sure it has 16-byte rows)
    sl->lib = first;
    sl->lib.host_seqs.clear();
    sl->lib.kbits_host.clear();
    sl->owned = false;
    sl->entry_lo.assign(1, 0u);
  } else {
    std::vector<std::string> names, seqs;
    for (int32_t id : lib_ids) {
      const DevLib& l = ctx->libs[id];
      sl->entry_lo.push_back((uint32_t)seqs.size());
      for (size_t i = 0; i < l.host_seqs.size(); ++i) {
        names.push_back("u" + std::to_string(id) + "_" + std::to_string(i));
        seqs.push_back(l.host_seqs[i]);
      }
    }
    mrg::FmIndex ix;
    try {
      mrg::build_index(names, seqs, ix);
    } catch (const std::bad_alloc&) {
      return fail(MRG_ERR_NOMEM, "mrg_cascade_run: out of memory indexing libraries %s", key.c_str());
    } catch (const std::exception& e) {
      return fail(MRG_ERR_FORMAT, "mrg_cascade_run: indexing libraries %s: %s", key.c_str(), e.what());
    }
    // build_index leaves jump tables and row context of an index of >= kLazyDeriveBases bases to the
    // device; a context with device_tables = 0 needs them from the host before upload_index reads them
    if (!ix.derived && !(ctx->device_tables && ix.n >= mrg::kLazyDeriveBases)) mrg::derive_tables(ix);
    sl->owned = true;
    struct Guard {
      SeedLib* s;
      ~Guard() {
        if (!s) return;
        free_dev_lib(s->lib);
        (void)hipFree(s->kbits);
      }
    } guard{sl.get()};
    int rc = upload_index(ctx, ix, sl->lib, true, false);
    if (rc) return rc;
    // presence bitmaps of the k-mers, k = 8..11: bit c = some text position starts the k-mer with
    // code c (first base in the low two bits)
    std::vector<uint32_t> bits(mrg::kSeedKbitsWords, 0u);
    for (size_t sg = 0; sg + 1 < ix.seg_start.size(); ++sg) {
      const uint32_t s0 = ix.seg_start[sg], s1 = ix.seg_start[sg + 1];
      for (uint32_t p = s0; p < s1; ++p) {
        const uint32_t w = p >> 4, sh = (p & 15u) * 2u;
        const uint64_t lo64 = (uint64_t)ix.text[w] | ((uint64_t)ix.text[w + 1] << 32);
        const uint32_t win = (uint32_t)(lo64 >> sh);  // 16 bases from p
        for (uint32_t k = 8; k <= 11 && p + k <= s1; ++k) {
          const uint32_t c = win & ((1u << (2 * k)) - 1u);
          bits[mrg::seed_kbits_word_off(k) + (c >> 5)] |= 1u << (c & 31u);
        }
      }
    }
    if ((rc = upload(&sl->kbits, bits))) return rc;
    guard.s = nullptr;
  }
  *out = sl.get();
  ctx->seed_libs.push_back(std::move(sl));
  return MRG_OK;
}
}  // namespace

}  // extern "C"

namespace {

// ---- shared fills of the kernels' parameter blocks (kernels.hpp): by field name, for every struct that has the fields ----

// the FM arrays of a resident library (what else a struct takes of it -- simple_segs, ctx, sa16, nblk, nsup, text_words -- and
// whether tabs.k[0] is cleared for "ftab" = 0 is its call site's business)
template <class P>
void fill_lib(P& p, const DevLib& l) {
  p.blocks = l.blocks;
  p.super = l.super;
  p.text = l.text;
  p.sa = l.sa;
  p.ftab = l.ftab;
  p.tabs = l.tabs;
  p.seg_start = l.seg_start;
  p.seg_ref = l.seg_ref;
  p.seg_off = l.seg_off;
  p.chunk_seg = l.chunk_seg;
  p.n = l.n;
  p.primary = l.primary;
}

// a pass's read window: the trims, the length range, the poly-T rule
template <class P>
void fill_window(P& p, const mrg_pass_cfg& c) {
  p.trim5 = c.trim5;
  p.trim3 = c.trim3;
  p.min_len = c.min_len;
  p.max_len = c.max_len;
  p.poly_t = c.poly_t;
}

// ... and its seed length and mismatch budget (max_mm_seed and pass_index where the struct has them: at the call site)
template <class P>
void fill_policy(P& p, const mrg_pass_cfg& c) {
  fill_window(p, c);
  p.seed_len = c.seed_len;
  p.max_mm_total = c.max_mm_total;
}

// ---- routing decisions of the cascade: each is made here and nowhere else ----

// Pass c can take the exact-match dictionary of its library for the stratum of `mm_seed` seed mismatches it starts with
// (the dictionary's key is matched letter for letter: only a pass whose seed covers it may take it)
bool pass_takes_dict(const mrg_pass_cfg& c, const DevLib& l, int32_t mm_seed = 0) {
  return c.max_mm_seed == mm_seed && l.dict_slots != nullptr && c.seed_len >= (int32_t)l.dict_key;
}

// A 2-mismatch pass goes through the anchor pairs of its library: for every read long enough to hold the four anchors,
// all strata of the pigeonhole search for the shorter ones, in one launch
bool pass_takes_pairs(const mrg_ctx& ctx, const mrg_pass_cfg& c, const DevLib& l) {
  return c.max_mm_seed == 2 && ctx.pair_seeds && l.pair_anchor && ctx.force_lds_mode < 0 && !c.poly_t &&
         c.seed_len >= (int32_t)(4u * l.pair_anchor);
}

// ... and it does so in pair_wave_kernel (dict.hip: one-word reads without N), not in stratum_kernel
bool pairs_by_wave(const mrg_ctx& ctx, bool dict_batch) { return dict_batch && ctx.pair_impl != 0; }

// One large library under a one-mismatch policy and (by the length hints) reads whose seed region is 3 A .. 4 A - 1 bases:
// three anchor pairs instead of two pieces of less than 2 A bases.  The anchor length A of the tables the pass wants
// (pairs.hip; built on the device at first use: ensure_bpair), or 0.
int64_t three_anchor_tables(const mrg_ctx& ctx, const mrg_pass_cfg& c, const DevLib& l) {
  const int64_t A = ctx.pair_big;
  if (!A || c.max_mm_seed != 1 || c.poly_t || l.n < mrg::kWideRowMinBases) return 0;
  const int64_t r_min = std::min<int64_t>(std::max<int64_t>(ctx.hint_min_len, c.min_len) - c.trim5 - c.trim3, c.seed_len);
  const int64_t r_max = std::min<int64_t>(std::min<int64_t>(ctx.hint_max_len, c.max_len) - c.trim5 - c.trim3, c.seed_len);
  return (r_min < 4 * A && r_max >= 3 * A) ? A : 0;
}

// A pass whose length window excludes every read of the batch (caller's hint: e.g. the hairpin
// pass, len > 25, on 22-nt reads) would only copy its input list: it is not launched; its
// counters stay zero and the next pass reads the same list.  (Never the last pass: that one
// writes the "unannotated" values.)
bool pass_skipped(const mrg_ctx& ctx, const mrg_pass_cfg& c, bool last_pass) {
  return !last_pass && (c.min_len > ctx.hint_max_len || c.max_len < ctx.hint_min_len);
}

// a library whose 9-mer bitmap filters the seed pieces of the FM kernels
bool small_lib(const mrg_ctx& ctx, const DevLib& l) { return l.kbits != nullptr && ctx.kmer_filter; }

// the read lengths of 33..63 nt a pass's window holds (bit b = length 33 + b); wave_lib = the library of a pass that runs in
// pair_wave_kernel: only those of them the kernel cannot take -- it sees the trimmed read, which must fit one word unless it
// is longer than the library's longest entry (then it cannot align at all)
uint64_t window_bits(const mrg_pass_cfg& c, const DevLib* wave_lib = nullptr) {
  uint64_t m = 0;
  for (int L = 33; L <= 63; ++L) {
    const int Lt = L - c.trim5 - c.trim3;
    if (L >= c.min_len && L <= c.max_len && (!wave_lib || (Lt > 32 && Lt <= (int)wave_lib->max_ref_len))) m |= 1ull << (L - 33);
  }
  return m;
}

// residency decision of match_kernel.  The superblock table (16 B per 65536 bp) and the segment
// prefix always sit in LDS (`overhead`, with the control block and the 9-mer bitmap).  With the jump table most seed
// searches need few LF steps, so the packed text (read by every verification) is the first thing worth
// staging and two resident workgroups per CU (<= 80 KB each) beat a fuller LDS:
//   2 = blocks + text, 3 = text only, 1 = blocks only, 0 = nothing.
struct Residency {
  int mode;
  uint64_t bytes;
};
Residency match_residency(const mrg_ctx& ctx, const DevLib& l, uint64_t overhead) {
  const uint64_t blk_bytes = (uint64_t)l.nblk * 16, txt_bytes = (uint64_t)l.text_words * 4;
  const uint64_t budget = (uint64_t)ctx.lds_budget, hard = 160 * 1024, half = 80 * 1024;
  Residency r{0, 0};
  if (blk_bytes + txt_bytes <= budget && overhead + blk_bytes + txt_bytes <= half)
    r = {2, blk_bytes + txt_bytes};
  else if (ctx.prefer_two_blocks && txt_bytes <= budget && overhead + txt_bytes <= half)
    r = {3, txt_bytes};
  else if (blk_bytes + txt_bytes <= budget && overhead + blk_bytes + txt_bytes <= hard)
    r = {2, blk_bytes + txt_bytes};
  else if (txt_bytes <= budget && overhead + txt_bytes <= hard)
    r = {3, txt_bytes};
  else if (blk_bytes <= budget && overhead + blk_bytes <= hard)
    r = {1, blk_bytes};
  if (ctx.force_lds_mode >= 0) {  // test hook: exercise a specific kernel variant
    const int m = (int)ctx.force_lds_mode;
    const uint64_t need = (m == 2 ? blk_bytes + txt_bytes : m == 3 ? txt_bytes : m == 1 ? blk_bytes : 0);
    if (overhead + need <= hard) r = {m, need};
  }
  return r;
}

// ---- launch plan: which passes run, and which consecutive ones share a (fused or seed) launch ----

// one unit of a seed launch (dict.hip): 0 = an FM search over its members' libraries, 1 = a dictionary lookup
struct SeedUnitPlan {
  uint32_t kind;
  std::vector<uint32_t> members;
  bool stratum0 = false;  // the exact stratum of a LATER 2-mismatch pass (see plan_chain)
};

struct Launch {
  enum Kind { kExact, kStrata, kPairs, kFused, kSeed };  // exact_dict_kernel; match / stratum kernel; anchor pairs; fused_kernel; seed kernels
  Kind kind = kStrata;
  uint32_t first = 0, end = 0;    // the passes it covers: [first, end), hint-skipped ones that ride inside a group included
  std::vector<uint32_t> members;  // those of them that run (kSeed: see units)
  int32_t k_first = 1, k_last = 1;             // kStrata / kPairs: the strata of the pigeonhole search it runs ...
  bool first_part = true, last_part = true;   // ... and whether it is the pass's first / last launch
  std::vector<SeedUnitPlan> units;  // kSeed
  bool small = false;               // kSeed: the size class of its libraries
  bool ends_cascade = false;        // nothing reads a survivor list behind it
};

// The launches of one chain -- the whole batch, or the FM side (dict_batch = false) or the one-word lane (dict_batch = true)
// of a split batch -- in the order they are issued.  Pure: no HIP call, nothing of the context is written.
// lane_long: the lane of a batch that may hold reads of 33..63 nt ("long_lane").
// A 2-mismatch `--best` pass on a library with an exact-match dictionary, right behind a seed
// launch: its exact stratum -- what most isomiRs are after the -5 / -3 trims -- rides in that launch
// as a dictionary unit (a 0-mismatch hit is final: nothing beats it, the lowest (entry, offset) wins
// ties as always); the pass's own launch then searches the reads that are left and does not count
// "processed" again ("stratum0_unit").
std::vector<Launch> plan_chain(const mrg_ctx& ctx, const mrg_pass_cfg* passes, uint32_t n_pass, uint64_t n, bool dict_batch,
                               bool lane_long) {
  auto lib = [&](uint32_t i) -> const DevLib& { return ctx.libs[passes[i].lib]; };
  bool runs[MRG_MAX_PASSES], stratum0_done[MRG_MAX_PASSES] = {false};
  for (uint32_t i = 0; i < n_pass; ++i) runs[i] = !pass_skipped(ctx, passes[i], i + 1 == n_pass);
  auto fusable = [&](uint32_t i) {
    // the first launched pass streams the whole read set and keeps the classic kernel (library
    // text + full bitmap in LDS); 2-mismatch policies have their own stratum-first instantiation.
    // (A fused launch counts offered / aligned reads in 16-bit per-lane fields: one workgroup per
    // CU must see fewer than 65536 chunks.)
    return ctx.fuse != 0 && passes[i].max_mm_seed <= 1 && n / (1024ull * (uint64_t)std::max(ctx.n_cu, 1)) < 60000ull;
  };
  // a pass seed_kernel can take as (part of) a unit, and the size class of its library
  auto seedable = [&](uint32_t i) {
    if (!dict_batch || !ctx.seed_units || ctx.force_lds_mode >= 0 || !fusable(i)) return false;
    return pass_takes_dict(passes[i], lib(i)) || !lib(i).host_seqs.empty() || lib(i).sa16 != nullptr;
  };
  auto small_class = [&](uint32_t i) { return !lib(i).host_seqs.empty(); };

  std::vector<Launch> plan;
  bool launched_any = false;
  for (uint32_t i = 0; i < n_pass;) {
    if (!runs[i]) {
      ++i;
      continue;
    }
    // (a batch that may hold reads of 33..63 nt: the one-word lane reads a list from its first launch on, and only a seed
    // launch can take such reads -- e.g. a batch of long reads only, whose first pass to run is the hairpin pass, len > 25)
    const bool lane_first = lane_long && window_bits(passes[i]) != 0;
    if ((launched_any || lane_first) && seedable(i)) {
      Launch L;
      L.kind = Launch::kSeed;
      L.first = i;
      L.small = small_class(i);
      uint32_t j = i;
      while (j < n_pass) {
        if (!runs[j]) {
          ++j;
          continue;
        }
        if (!seedable(j) || small_class(j) != L.small) break;
        const mrg_pass_cfg& c = passes[j];
        const bool k1 = pass_takes_dict(c, lib(j));
        int join = -1;
        if (!k1 && L.small)  // small libraries searched with one policy: one unit over their concatenation
          for (size_t u = 0; u < L.units.size(); ++u) {
            if (L.units[u].kind != 0u || L.units[u].members.size() >= mrg::kSeedMaxMembers) continue;
            const mrg_pass_cfg& d = passes[L.units[u].members[0]];
            if (d.max_mm_seed == c.max_mm_seed && d.trim5 == c.trim5 && d.trim3 == c.trim3 && d.min_len == c.min_len &&
                d.max_len == c.max_len && d.poly_t == c.poly_t) {
              join = (int)u;
              break;
            }
          }
        if (join >= 0) {
          L.units[join].members.push_back(j);
        } else {
          if (L.units.size() == mrg::kSeedMaxUnits) break;
          L.units.push_back(SeedUnitPlan{k1 ? 1u : 0u, {j}});
        }
        ++j;
      }
      // (passes skipped by the length hint at the end of the run stay with it: never the last pass)
      if (ctx.stratum0_unit && j < n_pass && runs[j] && !passes[j].poly_t && pass_takes_dict(passes[j], lib(j), 2) &&
          L.units.size() < mrg::kSeedMaxUnits && ctx.pair_seeds && ctx.force_lds_mode < 0) {
        SeedUnitPlan s0{1u, {j}};
        s0.stratum0 = true;
        L.units.push_back(s0);
        stratum0_done[j] = true;
      }
      L.end = j;
      L.ends_cascade = j == n_pass;
      plan.push_back(std::move(L));
      i = j;
      // (a seed launch does NOT set launched_any: behind a long lane's first launch the passes still see "no launch yet" --
      // a seed launch only where lane_first holds, never a fused one.  Kept: tests/test_gpu_split.py pins the lane's routes.)
      continue;
    }
    Launch L;
    L.first = i;
    uint32_t j = i;
    if (launched_any && fusable(i)) {
      const bool cls = small_lib(ctx, lib(i));
      while (j < n_pass && L.members.size() < mrg::kMaxFused) {
        if (!runs[j]) {
          ++j;
          continue;
        }
        if (!fusable(j)) break;
        if (ctx.fuse != 2 && small_lib(ctx, lib(j)) != cls) break;
        if (ctx.fuse == 3 && !cls) break;
        L.members.push_back(j++);
      }
      // passes skipped by the hint at the end of the run stay with the group (their events share
      // the group's); a trailing skipped pass is never the last pass of the cascade
    }
    launched_any = true;
    if (L.members.size() >= 2) {
      L.kind = Launch::kFused;
      L.end = j;
      L.ends_cascade = L.members.back() + 1 == n_pass;
      plan.push_back(std::move(L));
      i = j;
      continue;
    }
    const mrg_pass_cfg& c = passes[i];
    L.members.assign(1, i);
    L.end = i + 1;
    L.ends_cascade = i + 1 == n_pass;
    L.k_last = c.max_mm_seed + 1;
    L.first_part = !stratum0_done[i];
    if (dict_batch && pass_takes_dict(c, lib(i)) && ctx.force_lds_mode < 0) {
      // no seed mismatch, one-word reads, a library with an exact-match dictionary: dict.hip
      L.kind = Launch::kExact;
    } else if (pass_takes_pairs(ctx, c, lib(i))) {
      L.kind = Launch::kPairs;  // (whatever the batch or "pair_impl": stratum_kernel walks the pairs where pair_wave_kernel cannot)
    } else if (c.max_mm_seed == 2 && ctx.split_strata) {
      // strata 1..2 on the incoming reads, stratum 3 on the compacted survivors (kernels.hpp)
      Launch head = L;
      head.kind = Launch::kStrata;
      head.k_last = 2;
      head.last_part = head.ends_cascade = false;
      plan.push_back(std::move(head));
      L.kind = Launch::kStrata;
      L.k_first = L.k_last = 3;
      L.first_part = false;
    } else {
      L.kind = Launch::kStrata;
    }
    plan.push_back(std::move(L));
    ++i;
  }
  return plan;
}

// Round 6: which read lengths beyond 32 nt the one-word lane of a split batch takes (bit b = length 33 + b, up to 63): the
// seed kernels have instantiations that carry a read's second word (seeds from the first 32 bases, the rest compared
// where an alignment is verified; dictionary units answer such reads by FM search); exact_dict_kernel and the FM kernels
// of the lane do not, pair_wave_kernel takes a read whose TRIMMED length fits one word.  A length is let in when every
// pass of the cascade either runs in a seed launch, or cannot hold a read of that length in its window, or
// (pair_wave_kernel) sees at most 32 bases of it or could not align it at all (longer than the library's longest entry).
// Read off the lane's own plan; 0 = the lane is for reads of at most 32 nt.
uint64_t lane_long_mask(const mrg_ctx& ctx, const mrg_pass_cfg* passes, const std::vector<Launch>& lane_plan) {
  uint64_t mask = (1ull << 31) - 1ull;
  for (const Launch& L : lane_plan) {
    if (L.kind == Launch::kSeed) continue;  // every length
    // exact_dict_kernel, an FM kernel: only lengths its window keeps out (the lane is a dict_batch: with "pair_impl" = 0 its
    // anchor-pair launch is stratum_kernel, an FM kernel)
    const bool wave = L.kind == Launch::kPairs && pairs_by_wave(ctx, true);
    for (uint32_t i : L.members) mask &= ~window_bits(passes[i], wave ? &ctx.libs[passes[i].lib] : nullptr);
  }
  return mask;
}

// pair tables of a large library (three anchors of A bases, gaps A and 2 A: pairs.hip), built on the device the first
// time a cascade meets reads whose seed region is 3 A .. 4 A - 1 bases under a one-mismatch policy
int ensure_bpair(DevLib& lm, int64_t A, hipStream_t stream) {
  if (lm.bpair_anchor == (uint32_t)A || lm.bpair_failed) return MRG_OK;
  (void)hipFree(lm.bpair_jump);
  (void)hipFree(lm.bpair_rows);
  lm.bpair_jump = nullptr;
  lm.bpair_rows = nullptr;
  lm.bpair_anchor = 0;
  const uint64_t n_rows = (uint64_t)lm.n + 1, n_codes1 = (1ull << (4u * (uint32_t)A)) + 1ull;
  const uint64_t need = 2 * n_codes1 * 4 + 2 * n_rows * 8 + 4 * n_rows * 4 + (256ull << 20);
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  if (free_b < need || hipMalloc((void**)&lm.bpair_jump, 2 * n_codes1 * 4) != hipSuccess ||
      hipMalloc((void**)&lm.bpair_rows, 2 * n_rows * 8) != hipSuccess ||
      mrg::build_pair_tables_device(lm.sa, lm.text, (uint32_t)n_rows, (uint32_t)A, 2, lm.bpair_jump, lm.bpair_rows, lm.bpair_row_off,
                                    stream) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipFree(lm.bpair_jump);
    (void)hipFree(lm.bpair_rows);
    lm.bpair_jump = nullptr;
    lm.bpair_rows = nullptr;
    lm.bpair_failed = true;
  } else {
    lm.bpair_anchor = (uint32_t)A;
  }
  return MRG_OK;
}
// ... and handed to a parameter block (left as it is, anchor 0, where the build found no room: the pigeonhole pieces stay)
int bind_bpair(DevLib& lm, int64_t A, hipStream_t stream, const uint32_t** jump, const uint64_t** rows, uint32_t* row_off,
               uint32_t* anchor) {
  if (const int rc = ensure_bpair(lm, A, stream)) return rc;
  if (lm.bpair_anchor != (uint32_t)A) return MRG_OK;
  *jump = lm.bpair_jump;
  *rows = lm.bpair_rows;
  row_off[0] = lm.bpair_row_off[0];
  row_off[1] = lm.bpair_row_off[1];
  *anchor = (uint32_t)A;
  return MRG_OK;
}

// ---- issuing a plan ----

// What one mrg_cascade_run call puts onto its stream: the call's arguments and carved workspace (fixed), and the state the
// launches of the chain that is being issued hand on to one another -- which survivor list is the newest and in which form,
// and the per-pass events.
struct CascadeRun {
  mrg_ctx* ctx;
  const mrg_pass_cfg* passes;
  uint32_t n_pass;
  const uint64_t* d_reads;
  const uint8_t* d_lens;
  uint64_t n;
  int8_t* d_pass_id;
  int32_t *d_ref_id, *d_pos;
  uint8_t* d_mm;
  uint32_t* d_packed;
  uint32_t *idx[3], *counts;  // the workspace: three list buffers and their segment counts,
  uint64_t* stats;            // the per-pass counters,
  uint4* ws_walk;             // the records wave_seed_kernel's waves leave behind their stream
  hipStream_t stream;
  bool timed;  // ("fused_step": no event lives inside the step: nothing between its launches)
  // the chain: what its kernels see of the batch
  bool dict_batch;
  uint32_t words_eff;
  const uint64_t* nmask_eff;
  uint64_t long_mask = 0;  // the lengths beyond 32 nt its reads may have (lane_long_mask; only the lane of a split batch)
  // its survivor lists
  int cur_list = 0;          // which list buffer holds the newest survivor list
  bool have_list = false;    // false: the next pass that runs reads the identity list of all reads
  bool list_fat = false;     // the newest list carries its reads (16-byte entries, written by a seed launch or pair_wave_kernel)
  bool out_init = false;     // the first launch wrote every output (exact_dict_kernel, streaming): later ones write claims only
  int pair0 = 0, pair1 = 1;  // the two buffers the chain alternates between
  uint32_t prev_grid = 0, prev_seg_cap = 0;  // segments of the newest list and their capacity
  // its per-pass events
  hipEvent_t* evs = nullptr;
  uint8_t* ev_ix = nullptr;
  uint32_t ev_last = 0;

  int other_list(int cur) const { return cur == pair0 ? pair1 : pair0; }

  // "grid_pct": every launch with this share of its workgroups (the kernels loop over their chunks, so fewer
  // workgroups only means more trips each): leaves room on the CUs for the launches of ANOTHER cascade
  // running on another stream at the same time
  uint32_t scale_grid(uint32_t grid) const {
    return std::max<uint32_t>(1u, (uint32_t)((uint64_t)grid * (uint64_t)ctx->grid_pct / 100u));
  }
  // Capacity of a producer workgroup's list segment: it must hold every read the workgroup may be
  // offered -- its share of an identity list in chunks of `chunk` reads, or, reading a list, the
  // chunks it walks (chunk c belongs to segment c % in_nseg and goes to workgroup c % grid: of
  // in_nseg x depth chunks every grid-th one).
  // (0 = the segments would not fit the workspace: every launch adds at most grid x chunk entries of
  // rounding, kListSlack covers sixteen launches)
  uint32_t segment_capacity(uint32_t grid, uint64_t chunk, bool reads_list) const {
    uint64_t cap;
    if (!reads_list) {
      const uint64_t per_trip = chunk * grid;
      cap = ((n + per_trip - 1) / per_trip) * chunk;
    } else {
      const uint64_t depth = ((uint64_t)prev_seg_cap + chunk - 1) / chunk;  // chunks of the longest input segment
      cap = (((uint64_t)prev_grid * depth + grid - 1) / grid) * chunk;
    }
    if (cap * grid > n + mrg::kListSlack) return 0u;
    return (uint32_t)cap;
  }
  // a launch's grid -- per_cu workgroups per CU, at most max_grid, scaled -- and the capacity of its output segments when a
  // workgroup takes `chunk` reads per trip
  template <class P>
  int size_launch(P& p, uint32_t per_cu, uint32_t max_grid, uint64_t chunk, uint32_t* grid) const {
    *grid = scale_grid(std::min<uint32_t>((uint32_t)ctx->n_cu * per_cu, max_grid));
    p.out_seg_cap = segment_capacity(*grid, chunk, have_list);
    if (!p.out_seg_cap && n) return fail(MRG_ERR_ARG, "mrg_cascade_run: survivor lists outgrew the workspace");
    return MRG_OK;
  }

  // exact_dict_kernel and the FM kernels read index lists: a list that carries its reads is thinned into the other buffer
  // first (the spike-in pass and non-default plans only)
  int thin_list() {
    if (!have_list || !list_fat) return MRG_OK;
    const int other = other_list(cur_list);
    HIP_TRY(mrg::launch_list_thin(reinterpret_cast<const uint4*>(idx[cur_list]), idx[other], counts + cur_list * mrg::kMaxSegments,
                                  counts + other * mrg::kMaxSegments, prev_grid, prev_seg_cap, stream));
    cur_list = other;
    list_fat = false;
    return MRG_OK;
  }
  // list wiring of a launch: it reads the newest list (or the identity list) and, if anything runs behind it, writes the
  // chain's other buffer -- which becomes the newest list once the launch is issued (commit)
  template <class P>
  int wire_lists(P& p, bool wants_out) const {
    const int next_list = have_list ? other_list(cur_list) : pair0;
    p.idx_in = have_list ? idx[cur_list] : nullptr;
    p.in_count = counts + cur_list * mrg::kMaxSegments;
    p.in_nseg = prev_grid;
    p.in_seg_cap = prev_seg_cap;
    p.idx_out = wants_out ? idx[next_list] : nullptr;
    p.out_count = counts + next_list * mrg::kMaxSegments;
    return next_list;
  }
  template <class P>
  void commit(const P& p, int next_list, uint32_t grid, bool fat) {
    if (!p.idx_out) return;
    cur_list = next_list;
    have_list = true;
    list_fat = fat;
    prev_grid = grid;
    prev_seg_cap = p.out_seg_cap;
  }
  template <class P>
  void fill_outputs(P& p) const {
    p.pass_id = d_pass_id;
    p.ref_id = d_ref_id;
    p.pos = d_pos;
    p.mm = d_mm;
    p.packed = d_packed;
  }

  // the chain's events: the opening one, then one per pass boundary
  hipError_t begin_events(hipEvent_t* chain_evs, uint8_t* chain_ev_ix) {
    evs = chain_evs;
    ev_ix = chain_ev_ix;
    ev_last = 0;
    ev_ix[0] = 0;
    return timed ? hipEventRecord(evs[0], stream) : hipSuccess;
  }
  // pass i is issued: `fresh` = something was launched since the boundary before
  hipError_t mark(uint32_t i, bool fresh) {
    if (!fresh || !timed) {
      ev_ix[i + 1] = (uint8_t)ev_last;
      return hipSuccess;
    }
    ev_ix[i + 1] = (uint8_t)(i + 1);
    ev_last = i + 1;
    return hipEventRecord(evs[i + 1], stream);
  }

  int launch_exact(const Launch& L);
  int launch_fm(const Launch& L);
  int launch_fused(const Launch& L);
  int launch_seed(const Launch& L);
  int issue(const std::vector<Launch>& plan);
};

// one exact_dict_kernel launch (dict.hip) for pass L.first
int CascadeRun::launch_exact(const Launch& L) {
  const uint32_t i = L.first;
  const mrg_pass_cfg& c = passes[i];
  const DevLib& l = ctx->libs[c.lib];
  if (const int rc = thin_list()) return rc;
  mrg::ExactParams e;
  e.slots = reinterpret_cast<const uint4*>(l.dict_slots);
  e.log2_slots = l.dict_log2;
  e.key_bases = l.dict_key;
  e.kbits = (ctx->kmer_filter && c.seed_len >= (int32_t)mrg::kKmerBitsK) ? l.kbits : nullptr;
  fill_lib(e, l);
  e.simple_segs = l.simple ? 1u : 0u;
  e.reads = d_reads;
  e.lens = d_lens;
  e.n_total = (uint32_t)n;
  const int next_list = wire_lists(e, !L.ends_cascade);
  fill_outputs(e);
  e.counters = stats + (size_t)i * kStatsPerPass;
  fill_policy(e, c);
  e.pass_index = (int32_t)i;
  // (a workgroup takes chunks of 4096 reads: four per lane)
  uint32_t grid;
  if (const int rc = size_launch(e, 2u, 512u, mrg::kExactChunk, &grid)) return rc;
  ctx->last_lds[i] = 0u;
  ctx->last_mode[i] = 7u;
  ctx->last_group[i] = i;
  if (long_mask & window_bits(c))
    return fail(MRG_ERR_ARG, "mrg_cascade_run: internal: reads of more than 32 nt reached exact_dict_kernel (pass %u)", i);
  if (n) HIP_TRY(mrg::launch_exact_dict(e, grid, stream));
  ctx->last_variant[i] = (n && mrg::exact_dict_stretches(e, grid)) ? 16u : 0u;
  ctx->last_launches[i] += 1;
  HIP_TRY(mark(i, true));
  if (n && mrg::exact_dict_streams(e)) out_init = true;  // (every output of the batch is written: later launches write claims only)
  commit(e, next_list, grid, false);
  return MRG_OK;
}

// the classic path: one launch of match_kernel, stratum_kernel or pair_wave_kernel for strata [k_first, k_last] of pass L.first
int CascadeRun::launch_fm(const Launch& L) {
  const uint32_t i = L.first;
  const mrg_pass_cfg& c = passes[i];
  const DevLib& l = ctx->libs[c.lib];
  const bool by_pairs = L.kind == Launch::kPairs;
  // (the plan says whether the pass takes the pairs; the batch and "pair_impl" only pick the kernel that walks them.
  // pair_wave_kernel reads either list form; everything else launched here reads index lists)
  const bool pair_wave_route = by_pairs && pairs_by_wave(*ctx, dict_batch);
  if (!pair_wave_route)
    if (const int rc = thin_list()) return rc;
  mrg::MatchParams p;
  fill_lib(p, l);
  p.ctx = l.ctx;
  if (!ctx->use_ftab) p.tabs.k[0] = 0u;
  p.nblk = l.nblk;
  p.nsup = l.nsup;
  p.text_words = l.text_words;
  p.simple_segs = l.simple ? 1u : 0u;
  p.reads = d_reads;
  p.reads_hi = nullptr;
  p.lens = d_lens;
  p.nmask = nmask_eff;
  p.n_total = (uint32_t)n;
  const int next_list = wire_lists(p, !L.ends_cascade);
  p.in_stride = list_fat ? 4u : 1u;
  p.out_init = out_init ? 1u : 0u;
  p.k_first = L.k_first;
  p.k_last = L.k_last;
  p.count_processed = L.first_part ? 1u : 0u;
  // (the length hints only decide which passes are launched: every kernel reads the length array --
  // a caller whose equal hints do not describe the batch gets a skipped pass at worst, never a read
  // aligned with somebody else's length)
  p.uniform_len = 0u;
  fill_outputs(p);
  p.counters = stats + (size_t)i * kStatsPerPass;
  fill_policy(p, c);
  p.max_mm_seed = c.max_mm_seed;
  p.pass_index = (int32_t)i;
  p.wstop = (uint32_t)ctx->wstop;
  // a large library's wide intervals are pre-filtered by row context in the cooperative path:
  // send them there early (lane-serial verification of 100+ rows is what hurts short reads)
  p.wide_rows = l.ctx ? (uint32_t)std::min<int64_t>(ctx->wide_rows, ctx->ctx_wide_rows) : (uint32_t)ctx->wide_rows;

  // a small library's 9-mer bitmap (32 KB; only built for libraries whose text leaves room for
  // it next to a second workgroup) rides in LDS ("kmer_filter" = 0 switches it off)
  const bool use_kbits = small_lib(*ctx, l);
  const uint64_t kb_bytes = use_kbits ? (uint64_t)mrg::kKmerBitsWords * 4 : 0;
  p.kbits = use_kbits ? l.kbits : nullptr;
  const uint64_t txt_bytes = (uint64_t)l.text_words * 4, hard = 160 * 1024;
  const uint64_t overhead = (uint64_t)l.nsup * 16 + mrg::kMatchCtlBytes + kb_bytes;
  if (overhead > hard) return fail(MRG_ERR_ARG, "mrg_cascade_run: the superblock table of library %d does not fit LDS", c.lib);
  Residency res = match_residency(*ctx, l, overhead);
  // a strata launch of a 2-mismatch pass whose rows are compacted over the wave (stratum_kernel):
  // text in LDS when it fits, occ blocks always from L2
  const bool rows_kernel = c.max_mm_seed == 2 && ctx->force_lds_mode < 0 &&
                           (by_pairs || ctx->stratum_rows == 2 || (ctx->stratum_rows == 1 && L.k_first == L.k_last));
  p.pair_anchor = by_pairs ? l.pair_anchor : 0u;
  p.pair_jump = l.pair_jump;
  p.pair_rows = l.pair_rows;
  p.pair_jump_s = l.pair_jump_s;
  for (int t = 0; t < 3; ++t) {
    p.pair_row_off[t] = l.pair_row_off[t];
    p.pair_row_off_s[t] = l.pair_row_off_s[t];
  }
  const uint64_t rows_overhead = (uint64_t)l.nsup * 16 + mrg::kStratumCtlBytes + kb_bytes;
  bool rows_lds_text = false;
  if (rows_kernel) {
    if (rows_overhead > hard) return fail(MRG_ERR_ARG, "mrg_cascade_run: the superblock table of library %d does not fit LDS", c.lib);
    rows_lds_text = txt_bytes <= (uint64_t)ctx->lds_budget && rows_overhead + txt_bytes <= hard;
    res = rows_lds_text ? Residency{3, txt_bytes} : Residency{0, 0};
  }
  // one-word reads without N through the anchor pairs: pair_wave_kernel (dict.hip; every wave on its own, items
  // and rows compacted over the wave; nothing staged in LDS but the wave's 256 reads)
  const bool pair_wave = pair_wave_route && rows_kernel;
  if (pair_wave) res = Residency{0, 0};
  const uint32_t lds_total = pair_wave ? mrg::pair_wave_lds_total() : (uint32_t)((rows_kernel ? rows_overhead : overhead) + res.bytes);
  const uint32_t per_cu = pair_wave ? std::min<uint32_t>(5u, (160u * 1024u) / lds_total) : ((lds_total * 2u <= 160u * 1024u) ? 2u : 1u);
  // a workgroup's segment must hold every read it may be offered
  uint32_t grid;
  if (const int rc = size_launch(p, per_cu, mrg::kMaxSegments, 1024, &grid)) return rc;
  ctx->last_lds[i] = (uint32_t)res.bytes;
  ctx->last_mode[i] = !rows_kernel ? (uint32_t)res.mode : pair_wave ? 11u : (rows_lds_text ? 5u : 6u);
  ctx->last_group[i] = i;
  ctx->last_kbits_log2[i] = use_kbits ? 18u : 0u;
  ctx->last_pair_anchor[i] = p.pair_anchor;
  if (long_mask && !pair_wave && (long_mask & window_bits(c)))
    return fail(MRG_ERR_ARG, "mrg_cascade_run: internal: reads of more than 32 nt reached a one-word kernel (pass %u)", i);
  if (n && pair_wave) {
    p.reads_hi = long_mask ? d_reads + n : nullptr;
    ctx->last_variant[i] = long_mask ? 8u : 0u;
    HIP_TRY(mrg::launch_pair_wave(p, grid, stream));
  } else if (n && rows_kernel) {
    HIP_TRY(mrg::launch_stratum(p, words_eff, rows_lds_text, grid, lds_total, stream));
  } else if (n) {
    HIP_TRY(mrg::launch_match(p, words_eff, res.mode, grid, lds_total, stream));
  }
  ctx->last_launches[i] += 1;
  if (L.last_part) HIP_TRY(mark(i, true));
  commit(p, next_list, grid, pair_wave);
  return MRG_OK;
}

// one fused_kernel launch for the running passes L.members
int CascadeRun::launch_fused(const Launch& L) {
  const std::vector<uint32_t>& members = L.members;
  const uint32_t n_sub = (uint32_t)members.size();
  for (uint32_t q = 0; q < n_sub; ++q)
    if (long_mask & window_bits(passes[members[q]]))
      return fail(MRG_ERR_ARG, "mrg_cascade_run: internal: reads of more than 32 nt reached fused_kernel<1> (pass %u)", members[q]);
  mrg::FusedParams fp;
  std::memset(&fp, 0, sizeof fp);
  fp.n_sub = n_sub;
  // which sub-passes filter seed pieces with their library's 9-mer bitmap
  uint32_t lg[mrg::kMaxFused];
  for (uint32_t q = 0; q < n_sub; ++q) lg[q] = small_lib(*ctx, ctx->libs[passes[members[q]].lib]) ? 18u : 0u;
  // one 1024-thread workgroup per CU (128 VGPRs per lane), so the whole LDS is its own
  const uint64_t fixed = mrg::fused_fixed_lds_bytes();
  const uint64_t lds_cap = 160 * 1024;
  const uint64_t budget = std::min<uint64_t>((uint64_t)std::max<int64_t>(ctx->lds_budget, (int64_t)fixed), lds_cap) - fixed;
  // rounds: the sub-passes of a run of bitmap-filtered libraries are looked up together (few
  // items per read), with "round_large" = 1 so are those of a run of large ones (measured equal,
  // default 0: every unclaimed read has items in each of them)
  fp.n_rounds = 0;
  for (uint32_t q = 0; q < n_sub;) {
    uint32_t e = q + 1;
    if (lg[q] || ctx->round_large)
      while (e < n_sub && (lg[e] != 0) == (lg[q] != 0) && e - q < mrg::kMaxRoundSubs) ++e;
    fp.round_first[fp.n_rounds] = (uint8_t)q;
    fp.round_count[fp.n_rounds] = (uint8_t)(e - q);
    ++fp.n_rounds;
    q = e;
  }
  // the 9-mer table of each bitmap round: one entry per code with a bit per sub-pass, as many
  // codes (2^18 = every 9-mer, else folded: entry h = OR of the codes = h mod 2^log2) as the LDS
  // left by the other rounds' tables allows
  uint32_t n_tab_rounds = 0;
  for (uint32_t r = 0; r < fp.n_rounds; ++r) n_tab_rounds += lg[fp.round_first[r]] ? 1u : 0u;
  uint32_t kb_words = 0;
  for (uint32_t q = 0; q < n_sub; ++q) {
    const uint32_t i = members[q];
    const mrg_pass_cfg& c = passes[i];
    DevLib& l = ctx->libs[c.lib];
    mrg::SubPass& sp = fp.sub[q];
    fill_lib(sp, l);
    sp.ctx = l.ctx;
    sp.sa16 = reinterpret_cast<const uint4*>(l.sa16);
    if (!ctx->use_ftab) sp.tabs.k[0] = 0u;
    sp.nmask = nmask_eff;
    sp.counters = stats + (size_t)i * kStatsPerPass;
    sp.simple_segs = l.simple ? 1u : 0u;
    sp.kb_bit = 0xFFu;
    fill_policy(sp, c);
    sp.max_mm_seed = c.max_mm_seed;
    sp.pass_index = (int32_t)i;
    sp.pair_anchor = 0u;
    // (with "round_large" the large libraries' sub-passes share a round: no reads are set aside for the three anchor pairs)
    if (const int64_t A = ctx->round_large ? 0 : three_anchor_tables(*ctx, c, l))
      if (const int rc = bind_bpair(l, A, stream, &sp.pair_jump, &sp.pair_rows, sp.pair_row_off, &sp.pair_anchor)) return rc;
    ctx->last_pair_anchor[i] = sp.pair_anchor;
    ctx->last_lds[i] = 0u;
    ctx->last_mode[i] = 4u;
    ctx->last_group[i] = members[0];
    ctx->last_kbits_log2[i] = 0u;
  }
  for (uint32_t r = 0; r < fp.n_rounds; ++r) {
    const uint32_t q0 = fp.round_first[r], nq = fp.round_count[r];
    fp.round_kb_log2[r] = 0;
    fp.round_kb_bits[r] = 0;
    fp.round_kb_off[r] = 0;
    fp.round_kb_src[r] = nullptr;
    if (!lg[q0]) continue;
    const uint32_t bits = nq <= 4 ? 4u : 8u;
    uint32_t log2c = 18;
    while (log2c > 13 && ((uint64_t)(1u << log2c) * bits / 8) * n_tab_rounds > budget) --log2c;
    if (((uint64_t)(1u << log2c) * bits / 8) * n_tab_rounds > budget) {  // no room: unfiltered
      for (uint32_t q = q0; q < q0 + nq; ++q) ctx->last_kbits_log2[members[q]] = 255u;
      continue;
    }
    std::string key;
    for (uint32_t q = q0; q < q0 + nq; ++q) key += std::to_string(passes[members[q]].lib) + ",";
    key += "|" + std::to_string(log2c) + "|" + std::to_string(bits);
    uint32_t* d_tab = nullptr;
    for (auto& kv : ctx->round_tables)
      if (kv.first == key) d_tab = kv.second;
    if (!d_tab) {
      std::vector<uint32_t> tab(((size_t)1 << log2c) * bits / 32, 0u);
      for (uint32_t q = q0; q < q0 + nq; ++q) {
        const std::vector<uint32_t>& kbh = ctx->libs[passes[members[q]].lib].kbits_host;
        for (uint32_t c = 0; c < (1u << 18); ++c) {
          if (!((kbh[c >> 5] >> (c & 31u)) & 1u)) continue;
          const uint64_t bit = (uint64_t)(c & ((1u << log2c) - 1u)) * bits + (q - q0);
          tab[bit >> 5] |= 1u << (bit & 31u);
        }
      }
      HIP_TRY(hipMalloc((void**)&d_tab, tab.size() * 4));
      HIP_TRY(hipMemcpy(d_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
      ctx->round_tables.emplace_back(key, d_tab);
    }
    fp.round_kb_src[r] = d_tab;
    fp.round_kb_off[r] = kb_words;
    fp.round_kb_log2[r] = (uint8_t)log2c;
    fp.round_kb_bits[r] = (uint8_t)bits;
    const uint32_t words = (uint32_t)(((size_t)1 << log2c) * bits / 32);
    kb_words += words;
    for (uint32_t q = q0; q < q0 + nq; ++q) {
      fp.sub[q].kb_bit = q - q0;
      ctx->last_lds[members[q]] = words * 4u / nq;
      ctx->last_kbits_log2[members[q]] = log2c;
    }
  }
  fp.kb_words = kb_words;
  fp.reads = d_reads;
  fp.lens = d_lens;
  fp.nmask = nmask_eff;
  fp.n_total = (uint32_t)n;
  fp.uniform_len = 0u;  // (see launch_fm)
  if (const int rc = thin_list()) return rc;
  const int next_list = wire_lists(fp, !L.ends_cascade);
  fill_outputs(fp);
  fp.wstop = (uint32_t)ctx->wstop;
  const uint32_t lds_total = kb_words * 4u + (uint32_t)fixed;
  // 128 VGPRs per lane (no spills in the pipelined walk): 16 waves = one workgroup per CU
  uint32_t grid;
  if (const int rc = size_launch(fp, 1u, mrg::kMaxSegments, 1024, &grid)) return rc;
  if (n) HIP_TRY(mrg::launch_fused(fp, words_eff, grid, lds_total, stream));
  ctx->last_launches[L.first] = 1;
  // (the hint-skipped passes inside the group share its event)
  for (uint32_t q = L.first; q < L.end; ++q) HIP_TRY(mark(q, q == L.first));
  commit(fp, next_list, grid, false);
  return MRG_OK;
}

// one seed_kernel / wave_seed_kernel launch (dict.hip) for the units of L
int CascadeRun::launch_seed(const Launch& L) {
  const std::vector<SeedUnitPlan>& plan = L.units;
  mrg::SeedParams sp;
  std::memset(&sp, 0, sizeof sp);
  sp.n_units = (uint32_t)plan.size();
  for (uint32_t u = 0; u < sp.n_units; ++u) {
    mrg::SeedUnit& un = sp.unit[u];
    const mrg_pass_cfg& c0 = passes[plan[u].members[0]];
    un.kind = plan[u].kind;
    const DevLib* fm = &ctx->libs[c0.lib];
    SeedLib* sl = nullptr;
    if (un.kind == 0u) {
      std::vector<int32_t> ids;
      for (uint32_t i : plan[u].members) ids.push_back(passes[i].lib);
      if (const int rc = get_seed_lib(ctx, ids, &sl)) return rc;
      fm = &sl->lib;
      un.kbits = sl->kbits;
    } else {
      un.slots = reinterpret_cast<const uint4*>(fm->dict_slots);
      un.log2_slots = fm->dict_log2;
      un.key_bases = fm->dict_key;
    }
    // an FM unit of one library that wants its three-anchor tables (wave_seed_kernel parks those reads for the three anchor
    // pairs); a unit over several libraries is a small-library unit, a stratum-0 unit is a dictionary unit: neither has any
    if (const int64_t A = (un.kind == 0u && plan[u].members.size() == 1 && !plan[u].stratum0)
                              ? three_anchor_tables(*ctx, c0, ctx->libs[c0.lib]) : 0)
      if (const int rc = bind_bpair(ctx->libs[c0.lib], A, stream, &un.bpair_jump, &un.bpair_rows, un.bpair_row_off, &un.bpair_anchor))
        return rc;
    fill_lib(un, *fm);
    un.sa16 = reinterpret_cast<const uint4*>(fm->sa16);
    un.buckets = ctx->seed_buckets ? reinterpret_cast<const uint4*>(fm->buckets) : nullptr;
    un.bucket_k = fm->bucket_k;
    un.pos_rows = (ctx->seed_buckets && ctx->pos_scan) ? reinterpret_cast<const uint4*>(fm->pos_rows) : nullptr;
    un.simple_segs = fm->simple ? 1u : 0u;
    fill_window(un, c0);
    un.max_mm_seed = plan[u].stratum0 ? 0 : c0.max_mm_seed;
    un.n_members = (uint32_t)plan[u].members.size();
    un.min_seed_len = 0x7FFFFFFF;
    un.max_total = 0;
    for (uint32_t mi = 0; mi < un.n_members; ++mi) {
      const uint32_t i = plan[u].members[mi];
      const mrg_pass_cfg& c = passes[i];
      un.m[mi].pass_index = (int32_t)i;
      un.m[mi].seed_len = c.seed_len;
      un.m[mi].max_mm_total = c.max_mm_total;
      un.m[mi].entry_lo = sl ? sl->entry_lo[mi] : 0u;
      un.min_seed_len = std::min(un.min_seed_len, c.seed_len);
      un.max_total = std::max(un.max_total, c.max_mm_total);
      if (plan[u].stratum0) continue;  // (that pass has its own launch afterwards and reports that one)
      ctx->last_lds[i] = 0u;
      ctx->last_mode[i] = 8u;
      ctx->last_group[i] = L.first;
      ctx->last_kbits_log2[i] = un.kbits ? 22u : 0u;
    }
  }
  // which kernel: by default (-1) the tile kernel for the small libraries' launch (its waves are bound by what
  // they do per read; with more registers and fewer waves the wave kernel only draws level, and its parked
  // reads leave the list's order) and the wave kernel, 96 registers, for a launch on large libraries (bound by
  // the L2 misses of its bucket / slot lines: no barrier, nothing parked but overflowing buckets: 2.08 -> 1.8 ms)
  {
    const int64_t impl = ctx->seed_impl >= 0 ? ctx->seed_impl : (L.small ? 0 : 2);
    sp.impl = impl ? 1u : 0u;
    sp.wave_regs = impl >= 2 ? 1u : 0u;
    for (uint32_t q = L.first; q < L.end; ++q)
      ctx->last_variant[q] = (sp.impl ? ((sp.wave_regs & 1u) ? 2u : 1u) : 0u) | ((have_list && list_fat) ? 4u : 0u) | (long_mask ? 8u : 0u);
  }
  sp.reads_per_lane = 1u;
  sp.item_cap = mrg::kSeedThreads * sp.reads_per_lane * 2u;
  sp.row_cap = sp.impl ? 192u : (L.small ? 1024u : 2048u);
  sp.stats = stats;
  sp.reads = d_reads;
  sp.reads_hi = long_mask ? d_reads + n : nullptr;
  sp.lens = d_lens;
  sp.n_total = (uint32_t)n;
  const int next_list = wire_lists(sp, !L.ends_cascade);
  sp.in_stride = list_fat ? 4u : 1u;
  sp.out_init = out_init ? 1u : 0u;
  fill_outputs(sp);
  {
    // which instantiation the launch gets: mrg_pass_stats.lds_mode 8 = seed_kernel<false, 8>, 9 = <true, 6>
    bool with_buckets = false;
    for (uint32_t u = 0; u < sp.n_units; ++u) with_buckets |= sp.unit[u].kind == 0u && sp.unit[u].buckets != nullptr;
    if (with_buckets)
      for (uint32_t q = L.first; q < L.end; ++q)
        if (ctx->last_mode[q] == 8u) ctx->last_mode[q] = 9u;
    // mrg_pass_stats.pair_anchor, as a fused launch reports it: only wave_seed_kernel's instantiation with buckets
    // parks the reads of 3 A .. 4 A - 1 seed bases for the three anchor pairs
    for (uint32_t u = 0; u < sp.n_units; ++u)
      if (sp.impl && with_buckets && sp.unit[u].bpair_anchor)
        for (uint32_t i : plan[u].members) ctx->last_pair_anchor[i] = sp.unit[u].bpair_anchor;
  }
  const uint32_t per_cu = ctx->seed_wgs > 0 ? (uint32_t)ctx->seed_wgs : mrg::seed_wgs_per_cu(sp);
  uint32_t grid;
  if (const int rc = size_launch(sp, per_cu, mrg::kMaxSegments, (uint64_t)mrg::kSeedThreads * sp.reads_per_lane, &grid)) return rc;
  sp.walk_buf = nullptr;
  sp.walk_cap = 0;
  sp.walk_diag = (uint32_t)ctx->walk_diag;
  if (sp.impl) {
    // units with position lists (round 6): every wave keeps the records of the reads it leaves to them in its own stretch
    // of a context buffer and walks the lists behind its stream
    bool lists = false;
    for (uint32_t u = 0; u < sp.n_units; ++u) lists |= sp.unit[u].kind == 0u && sp.unit[u].pos_rows != nullptr;
    if (lists) {
      sp.walk_buf = ws_walk;
      sp.walk_cap = (uint32_t)std::min<int64_t>(std::max<int64_t>(ctx->walk_cap, 0), (int64_t)kWalkCap);
    }
  }
  if (n) HIP_TRY(mrg::launch_seed(sp, grid, stream));
  ctx->last_launches[L.first] = 1;
  for (uint32_t q = L.first; q < L.end; ++q) HIP_TRY(mark(q, q == L.first));
  commit(sp, next_list, grid, true);
  return MRG_OK;
}

// the launches of the chain's plan, in order; a pass no launch covers was skipped by the length hint and shares the event of
// the boundary before it
int CascadeRun::issue(const std::vector<Launch>& plan) {
  uint32_t next = 0;
  for (const Launch& L : plan) {
    for (; next < L.first; ++next) HIP_TRY(mark(next, false));
    const int rc = L.kind == Launch::kExact ? launch_exact(L)
                   : L.kind == Launch::kFused ? launch_fused(L)
                   : L.kind == Launch::kSeed ? launch_seed(L)
                                             : launch_fm(L);
    if (rc != MRG_OK) return rc;
    next = L.end;
  }
  return MRG_OK;
}

// mrg_cascade_run / mrg_cascade_run_packed: d_packed != null = the one-array output form
int cascade_run_impl(mrg_ctx* ctx, const uint64_t* d_reads, uint32_t words_per_read,
                    const uint8_t* d_lens, const uint64_t* d_nmask, uint64_t n,
                    const mrg_pass_cfg* passes, uint32_t n_pass, int8_t* d_pass_id,
                    int32_t* d_ref_id, int32_t* d_pos, uint8_t* d_mm, uint32_t* d_packed, uint64_t* d_pass_counts,
                    void* d_workspace, uint64_t workspace_bytes, void* stream_) {
  if (!ctx || !passes || !d_workspace) return fail(MRG_ERR_ARG, "mrg_cascade_run: null argument");
  if (n && (!d_reads || !d_lens || (!d_packed && (!d_pass_id || !d_ref_id || !d_pos || !d_mm))))
    return fail(MRG_ERR_ARG, "mrg_cascade_run: null read/output buffers");
  if (d_packed && n_pass > 15) return fail(MRG_ERR_ARG, "mrg_cascade_run_packed: at most 15 passes fit the packed word");
  if (n_pass == 0 || n_pass > MRG_MAX_PASSES)
    return fail(MRG_ERR_ARG, "mrg_cascade_run: n_pass %u not in [1,%d]", n_pass, MRG_MAX_PASSES);
  if (words_per_read != 1 && words_per_read != 2 && words_per_read != 4 && words_per_read != 8)
    return fail(MRG_ERR_ARG, "mrg_cascade_run: words_per_read must be 1, 2, 4 or 8 (got %u)", words_per_read);
  if (n >= 0xfffffff0ull) return fail(MRG_ERR_ARG, "mrg_cascade_run: at most 2^32-16 reads per call");
  uint64_t need = 0;
  mrg_cascade_workspace_bytes(n, &need);
  if (workspace_bytes < need)
    return fail(MRG_ERR_ARG, "mrg_cascade_run: workspace %llu < %llu bytes",
                (unsigned long long)workspace_bytes, (unsigned long long)need);
  for (uint32_t i = 0; i < n_pass; ++i) {
    const mrg_pass_cfg& c = passes[i];
    if (c.lib < 0 || (size_t)c.lib >= ctx->libs.size())
      return fail(MRG_ERR_ARG, "mrg_cascade_run: pass %u names unknown library %d", i, c.lib);
    if (c.max_mm_seed < 0 || c.max_mm_seed > 3 || c.max_mm_total < c.max_mm_seed || c.trim5 < 0 ||
        c.trim5 > 31 || c.trim3 < 0 || c.seed_len < 1)
      return fail(MRG_ERR_ARG, "mrg_cascade_run: pass %u has an invalid policy", i);
  }
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t stream = (hipStream_t)stream_;
  if (!ctx->ev_ready) {
    for (auto& e : ctx->ev) HIP_TRY(hipEventCreate(&e));
    for (auto& e : ctx->ev0) HIP_TRY(hipEventCreate(&e));
    ctx->ev_ready = true;
  }

  // one-word reads without N: the batches the dictionary kernels (dict.hip) take.  A batch with
  // longer reads, reads with N or very short reads is SPLIT: the reads of split_min_len .. 32 nt
  // without N -- most of any small-RNA read set -- go through the cascade as the one-word batch they
  // are (the kernels read word 0 of the plane-major array), the rest through the FM kernels (whose
  // backtracking search does not mind a 16-nt read's 8-base seeds); two cascades over disjoint lists,
  // one after the other, adding to the same counters.  (The length hint only says whether a one-word
  // batch may hold such short reads: a wrong hint costs time, never a result.)
  const bool dict_batch = ctx->dict && words_per_read == 1 && !d_nmask;
  const bool split = ctx->dict && ctx->split_mixed && n > 0 && ctx->force_lds_mode < 0 &&
                     (!dict_batch || ctx->hint_min_len < ctx->split_min_len) &&
                     (ctx->hint_min_len <= 32 || (ctx->long_lane && words_per_read >= 2 && ctx->hint_min_len <= 63)) &&
                     ctx->hint_max_len >= ctx->split_min_len;  // (some read may be on either side)
  // the one-word lane of a split batch may take reads of 33..63 nt ("long_lane"): the lengths its plan lets in
  const bool lane_long = split && ctx->long_lane && words_per_read >= 2 && ctx->hint_max_len > 32;
  // chain 0: the whole batch, or the FM side of a split one (long reads and reads with N); chain 1: the one-word lane
  std::vector<Launch> plans[2];
  plans[0] = plan_chain(*ctx, passes, n_pass, n, split ? false : dict_batch, false);
  if (split) plans[1] = plan_chain(*ctx, passes, n_pass, n, true, lane_long);
  const uint64_t long_plan = lane_long ? lane_long_mask(*ctx, passes, plans[1]) : 0;

  char* ws = (char*)d_workspace;
  CascadeRun run{ctx, passes, n_pass, d_reads, d_lens, n, d_pass_id, d_ref_id, d_pos, d_mm, d_packed};
  for (int b = 0; b < 3; ++b) run.idx[b] = (uint32_t*)(ws + b * ws_idx_bytes(n));
  run.counts = (uint32_t*)(ws + 3 * ws_idx_bytes(n));
  run.stats = (uint64_t*)(ws + 3 * ws_idx_bytes(n) + kWsCountsBytes);
  run.ws_walk = (uint4*)(ws + 3 * ws_idx_bytes(n) + kWsCountsBytes + kWsStatsBytes);
  run.stream = stream;
  run.timed = !ctx->fused_step;
  run.dict_batch = dict_batch;
  run.words_eff = words_per_read;
  run.nmask_eff = d_nmask;
  // per-pass counters only; the outputs need no memset (the last pass writes the
  // "unannotated" values for whatever it does not claim)
  HIP_TRY(hipMemsetAsync(run.stats, 0, kWsStatsBytes, stream));
  ctx->last_timed = run.timed;
  HIP_TRY(run.begin_events(ctx->ev, ctx->ev_ix));
  for (uint32_t i = 0; i < n_pass; ++i) {
    ctx->last_lds[i] = 0;
    ctx->last_mode[i] = 0;
    ctx->last_group[i] = i;
    ctx->last_launches[i] = 0;
    ctx->last_kbits_log2[i] = 0;
    ctx->last_pair_anchor[i] = 0;
    ctx->last_variant[i] = 0;
  }
  uint32_t split_grid = 0, split_cap = 0;
  if (split) {
    mrg::SplitParams sp;
    sp.lens = d_lens;
    sp.nmask = d_nmask;
    sp.n_total = (uint32_t)n;
    sp.long_ok = long_plan;
    sp.nmask_hi = (d_nmask && words_per_read >= 2) ? d_nmask + n : nullptr;
    sp.min_len = (uint32_t)ctx->split_min_len;
    split_grid = std::min<uint32_t>((uint32_t)ctx->n_cu * 2u, mrg::kMaxSegments);
    split_cap = run.segment_capacity(split_grid, 1024, false);
    if (!split_cap) return fail(MRG_ERR_ARG, "mrg_cascade_run: survivor lists outgrew the workspace");
    sp.seg_cap = split_cap;
    sp.idx_rest = run.idx[0];
    sp.cnt_rest = run.counts;
    sp.idx_short = run.idx[2];
    sp.cnt_short = run.counts + 2 * mrg::kMaxSegments;
    HIP_TRY(mrg::launch_split(sp, split_grid, stream));
  }
  ctx->last_split = split ? 1u : 0u;
  for (int chain = 0; chain < (split ? 2 : 1); ++chain) {
    if (split) {
      // split_kernel wrote index lists: the long reads and the reads with N in buffer 0 (alternating with 1), the one-word
      // reads parked in buffer 2 (alternating with 1)
      run.have_list = true;
      run.list_fat = false;
      run.out_init = false;
      run.prev_grid = split_grid;
      run.prev_seg_cap = split_cap;
      run.pair0 = run.cur_list = chain == 0 ? 0 : 2;
      run.pair1 = 1;
      run.dict_batch = chain == 1;
      if (chain == 1) {
        run.words_eff = 1u;
        run.nmask_eff = nullptr;
        run.long_mask = long_plan;  // (... and the reads of 33..63 nt the plan lets in)
      }
      // (each cascade records its own per-pass events: mrg_pass_stats.ms / .ms_rest)
      HIP_TRY(run.begin_events(chain == 0 ? ctx->ev0 : ctx->ev, chain == 0 ? ctx->ev0_ix : ctx->ev_ix));
    }
    const int rc = run.issue(plans[chain]);
    if (rc != MRG_OK) return rc;
  }
  ctx->pending_export_out = nullptr;
  if (d_pass_counts) {
    if (ctx->fused_step) {
      ctx->pending_export_out = d_pass_counts;  // (the tally launch behind this cascade copies them: mrg_tally_run*)
      ctx->pending_export_stream = stream;
    } else {
      HIP_TRY(mrg::launch_export_pass_counts(run.stats, n_pass, d_pass_counts, stream));
    }
  }
  ctx->last_stream = stream;
  ctx->last_stats_dev = run.stats;
  ctx->last_n_pass = n_pass;
  ++ctx->run_id;
  // a length hint describes ONE batch: it never outlives the run it was set for
  ctx->hint_min_len = 0;
  ctx->hint_max_len = 255;
  return MRG_OK;
}
}  // namespace

extern "C" {

int mrg_cascade_run(mrg_ctx* ctx, const uint64_t* d_reads, uint32_t words_per_read, const uint8_t* d_lens, const uint64_t* d_nmask,
                    uint64_t n, const mrg_pass_cfg* passes, uint32_t n_pass, int8_t* d_pass_id, int32_t* d_ref_id, int32_t* d_pos,
                    uint8_t* d_mm, uint64_t* d_pass_counts, void* d_workspace, uint64_t workspace_bytes, void* stream) {
  return cascade_run_impl(ctx, d_reads, words_per_read, d_lens, d_nmask, n, passes, n_pass, d_pass_id, d_ref_id, d_pos, d_mm, nullptr,
                          d_pass_counts, d_workspace, workspace_bytes, stream);
}

int mrg_cascade_run_packed(mrg_ctx* ctx, const uint64_t* d_reads, uint32_t words_per_read, const uint8_t* d_lens,
                           const uint64_t* d_nmask, uint64_t n, const mrg_pass_cfg* passes, uint32_t n_pass, uint32_t* d_packed,
                           uint64_t* d_pass_counts, void* d_workspace, uint64_t workspace_bytes, void* stream) {
  if (n && !d_packed) return fail(MRG_ERR_ARG, "mrg_cascade_run_packed: null output buffer");
  return cascade_run_impl(ctx, d_reads, words_per_read, d_lens, d_nmask, n, passes, n_pass, nullptr, nullptr, nullptr, nullptr,
                          d_packed, d_pass_counts, d_workspace, workspace_bytes, stream);
}

int mrg_pack_assignments(mrg_ctx* ctx, const int8_t* d_pass_id, const int32_t* d_ref_id, const int32_t* d_pos, const uint8_t* d_mm,
                         uint64_t n, uint32_t* d_packed, void* stream) {
  if (!ctx) return fail(MRG_ERR_ARG, "mrg_pack_assignments: null argument");
  if (n && (!d_pass_id || !d_ref_id || !d_pos || !d_mm || !d_packed)) return fail(MRG_ERR_ARG, "mrg_pack_assignments: null buffers");
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(mrg::launch_pack_assignments(d_pass_id, d_ref_id, d_pos, d_mm, n, d_packed, (hipStream_t)stream));
  return MRG_OK;
}

int mrg_cascade_run_id(const mrg_ctx* ctx, uint64_t* run_id) {
  if (!ctx || !run_id) return fail(MRG_ERR_ARG, "mrg_cascade_run_id: null argument");
  *run_id = ctx->run_id;
  return MRG_OK;
}

int mrg_cascade_stats(mrg_ctx* ctx, mrg_pass_stats* out, uint32_t n_pass) {
  if (!ctx || !out) return fail(MRG_ERR_ARG, "mrg_cascade_stats: null argument");
  if (!ctx->last_stats_dev || n_pass != ctx->last_n_pass)
    return fail(MRG_ERR_ARG, "mrg_cascade_stats: no matching cascade run (%u vs %u passes)", n_pass,
                ctx->last_n_pass);
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipStreamSynchronize(ctx->last_stream));
  uint64_t host[MRG_MAX_PASSES * kStatsPerPass];
  HIP_TRY(hipMemcpy(host, ctx->last_stats_dev, (size_t)n_pass * kStatsPerPass * 8, hipMemcpyDeviceToHost));
  for (uint32_t i = 0; i < n_pass; ++i) {
    out[i].processed = host[i * kStatsPerPass + 0];
    out[i].aligned = host[i * kStatsPerPass + 1];
    out[i].steps = host[i * kStatsPerPass + 2];
    out[i].candidates = host[i * kStatsPerPass + 3];
    out[i].lookups = host[i * kStatsPerPass + 4];
    float ms = 0.f;
    if (ctx->last_timed) HIP_TRY(hipEventElapsedTime(&ms, ctx->ev[ctx->ev_ix[i]], ctx->ev[ctx->ev_ix[i + 1]]));
    out[i].ms = ms;
    out[i].ms_rest = 0.f;
    if (ctx->last_split && ctx->last_timed) HIP_TRY(hipEventElapsedTime(&out[i].ms_rest, ctx->ev0[ctx->ev0_ix[i]], ctx->ev0[ctx->ev0_ix[i + 1]]));
    out[i].lds_bytes = ctx->last_lds[i];
    out[i].lds_mode = ctx->last_mode[i];
    out[i].group = ctx->last_group[i];
    out[i].n_launches = ctx->last_launches[i];
    out[i].kbits_log2 = ctx->last_kbits_log2[i];
    out[i].pair_anchor = ctx->last_pair_anchor[i];
    out[i].variant = ctx->last_variant[i];
    out[i].reserved = 0;
  }
  return MRG_OK;
}

// ------------------------------------------------------- reads of any length
namespace {

// the library half of a long-read descriptor (the policy half is its caller's): everything from global memory
void fill_long_lib(mrg::LongPass& q, const mrg_ctx& ctx, const DevLib& l) {
  std::memset(&q, 0, sizeof q);
  fill_lib(q, l);
  if (!ctx.use_ftab || !l.ftab) q.tabs.k[0] = 0u;
  q.simple_segs = l.simple ? 1u : 0u;
}

}  // namespace

int mrg_cascade_run_long(mrg_ctx* ctx, const uint64_t* d_words, const uint64_t* d_nmask, const uint64_t* d_word_off,
                         const uint32_t* d_lens, uint64_t n, const mrg_pass_cfg* passes, uint32_t n_pass, int8_t* d_pass_id,
                         int32_t* d_ref_id, int32_t* d_pos, uint8_t* d_mm, uint64_t* d_pass_counts, mrg_pass_stats* stats,
                         void* stream_) {
  if (!ctx || !passes) return fail(MRG_ERR_ARG, "mrg_cascade_run_long: null argument");
  if (n && (!d_words || !d_word_off || !d_lens || !d_pass_id || !d_ref_id || !d_pos || !d_mm))
    return fail(MRG_ERR_ARG, "mrg_cascade_run_long: null read/output buffers");
  if (n_pass == 0 || n_pass > MRG_MAX_PASSES)
    return fail(MRG_ERR_ARG, "mrg_cascade_run_long: n_pass %u not in [1,%d]", n_pass, MRG_MAX_PASSES);
  if (n >= 0xfffffff0ull) return fail(MRG_ERR_ARG, "mrg_cascade_run_long: at most 2^32-16 reads per call");
  std::vector<mrg::LongPass> host(n_pass);
  for (uint32_t i = 0; i < n_pass; ++i) {
    const mrg_pass_cfg& c = passes[i];
    if (c.lib < 0 || (size_t)c.lib >= ctx->libs.size())
      return fail(MRG_ERR_ARG, "mrg_cascade_run_long: pass %u names unknown library %d", i, c.lib);
    if (c.max_mm_seed < 0 || c.max_mm_seed > 3 || c.max_mm_total < c.max_mm_seed || c.max_mm_total > 255 || c.trim5 < 0 ||
        c.trim3 < 0 || c.seed_len < 1)
      return fail(MRG_ERR_ARG, "mrg_cascade_run_long: pass %u has an invalid policy", i);
    mrg::LongPass& q = host[i];
    fill_long_lib(q, *ctx, ctx->libs[c.lib]);
    fill_policy(q, c);
    q.max_mm_seed = c.max_mm_seed;
  }
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t stream = (hipStream_t)stream_;
  struct Scratch {
    void* p = nullptr;
    ~Scratch() { (void)hipFree(p); }
  } scratch;
  const size_t table_bytes = ((size_t)n_pass * sizeof(mrg::LongPass) + 255) / 256 * 256;
  const size_t stats_bytes = (size_t)n_pass * kStatsPerPass * 8;
  HIP_TRY(hipMalloc(&scratch.p, table_bytes + stats_bytes));
  uint64_t* d_stats = reinterpret_cast<uint64_t*>((char*)scratch.p + table_bytes);
  HIP_TRY(hipMemcpyAsync(scratch.p, host.data(), (size_t)n_pass * sizeof(mrg::LongPass), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipMemsetAsync(d_stats, 0, stats_bytes, stream));
  struct Events {  // (destroyed on every way out: advisor, round 5)
    hipEvent_t a = nullptr, b = nullptr;
    ~Events() {
      if (a) (void)hipEventDestroy(a);
      if (b) (void)hipEventDestroy(b);
    }
  } evs_long;
  HIP_TRY(hipEventCreate(&evs_long.a));
  HIP_TRY(hipEventCreate(&evs_long.b));
  const hipEvent_t e0 = evs_long.a, e1 = evs_long.b;
  hipError_t err = hipEventRecord(e0, stream);
  if (err == hipSuccess && n) {
    mrg::LongParams p;
    std::memset(&p, 0, sizeof p);
    p.pass = reinterpret_cast<const mrg::LongPass*>(scratch.p);
    p.n_pass = n_pass;
    p.words = d_words;
    p.nmask = d_nmask;
    p.word_off = d_word_off;
    p.lens = d_lens;
    p.n = (uint32_t)n;
    p.wstop = (uint32_t)ctx->wstop;
    p.pass_id = d_pass_id;
    p.ref_id = d_ref_id;
    p.pos = d_pos;
    p.mm = d_mm;
    p.counters = d_stats;
    p.pass_counts = d_pass_counts;
    // one wave per read, four per workgroup; more reads than resident waves: the kernel strides
    const uint64_t want = (n + 3) / 4;
    const uint32_t grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(want, (uint64_t)ctx->n_cu * 8u));
    err = mrg::launch_long_reads(p, grid, stream);
  }
  if (err == hipSuccess) err = hipEventRecord(e1, stream);
  uint64_t got[MRG_MAX_PASSES * kStatsPerPass];
  if (err == hipSuccess) err = hipMemcpyAsync(got, d_stats, stats_bytes, hipMemcpyDeviceToHost, stream);
  if (err == hipSuccess) err = hipStreamSynchronize(stream);
  float ms = 0.f;
  if (err == hipSuccess) err = hipEventElapsedTime(&ms, e0, e1);
  HIP_TRY(err);
  if (stats) {
    uint64_t offered = 0;
    for (uint32_t i = 0; i < n_pass; ++i) offered += got[i * kStatsPerPass];
    for (uint32_t i = 0; i < n_pass; ++i) {
      stats[i].processed += got[i * kStatsPerPass + 0];
      stats[i].aligned += got[i * kStatsPerPass + 1];
      stats[i].steps += got[i * kStatsPerPass + 2];
      stats[i].candidates += got[i * kStatsPerPass + 3];
      stats[i].lookups += got[i * kStatsPerPass + 4];
      // one launch carries every pass: its time is shared out by the reads each pass was offered
      if (offered) stats[i].ms += ms * (float)((double)got[i * kStatsPerPass] / (double)offered);
    }
  }
  return MRG_OK;
}

// ----------------------------------------------------------------- tally
int mrg_tally_counts_len(uint32_t n_mirna, uint32_t n_samples, uint32_t n_pass, uint64_t* len) {
  if (!len) return fail(MRG_ERR_ARG, "mrg_tally_counts_len: null argument");
  *len = 2ull * n_mirna * n_samples + (uint64_t)(n_pass + 1) * n_samples + n_samples;
  return MRG_OK;
}

}  // extern "C"

namespace {
int tally_run_impl(mrg_ctx* ctx, const int8_t* d_pass_id, const int32_t* d_ref_id, const uint32_t* d_packed,
                  const uint32_t* d_quant, uint64_t n, uint32_t n_samples, uint32_t n_mirna,
                  uint32_t n_pass, int32_t canon_pass, int32_t isomir_pass, uint64_t* d_counts,
                  void* stream_) {
  if (!ctx || !d_counts) return fail(MRG_ERR_ARG, "mrg_tally_run: null argument");
  if (n && ((!d_packed && (!d_pass_id || !d_ref_id)) || !d_quant)) return fail(MRG_ERR_ARG, "mrg_tally_run: null buffers");
  if (n_samples == 0 || n_pass == 0 || n_pass > MRG_MAX_PASSES)
    return fail(MRG_ERR_ARG, "mrg_tally_run: bad n_samples/n_pass");
  HIP_TRY(hipSetDevice(ctx->device));
  if (n == 0) return MRG_OK;
  mrg::TallyParams p;
  p.packed = d_packed;
  p.pass_id = d_pass_id;
  p.ref_id = d_ref_id;
  p.quant = d_quant;
  p.n = n;
  p.n_samples = n_samples;
  p.n_mirna = n_mirna;
  p.n_pass = n_pass;
  p.canon_pass = canon_pass;
  p.isomir_pass = isomir_pass;
  p.counts = d_counts;
  p.export_stats = nullptr;
  p.export_out = nullptr;
  p.export_n_pass = 0;
  if (ctx->pending_export_out && ctx->pending_export_stream == (hipStream_t)stream_) {
    // "fused_step": the cascade in front left its per-pass counters to this launch
    p.export_stats = ctx->last_stats_dev;
    p.export_out = ctx->pending_export_out;
    p.export_n_pass = ctx->last_n_pass;
  }
  ctx->pending_export_out = nullptr;
  const bool in_ok = d_packed ? ((uintptr_t)d_packed % 16 == 0) : (((uintptr_t)d_pass_id % 4 == 0) && ((uintptr_t)d_ref_id % 16 == 0));
  p.vec4 = (n_samples == 1 && in_ok && ((uintptr_t)d_quant % 16 == 0)) ? 1u : 0u;
  uint64_t bins = 0;
  mrg_tally_counts_len(n_mirna, n_samples, n_pass, &bins);
  // LDS histogram: the category bins are replicated (kernels.hip: tally_kernel)
  const uint64_t lds = (bins + (uint64_t)(n_pass + 1) * n_samples * (mrg::kTallyCatReplicas - 1)) * 8;
  const bool lds_hist = lds <= (uint64_t)ctx->lds_budget;
  uint64_t want = ((p.vec4 ? (n + 3) / 4 : n) + mrg::kTallyThreads - 1) / mrg::kTallyThreads;
  uint32_t per_cu = lds_hist ? (lds * 2 <= 160 * 1024 ? 2u : 1u) : 2u;
  uint32_t grid = (uint32_t)std::min<uint64_t>(want, (uint64_t)ctx->n_cu * per_cu);
  HIP_TRY(mrg::launch_tally(p, lds_hist, grid, lds_hist ? (uint32_t)lds : 0u, (hipStream_t)stream_));
  uint32_t* last = ctx->last_tally_launch[MRG_TALLY_LAUNCH_COUNTS];  // (a launch that failed leaves the record alone)
  last[0] = (lds_hist ? MRG_TALLY_LDS_HIST : 0u) | (p.vec4 ? MRG_TALLY_VEC4 : 0u);
  last[1] = grid;
  last[2] = lds_hist ? (uint32_t)lds : 0u;
  return MRG_OK;
}
}  // namespace

extern "C" {

int mrg_tally_run(mrg_ctx* ctx, const int8_t* d_pass_id, const int32_t* d_ref_id, const uint32_t* d_quant, uint64_t n,
                  uint32_t n_samples, uint32_t n_mirna, uint32_t n_pass, int32_t canon_pass, int32_t isomir_pass, uint64_t* d_counts,
                  void* stream) {
  return tally_run_impl(ctx, d_pass_id, d_ref_id, nullptr, d_quant, n, n_samples, n_mirna, n_pass, canon_pass, isomir_pass, d_counts, stream);
}

int mrg_tally_run_packed(mrg_ctx* ctx, const uint32_t* d_packed, const uint32_t* d_quant, uint64_t n, uint32_t n_samples,
                         uint32_t n_mirna, uint32_t n_pass, int32_t canon_pass, int32_t isomir_pass, uint64_t* d_counts, void* stream) {
  if (n && !d_packed) return fail(MRG_ERR_ARG, "mrg_tally_run_packed: null buffers");
  // (the packed word's entry field saturates at 0x3FFFF: a larger library would be tallied into the wrong bin)
  if (n_mirna > 0x3FFFFu)
    return fail(MRG_ERR_ARG, "mrg_tally_run_packed: %u miRNA entries do not fit the packed word's 18-bit entry field (use mrg_tally_run)", n_mirna);
  return tally_run_impl(ctx, nullptr, nullptr, d_packed, d_quant, n, n_samples, n_mirna, n_pass, canon_pass, isomir_pass, d_counts, stream);
}

// ------------------------------------------------------------ multi-GPU (RCCL over xGMI)
#define RCCL_TRY(api, expr)                                                                         \
  do {                                                                                              \
    ncclResult_t r_ = (expr);                                                                       \
    if (r_ != ncclSuccess)                                                                          \
      return fail(MRG_ERR_HIP, "%s failed: %s", #expr, (api)->GetErrorString ? (api)->GetErrorString(r_) : "?"); \
  } while (0)

int mrg_comm_unique_id(void* id128) {
  if (!id128) return fail(MRG_ERR_ARG, "mrg_comm_unique_id: null argument");
  RcclApi* api = rccl_api();
  if (!api->handle) return fail(MRG_ERR_IO, "mrg_comm_unique_id: %s", api->error.c_str());
  ncclUniqueId id;
  RCCL_TRY(api, api->GetUniqueId(&id));
  static_assert(sizeof(id) == MRG_COMM_ID_BYTES, "ncclUniqueId size");
  std::memcpy(id128, &id, sizeof id);
  return MRG_OK;
}

int mrg_comm_init(mrg_ctx* ctx, const void* id128, int32_t rank, int32_t world) {
  if (!ctx || !id128) return fail(MRG_ERR_ARG, "mrg_comm_init: null argument");
  if (world < 1 || rank < 0 || rank >= world) return fail(MRG_ERR_ARG, "mrg_comm_init: rank %d of %d", rank, world);
  if (ctx->comm) return fail(MRG_ERR_ARG, "mrg_comm_init: the context already has a communicator");
  RcclApi* api = rccl_api();
  if (!api->handle) return fail(MRG_ERR_IO, "mrg_comm_init: %s", api->error.c_str());
  HIP_TRY(hipSetDevice(ctx->device));
  ncclUniqueId id;
  std::memcpy(&id, id128, sizeof id);
  RCCL_TRY(api, api->CommInitRank(&ctx->comm, world, id, rank));
  ctx->comm_rank = rank;
  ctx->comm_world = world;
  return MRG_OK;
}

int mrg_allreduce(mrg_ctx* ctx, uint64_t* d_buf, uint64_t n, void* stream) {
  if (!ctx || (n && !d_buf)) return fail(MRG_ERR_ARG, "mrg_allreduce: null argument");
  if (!ctx->comm) {
    if (ctx->comm_world == 1) return MRG_OK;  // one process, nothing to add
    return fail(MRG_ERR_ARG, "mrg_allreduce: call mrg_comm_init first");
  }
  if (n == 0) return MRG_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  RcclApi* api = rccl_api();
  RCCL_TRY(api, api->AllReduce(d_buf, d_buf, (size_t)n, ncclUint64, ncclSum, ctx->comm, (hipStream_t)stream));
  return MRG_OK;
}

int mrg_comm_destroy(mrg_ctx* ctx) {
  if (!ctx) return fail(MRG_ERR_ARG, "mrg_comm_destroy: null argument");
  if (ctx->comm) {
    RcclApi* api = rccl_api();
    ncclComm_t c = ctx->comm;
    ctx->comm = nullptr;
    ctx->comm_world = 1;
    RCCL_TRY(api, api->CommDestroy(c));
  }
  return MRG_OK;
}

// ------------------------------------------------------------ A-to-I position tally
int mrg_edit_counts_len(uint32_t n_bins, uint32_t n_samples, uint64_t* len) {
  if (!len) return fail(MRG_ERR_ARG, "mrg_edit_counts_len: null argument");
  *len = (uint64_t)n_bins * n_samples * (3ull + mrg::kEditPositions);
  return MRG_OK;
}

}  // extern "C"

namespace {
int edit_tally_impl(mrg_ctx* ctx, const uint64_t* d_reads, uint32_t words_per_read, const uint8_t* d_lens,
                       const uint64_t* d_nmask, const int8_t* d_pass_id, const int32_t* d_ref_id,
                       const int32_t* d_pos, const uint32_t* d_packed, const uint32_t* d_quant, const uint8_t* d_keep,
                       const uint32_t* d_remap, uint64_t n, uint32_t n_samples, uint32_t n_bins, int32_t lib,
                       int32_t canon_pass, int32_t isomir_pass, int32_t isomir_trim5, uint32_t flank5,
                       uint32_t flank3, uint32_t from_base, uint32_t to_base, uint64_t* d_counts, void* stream) {
  if (!ctx || !d_counts) return fail(MRG_ERR_ARG, "mrg_edit_tally_run: null argument");
  if (n && (!d_reads || !d_lens || (!d_packed && (!d_pass_id || !d_ref_id || !d_pos)) || !d_quant))
    return fail(MRG_ERR_ARG, "mrg_edit_tally_run: null buffers");
  if (lib < 0 || (size_t)lib >= ctx->libs.size()) return fail(MRG_ERR_ARG, "mrg_edit_tally_run: unknown library %d", lib);
  if (words_per_read != 1 && words_per_read != 2 && words_per_read != 4 && words_per_read != 8)
    return fail(MRG_ERR_ARG, "mrg_edit_tally_run: words_per_read must be 1, 2, 4 or 8");
  if (n_samples == 0 || n_bins == 0 || from_base > 3 || to_base > 3 || from_base == to_base)
    return fail(MRG_ERR_ARG, "mrg_edit_tally_run: bad n_samples / n_bins / bases");
  const DevLib& l = ctx->libs[lib];
  if (l.n_seg != l.n_ref || !l.simple)
    return fail(MRG_ERR_ARG, "mrg_edit_tally_run: the miRNA library must hold one N-free segment per entry");
  if (!d_remap && n_bins != l.n_ref)
    return fail(MRG_ERR_ARG, "mrg_edit_tally_run: n_bins %u != %u library entries (no remap given)", n_bins, l.n_ref);
  if (l.max_ref_len > mrg::kEditPositions + flank5 + flank3)
    return fail(MRG_ERR_ARG, "mrg_edit_tally_run: a library entry is longer than %u + flanks", mrg::kEditPositions);
  HIP_TRY(hipSetDevice(ctx->device));
  if (n == 0) return MRG_OK;
  mrg::EditParams p;
  p.reads = d_reads;
  p.lens = d_lens;
  p.nmask = d_nmask;
  p.words_per_read = words_per_read;
  p.packed = d_packed;
  p.pass_id = d_pass_id;
  p.ref_id = d_ref_id;
  p.pos = d_pos;
  p.quant = d_quant;
  p.keep = d_keep;
  p.remap = d_remap;
  p.n = n;
  p.n_samples = n_samples;
  p.n_bins = n_bins;
  p.canon_pass = canon_pass;
  p.isomir_pass = isomir_pass;
  p.isomir_trim5 = isomir_trim5;
  p.flank5 = flank5;
  p.flank3 = flank3;
  p.from_base = from_base;
  p.to_base = to_base;
  p.text = l.text;
  p.seg_start = l.seg_start;
  p.counts = d_counts;
  const bool in_ok = d_packed ? ((uintptr_t)d_packed % 16 == 0)
                              : (((uintptr_t)d_pass_id % 4 == 0) && ((uintptr_t)d_ref_id % 16 == 0) && ((uintptr_t)d_pos % 16 == 0));
  p.vec4 = (n_samples == 1 && words_per_read == 1 && ((uintptr_t)d_reads % 16 == 0) && ((uintptr_t)d_lens % 4 == 0) && in_ok &&
            ((uintptr_t)d_quant % 16 == 0))
               ? 1u
               : 0u;
  p.text_words = l.text_words;
  p.n_entries = l.n_ref;
  // LDS: the per-entry totals first (every kept read hits them), then -- if two workgroups per CU
  // still fit -- the library's text and entry starts, so that a read costs no gather
  const uint64_t hist_b = mrg::edit_hist_lds_bytes(n_bins, n_samples);
  const uint64_t lib_b = (uint64_t)l.text_words * 4 + (((uint64_t)l.n_ref + 4) & ~3ull) * 4;
  const uint64_t budget = (uint64_t)std::max<int64_t>(ctx->lds_budget, (int64_t)mrg::kEditHashLdsBytes) - mrg::kEditHashLdsBytes;
  const bool lds_hist = hist_b <= budget;
  const bool lds_lib = (lds_hist ? hist_b : 0) + lib_b + mrg::kEditHashLdsBytes <= std::min<uint64_t>(budget, 80 * 1024);
  const uint64_t lds = (lds_hist ? hist_b : 0) + (lds_lib ? lib_b : 0) + mrg::kEditHashLdsBytes;
  const uint64_t want = ((p.vec4 ? (n + 3) / 4 : n) + mrg::kEditThreads - 1) / mrg::kEditThreads;
  const uint32_t per_cu = lds * 2 <= 160 * 1024 ? 2u : 1u;
  const uint32_t grid = (uint32_t)std::min<uint64_t>(want, (uint64_t)ctx->n_cu * per_cu);
  HIP_TRY(mrg::launch_edit_tally(p, lds_hist, lds_lib, grid, (uint32_t)lds, (hipStream_t)stream));
  uint32_t* last = ctx->last_tally_launch[MRG_TALLY_LAUNCH_EDIT];
  last[0] = (lds_hist ? MRG_TALLY_LDS_HIST : 0u) | (lds_lib ? MRG_TALLY_LDS_LIB : 0u) | (p.vec4 ? MRG_TALLY_VEC4 : 0u);
  last[1] = grid;
  last[2] = (uint32_t)lds;
  return MRG_OK;
}
}  // namespace

extern "C" {

int mrg_edit_tally_run(mrg_ctx* ctx, const uint64_t* d_reads, uint32_t words_per_read, const uint8_t* d_lens, const uint64_t* d_nmask,
                       const int8_t* d_pass_id, const int32_t* d_ref_id, const int32_t* d_pos, const uint32_t* d_quant,
                       const uint8_t* d_keep, const uint32_t* d_remap, uint64_t n, uint32_t n_samples, uint32_t n_bins, int32_t lib,
                       int32_t canon_pass, int32_t isomir_pass, int32_t isomir_trim5, uint32_t flank5, uint32_t flank3,
                       uint32_t from_base, uint32_t to_base, uint64_t* d_counts, void* stream) {
  return edit_tally_impl(ctx, d_reads, words_per_read, d_lens, d_nmask, d_pass_id, d_ref_id, d_pos, nullptr, d_quant, d_keep, d_remap, n,
                         n_samples, n_bins, lib, canon_pass, isomir_pass, isomir_trim5, flank5, flank3, from_base, to_base, d_counts,
                         stream);
}

int mrg_edit_tally_run_packed(mrg_ctx* ctx, const uint64_t* d_reads, uint32_t words_per_read, const uint8_t* d_lens,
                              const uint64_t* d_nmask, const uint32_t* d_packed, const uint32_t* d_quant, const uint8_t* d_keep,
                              const uint32_t* d_remap, uint64_t n, uint32_t n_samples, uint32_t n_bins, int32_t lib, int32_t canon_pass,
                              int32_t isomir_pass, int32_t isomir_trim5, uint32_t flank5, uint32_t flank3, uint32_t from_base,
                              uint32_t to_base, uint64_t* d_counts, void* stream) {
  if (n && !d_packed) return fail(MRG_ERR_ARG, "mrg_edit_tally_run_packed: null buffers");
  // (entry and offset fields of the packed word saturate at 0x3FFFF / 0xFF)
  if (ctx && lib >= 0 && (size_t)lib < ctx->libs.size() && (ctx->libs[lib].n_ref > 0x3FFFFu || ctx->libs[lib].max_ref_len >= 0xFFu))
    return fail(MRG_ERR_ARG, "mrg_edit_tally_run_packed: the library (%u entries, longest %u) does not fit the packed word (use mrg_edit_tally_run)",
                ctx->libs[lib].n_ref, ctx->libs[lib].max_ref_len);
  return edit_tally_impl(ctx, d_reads, words_per_read, d_lens, d_nmask, nullptr, nullptr, nullptr, d_packed, d_quant, d_keep, d_remap, n,
                         n_samples, n_bins, lib, canon_pass, isomir_pass, isomir_trim5, flank5, flank3, from_base, to_base, d_counts,
                         stream);
}

int mrg_ctx_last_tally_launch(const mrg_ctx* ctx, int32_t which, uint32_t* out4) {
  if (!ctx || !out4) return fail(MRG_ERR_ARG, "mrg_ctx_last_tally_launch: null argument");
  if (which != MRG_TALLY_LAUNCH_COUNTS && which != MRG_TALLY_LAUNCH_EDIT)
    return fail(MRG_ERR_ARG, "mrg_ctx_last_tally_launch: which must be 0 (tally) or 1 (edit tally)");
  for (int i = 0; i < 4; ++i) out4[i] = ctx->last_tally_launch[which][i];
  return MRG_OK;
}

// ------------------------------------------------------------ count best
namespace {

int fill_count_params(mrg_ctx* ctx, const char* who, const uint64_t* d_reads, uint32_t words_per_read,
                      const uint8_t* d_lens, const uint64_t* d_nmask, uint64_t n, int32_t lib, int32_t seed_len,
                      int32_t max_mm_seed, int32_t max_mm_total, mrg::CountParams* p, uint32_t* grid,
                      uint32_t* lds_bytes) {
  if (!ctx) return fail(MRG_ERR_ARG, "%s: null argument", who);
  if (n && (!d_reads || !d_lens)) return fail(MRG_ERR_ARG, "%s: null buffers", who);
  if (lib < 0 || (size_t)lib >= ctx->libs.size()) return fail(MRG_ERR_ARG, "%s: unknown library %d", who, lib);
  if (words_per_read != 1 && words_per_read != 2 && words_per_read != 4 && words_per_read != 8)
    return fail(MRG_ERR_ARG, "%s: words_per_read must be 1, 2, 4 or 8", who);
  if (max_mm_seed < 0 || max_mm_seed > 2 || max_mm_total < max_mm_seed || seed_len < 1)
    return fail(MRG_ERR_ARG, "%s: invalid policy", who);
  if (n >= 0x7fffffffull) return fail(MRG_ERR_ARG, "%s: too many reads for one call", who);
  const DevLib& l = ctx->libs[lib];
  const uint64_t lds = (uint64_t)l.nsup * 16;
  if (lds > 160 * 1024) return fail(MRG_ERR_ARG, "%s: library too large for one call (split it)", who);
  std::memset(p, 0, sizeof(*p));
  fill_lib(*p, l);
  p->ctx = l.ctx;
  if (!ctx->use_ftab) p->tabs.k[0] = 0u;
  p->nsup = l.nsup;
  p->reads = d_reads;
  p->lens = d_lens;
  p->nmask = d_nmask;
  p->n_reads = n;
  p->seed_len = seed_len;
  p->max_mm_seed = max_mm_seed;
  p->max_mm_total = max_mm_total;
  p->wstop = (uint32_t)ctx->wstop;
  p->max_rows = 4096u;
  const uint64_t want = (n + mrg::kCountThreads - 1) / mrg::kCountThreads;
  const uint32_t per_cu = lds ? (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(8, (160 * 1024) / lds)) : 8u;
  *grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(want, (uint64_t)ctx->n_cu * per_cu));
  *lds_bytes = (uint32_t)lds;
  return MRG_OK;
}

}  // namespace

int mrg_count_best(mrg_ctx* ctx, const uint64_t* d_reads, uint32_t words_per_read, const uint8_t* d_lens,
                   const uint64_t* d_nmask, uint64_t n, int32_t lib, int32_t seed_len, int32_t max_mm_seed,
                   int32_t max_mm_total, uint8_t* d_best_mm, uint8_t* d_count, void* stream) {
  mrg::CountParams p;
  uint32_t grid = 0, lds = 0;
  int rc = fill_count_params(ctx, "mrg_count_best", d_reads, words_per_read, d_lens, d_nmask, n, lib, seed_len,
                             max_mm_seed, max_mm_total, &p, &grid, &lds);
  if (rc != MRG_OK) return rc;
  if (n && (!d_best_mm || !d_count)) return fail(MRG_ERR_ARG, "mrg_count_best: null buffers");
  HIP_TRY(hipSetDevice(ctx->device));
  if (n == 0) return MRG_OK;
  p.best_mm = d_best_mm;
  p.count = d_count;
  // one-mismatch run on one-word reads without N: the largest jump table's K-mers and their variants first (kernels.hip:
  // count_variants_kernel); the pigeonhole kernel then takes what that left (reads shorter than a usable table, longer than
  // the seed) -- nothing, for the 18..21-nt reads the -ai path submits
  if (ctx->count_variants && words_per_read == 1 && !d_nmask && max_mm_seed == 1 && ctx->use_ftab) {
    const uint64_t want = (n + 7) / 8;
    const uint32_t vgrid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(want, (uint64_t)ctx->n_cu * 32u));
    HIP_TRY(mrg::launch_count_variants(p, vgrid, (hipStream_t)stream));
    p.only_todo = 1u;
    if (ctx->count_variants == 2) return MRG_OK;  // (tests: the reads it left keep best_mm 254, their count is not written)
  }
  HIP_TRY(mrg::launch_count(p, words_per_read, grid, lds, (hipStream_t)stream));
  return MRG_OK;
}

int mrg_list_best_count(mrg_ctx* ctx, const uint64_t* d_reads, uint32_t words_per_read, const uint8_t* d_lens,
                        const uint64_t* d_nmask, uint64_t n, int32_t lib, int32_t seed_len, int32_t max_mm_seed,
                        int32_t max_mm_total, uint8_t* d_best_mm, uint64_t* d_offsets, uint64_t* total,
                        void* stream) {
  mrg::CountParams p;
  uint32_t grid = 0, lds = 0;
  int rc = fill_count_params(ctx, "mrg_list_best_count", d_reads, words_per_read, d_lens, d_nmask, n, lib,
                             seed_len, max_mm_seed, max_mm_total, &p, &grid, &lds);
  if (rc != MRG_OK) return rc;
  if (!d_offsets || !total || (n && !d_best_mm)) return fail(MRG_ERR_ARG, "mrg_list_best_count: null buffers");
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  // per-read stratum sizes live in the context's scratch buffer (grown, never shrunk: repeated
  // calls do not allocate)
  const uint64_t need_bytes = (n + 1) * sizeof(uint32_t);
  if (ctx->scratch_bytes < need_bytes) {
    HIP_TRY(hipStreamSynchronize(st));
    (void)hipFree(ctx->scratch);
    ctx->scratch = nullptr;
    ctx->scratch_bytes = 0;
    HIP_TRY(hipMalloc(&ctx->scratch, need_bytes));
    ctx->scratch_bytes = need_bytes;
  }
  uint32_t* cnt = (uint32_t*)ctx->scratch;
  hipError_t e = hipMemsetAsync(cnt, 0, (n + 1) * sizeof(uint32_t), st);
  if (e == hipSuccess && n) {
    p.best_mm = d_best_mm;
    p.count32 = cnt;
    p.max_rows = 1u << 20;
    e = mrg::launch_count(p, words_per_read, grid, lds, st);
  }
  if (e == hipSuccess) e = mrg::exclusive_sum_u32_u64(cnt, d_offsets, n + 1, st);
  if (e == hipSuccess) e = hipMemcpyAsync(total, d_offsets + n, sizeof(uint64_t), hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  HIP_TRY(e);
  return MRG_OK;
}

int mrg_list_best_fill(mrg_ctx* ctx, const uint64_t* d_reads, uint32_t words_per_read, const uint8_t* d_lens,
                       const uint64_t* d_nmask, uint64_t n, int32_t lib, int32_t seed_len, int32_t max_mm_seed,
                       int32_t max_mm_total, const uint8_t* d_best_mm, const uint64_t* d_offsets, uint64_t cap,
                       int32_t* d_ref, int32_t* d_pos, void* stream) {
  mrg::CountParams p;
  uint32_t grid = 0, lds = 0;
  int rc = fill_count_params(ctx, "mrg_list_best_fill", d_reads, words_per_read, d_lens, d_nmask, n, lib,
                             seed_len, max_mm_seed, max_mm_total, &p, &grid, &lds);
  if (rc != MRG_OK) return rc;
  if (n && (!d_best_mm || !d_offsets)) return fail(MRG_ERR_ARG, "mrg_list_best_fill: null buffers");
  if (cap && (!d_ref || !d_pos)) return fail(MRG_ERR_ARG, "mrg_list_best_fill: null output buffers");
  HIP_TRY(hipSetDevice(ctx->device));
  if (n == 0 || cap == 0) return MRG_OK;
  p.best_mm = const_cast<uint8_t*>(d_best_mm);
  p.offsets = d_offsets;
  p.out_ref = d_ref;
  p.out_pos = d_pos;
  p.out_cap = cap;
  p.max_rows = 1u << 20;
  HIP_TRY(mrg::launch_count(p, words_per_read, grid, lds, (hipStream_t)stream));
  return MRG_OK;
}

namespace {

int fill_valid_params(mrg_ctx* ctx, const char* who, const uint64_t* d_reads, uint32_t words_per_read, const uint8_t* d_lens,
                      const uint64_t* d_nmask, uint64_t n, int32_t lib, int32_t strands, int32_t seed_len, int32_t max_mm_seed,
                      int32_t max_mm_total, mrg::ValidParams* p, uint32_t* grid, uint32_t* lds_bytes) {
  std::memset(p, 0, sizeof(*p));
  int rc = fill_count_params(ctx, who, d_reads, words_per_read, d_lens, d_nmask, n, lib, seed_len, max_mm_seed, max_mm_total,
                             &p->c, grid, lds_bytes);
  if (rc != MRG_OK) return rc;
  if (strands != 1 && strands != 2) return fail(MRG_ERR_ARG, "%s: strands must be 1 (forward) or 2 (both)", who);
  if (max_mm_total > 3) return fail(MRG_ERR_ARG, "%s: at most 3 mismatches", who);
  p->strands = (uint32_t)strands;
  p->c.max_rows = 0xFFFFFFFFu;  // (valid_kernel walks every row of a seed interval)
  return MRG_OK;
}

}  // namespace

int mrg_list_valid_count(mrg_ctx* ctx, const uint64_t* d_reads, uint32_t words_per_read, const uint8_t* d_lens,
                         const uint64_t* d_nmask, uint64_t n, int32_t lib, int32_t strands, int32_t seed_len, int32_t max_mm_seed,
                         int32_t max_mm_total, uint32_t* d_counts, void* stream) {
  mrg::ValidParams p;
  uint32_t grid = 0, lds = 0;
  int rc = fill_valid_params(ctx, "mrg_list_valid_count", d_reads, words_per_read, d_lens, d_nmask, n, lib, strands, seed_len,
                             max_mm_seed, max_mm_total, &p, &grid, &lds);
  if (rc != MRG_OK) return rc;
  if (n && !d_counts) return fail(MRG_ERR_ARG, "mrg_list_valid_count: null buffers");
  HIP_TRY(hipSetDevice(ctx->device));
  if (n == 0) return MRG_OK;
  p.counts = d_counts;
  HIP_TRY(mrg::launch_valid(p, false, words_per_read, grid, lds, (hipStream_t)stream));
  return MRG_OK;
}

int mrg_list_valid_fill(mrg_ctx* ctx, const uint64_t* d_reads, uint32_t words_per_read, const uint8_t* d_lens,
                        const uint64_t* d_nmask, uint64_t n, int32_t lib, int32_t strands, int32_t stratum_mode, int32_t seed_len,
                        int32_t max_mm_seed, int32_t max_mm_total, const uint8_t* d_best_mm, const uint64_t* d_offsets, uint64_t cap,
                        int32_t* d_ref, int32_t* d_pos, uint8_t* d_strand, uint8_t* d_mm, void* stream) {
  mrg::ValidParams p;
  uint32_t grid = 0, lds = 0;
  int rc = fill_valid_params(ctx, "mrg_list_valid_fill", d_reads, words_per_read, d_lens, d_nmask, n, lib, strands, seed_len,
                             max_mm_seed, max_mm_total, &p, &grid, &lds);
  if (rc != MRG_OK) return rc;
  if (stratum_mode != MRG_STRATUM_BEST && stratum_mode != MRG_STRATUM_ALL)
    return fail(MRG_ERR_ARG, "mrg_list_valid_fill: stratum_mode must be MRG_STRATUM_BEST or MRG_STRATUM_ALL");
  if (n && (!d_best_mm || !d_offsets)) return fail(MRG_ERR_ARG, "mrg_list_valid_fill: null buffers");
  if (cap && (!d_ref || !d_pos || !d_strand || !d_mm)) return fail(MRG_ERR_ARG, "mrg_list_valid_fill: null output buffers");
  HIP_TRY(hipSetDevice(ctx->device));
  if (n == 0 || cap == 0) return MRG_OK;
  p.all = stratum_mode == MRG_STRATUM_ALL ? 1u : 0u;
  p.c.best_mm = const_cast<uint8_t*>(d_best_mm);
  p.c.offsets = d_offsets;
  p.c.out_ref = d_ref;
  p.c.out_pos = d_pos;
  p.c.out_cap = cap;
  p.out_strand = d_strand;
  p.out_mm = d_mm;
  HIP_TRY(mrg::launch_valid(p, true, words_per_read, grid, lds, (hipStream_t)stream));
  return MRG_OK;
}

namespace {

// the checks and the parameter block the two sweeps of the ragged listing share
int fill_long_valid_params(mrg_ctx* ctx, const char* who, const uint64_t* d_words, const uint64_t* d_nmask, const uint64_t* d_word_off,
                           const uint32_t* d_lens, uint64_t n, int32_t lib, int32_t strands, int32_t seed_len, int32_t max_mm_seed,
                           int32_t max_mm_total, mrg::LongValidParams* p, uint32_t* grid) {
  if (!ctx) return fail(MRG_ERR_ARG, "%s: null argument", who);
  if (n && (!d_words || !d_word_off || !d_lens)) return fail(MRG_ERR_ARG, "%s: null buffers", who);
  if (lib < 0 || (size_t)lib >= ctx->libs.size()) return fail(MRG_ERR_ARG, "%s: unknown library %d", who, lib);
  if (strands != 1 && strands != 2) return fail(MRG_ERR_ARG, "%s: strands must be 1 (forward) or 2 (both)", who);
  if (max_mm_seed < 0 || max_mm_seed > 2 || max_mm_total < max_mm_seed || seed_len < 1) return fail(MRG_ERR_ARG, "%s: invalid policy", who);
  if (max_mm_total > 3) return fail(MRG_ERR_ARG, "%s: at most 3 mismatches", who);
  if (n >= 0x7fffffffull) return fail(MRG_ERR_ARG, "%s: too many reads for one call", who);
  std::memset(p, 0, sizeof(*p));
  fill_long_lib(p->lib, *ctx, ctx->libs[lib]);
  p->lib.seed_len = seed_len;
  p->lib.max_mm_seed = max_mm_seed;
  p->lib.max_mm_total = max_mm_total;
  p->words = d_words;
  p->nmask = d_nmask;
  p->word_off = d_word_off;
  p->lens = d_lens;
  p->n = (uint32_t)n;
  p->wstop = (uint32_t)ctx->wstop;
  p->strands = (uint32_t)strands;
  // one wave per read, four per workgroup; more reads than resident waves: the kernel strides
  *grid = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + 3) / 4, (uint64_t)ctx->n_cu * 8u));
  return MRG_OK;
}

}  // namespace

int mrg_list_valid_long_count(mrg_ctx* ctx, const uint64_t* d_words, const uint64_t* d_nmask, const uint64_t* d_word_off,
                              const uint32_t* d_lens, uint64_t n, int32_t lib, int32_t strands, int32_t seed_len, int32_t max_mm_seed,
                              int32_t max_mm_total, uint32_t* d_counts, void* stream) {
  mrg::LongValidParams p;
  uint32_t grid = 0;
  int rc = fill_long_valid_params(ctx, "mrg_list_valid_long_count", d_words, d_nmask, d_word_off, d_lens, n, lib, strands, seed_len,
                                  max_mm_seed, max_mm_total, &p, &grid);
  if (rc != MRG_OK) return rc;
  if (n && !d_counts) return fail(MRG_ERR_ARG, "mrg_list_valid_long_count: null buffers");
  HIP_TRY(hipSetDevice(ctx->device));
  if (n == 0) return MRG_OK;
  p.counts = d_counts;
  HIP_TRY(mrg::launch_long_valid(p, false, grid, (hipStream_t)stream));
  return MRG_OK;
}

int mrg_list_valid_long_fill(mrg_ctx* ctx, const uint64_t* d_words, const uint64_t* d_nmask, const uint64_t* d_word_off,
                             const uint32_t* d_lens, uint64_t n, int32_t lib, int32_t strands, int32_t seed_len, int32_t max_mm_seed,
                             int32_t max_mm_total, int32_t stratum_mode, const uint8_t* d_best_mm, const uint64_t* d_offsets,
                             uint64_t cap, int32_t* d_ref, int32_t* d_pos, uint8_t* d_strand, uint8_t* d_mm, void* stream) {
  mrg::LongValidParams p;
  uint32_t grid = 0;
  int rc = fill_long_valid_params(ctx, "mrg_list_valid_long_fill", d_words, d_nmask, d_word_off, d_lens, n, lib, strands, seed_len,
                                  max_mm_seed, max_mm_total, &p, &grid);
  if (rc != MRG_OK) return rc;
  if (stratum_mode != MRG_STRATUM_BEST && stratum_mode != MRG_STRATUM_ALL)
    return fail(MRG_ERR_ARG, "mrg_list_valid_long_fill: stratum_mode must be MRG_STRATUM_BEST or MRG_STRATUM_ALL");
  if (n && (!d_best_mm || !d_offsets)) return fail(MRG_ERR_ARG, "mrg_list_valid_long_fill: null buffers");
  if (cap && (!d_ref || !d_pos || !d_strand || !d_mm)) return fail(MRG_ERR_ARG, "mrg_list_valid_long_fill: null output buffers");
  HIP_TRY(hipSetDevice(ctx->device));
  if (n == 0 || cap == 0) return MRG_OK;
  p.all = stratum_mode == MRG_STRATUM_ALL ? 1u : 0u;
  p.best_mm = d_best_mm;
  p.offsets = d_offsets;
  p.cap = cap;
  p.out_ref = d_ref;
  p.out_pos = d_pos;
  p.out_strand = d_strand;
  p.out_mm = d_mm;
  HIP_TRY(mrg::launch_long_valid(p, true, grid, (hipStream_t)stream));
  return MRG_OK;
}

int mrg_write_bowtie(const char* path, int32_t sam, const char* cmdline, const mrg_index* const* parts, uint32_t n_parts,
                     uint64_t n_reads, const char* names, const uint64_t* names_off, const char* seqs, const uint64_t* seqs_off,
                     const uint64_t* offsets, const int32_t* entry, const int32_t* offset, const uint8_t* strand, const uint8_t* mm,
                     const uint8_t* suppressed, int32_t m, uint64_t* summary) {
  if ((n_parts && !parts) || (n_reads && (!names || !names_off || !seqs || !seqs_off || !offsets)) || !summary)
    return fail(MRG_ERR_ARG, "mrg_write_bowtie: null argument");
  if (n_reads && offsets[n_reads] && (!entry || !offset || !strand || !mm))
    return fail(MRG_ERR_ARG, "mrg_write_bowtie: null alignment arrays");
  std::vector<const mrg::FmIndex*> ix(n_parts);
  for (uint32_t i = 0; i < n_parts; ++i) {
    if (!parts[i]) return fail(MRG_ERR_ARG, "mrg_write_bowtie: null index");
    ix[i] = &parts[i]->ix;
  }
  try {
    mrg::write_bowtie(path, sam != 0, cmdline, ix, n_reads, names, names_off, seqs, seqs_off, offsets, entry, offset, strand, mm,
                      suppressed, m, summary);
    return MRG_OK;
  } catch (const std::exception& e) {
    return fail(MRG_ERR_IO, "mrg_write_bowtie: %s", e.what());
  }
}

// ------------------------------------------------- predict mode: clusters
namespace {
int cluster_check(const char* who, const mrg_ctx* ctx, uint64_t rows, uint32_t n_entries, uint32_t pos_bits) {
  if (!ctx) return fail(MRG_ERR_ARG, "%s: null argument", who);
  if (rows >= 0xffffffffull) return fail(MRG_ERR_ARG, "%s: %llu alignment rows; the limit is 2^32 - 2", who, (unsigned long long)rows);
  if (pos_bits < 1 || pos_bits > 31) return fail(MRG_ERR_ARG, "%s: positions must be below 2^31 (pos_bits %u)", who, pos_bits);
  if ((uint64_t)n_entries + 1 > (1ull << (63u - pos_bits)) - 1)
    return fail(MRG_ERR_ARG, "%s: %u entries do not fit the %u entry bits of the key", who, n_entries, 63u - pos_bits);
  return MRG_OK;
}
size_t cluster_tmp_bytes(uint64_t rows) { return std::max(mrg::prims::radix_temp_bytes(rows + 1), mrg::prims::scan_temp_bytes(rows + 1)); }
}  // namespace

int mrg_cluster_workspace_bytes(uint64_t rows, uint64_t* tmp_bytes, uint64_t* work_bytes) {
  if (!tmp_bytes || !work_bytes) return fail(MRG_ERR_ARG, "mrg_cluster_workspace_bytes: null argument");
  *tmp_bytes = cluster_tmp_bytes(rows);
  *work_bytes = mrg::cluster_work_bytes(rows);
  return MRG_OK;
}

int mrg_cluster_keys(mrg_ctx* ctx, const uint64_t* d_offsets, uint64_t n_reads, const int32_t* d_ref, const int32_t* d_pos,
                     const uint8_t* d_strand, uint64_t rows, uint64_t row_base, uint64_t total_rows, uint32_t entry_base,
                     uint32_t n_entries, uint32_t pos_bits, int32_t order, const uint8_t* d_entry_keep, uint64_t* d_keys,
                     uint32_t* d_vals, uint32_t* d_owner, void* stream) {
  int rc = cluster_check("mrg_cluster_keys", ctx, total_rows, n_entries, pos_bits);
  if (rc != MRG_OK) return rc;
  if (order != MRG_CLUSTER_ORDER && order != MRG_SAM_ORDER) return fail(MRG_ERR_ARG, "mrg_cluster_keys: unknown key order %d", order);
  if (row_base + rows > total_rows || n_reads >= 0xffffffffull) return fail(MRG_ERR_ARG, "mrg_cluster_keys: rows or reads out of range");
  if (rows && (!n_reads || !d_offsets || !d_ref || !d_pos || !d_strand || !d_keys || !d_vals || !d_owner))
    return fail(MRG_ERR_ARG, "mrg_cluster_keys: null buffers");
  HIP_TRY(hipSetDevice(ctx->device));
  mrg::ClusterKeysArgs a{d_offsets, n_reads, d_ref, d_pos, d_strand, (uint32_t)rows, entry_base, (uint32_t)row_base, n_entries, pos_bits,
                         order, d_entry_keep, d_keys, d_vals, d_owner};
  HIP_TRY(mrg::cluster_keys_launch(a, (hipStream_t)stream));
  return MRG_OK;
}

int mrg_cluster_sort(mrg_ctx* ctx, uint64_t* d_keys0, uint64_t* d_keys1, uint32_t* d_vals0, uint32_t* d_vals1, uint64_t rows,
                     uint32_t bits, void* d_tmp, uint64_t tmp_bytes, int32_t* in_second, void* stream) {
  if (!ctx || !in_second) return fail(MRG_ERR_ARG, "mrg_cluster_sort: null argument");
  if (rows >= 0xffffffffull) return fail(MRG_ERR_ARG, "mrg_cluster_sort: %llu alignment rows; the limit is 2^32 - 2", (unsigned long long)rows);
  if (bits > 64) return fail(MRG_ERR_ARG, "mrg_cluster_sort: %u key bits", bits);
  if (rows && (!d_keys0 || !d_keys1 || !d_vals0 || !d_vals1 || !d_tmp)) return fail(MRG_ERR_ARG, "mrg_cluster_sort: null buffers");
  if (tmp_bytes < cluster_tmp_bytes(rows)) return fail(MRG_ERR_ARG, "mrg_cluster_sort: scratch smaller than mrg_cluster_workspace_bytes");
  HIP_TRY(hipSetDevice(ctx->device));
  bool second = false;
  HIP_TRY(mrg::prims::radix_sort_pairs_u64(d_keys0, d_keys1, d_vals0, d_vals1, (uint32_t)rows, bits, d_tmp, (hipStream_t)stream, &second));
  *in_second = second ? 1 : 0;
  return MRG_OK;
}

int mrg_cluster_scan(mrg_ctx* ctx, const uint64_t* d_keys, const uint32_t* d_vals, uint64_t rows, const uint32_t* d_owner,
                     const uint8_t* d_lens, uint32_t n_entries, uint32_t pos_bits, int32_t threshold, void* d_work, uint64_t work_bytes,
                     void* d_tmp, uint64_t tmp_bytes, uint32_t* d_member, uint64_t* n_valid, uint64_t* n_clusters, void* stream) {
  int rc = cluster_check("mrg_cluster_scan", ctx, rows, n_entries, pos_bits);
  if (rc != MRG_OK) return rc;
  if (!n_valid || !n_clusters) return fail(MRG_ERR_ARG, "mrg_cluster_scan: null argument");
  if (threshold < 1) return fail(MRG_ERR_ARG, "mrg_cluster_scan: the overlap threshold must be at least 1 (got %d)", threshold);
  *n_valid = *n_clusters = 0;
  if (rows == 0) return MRG_OK;
  if (!d_keys || !d_vals || !d_owner || !d_lens || !d_work || !d_tmp || !d_member) return fail(MRG_ERR_ARG, "mrg_cluster_scan: null buffers");
  if (work_bytes < mrg::cluster_work_bytes(rows) || tmp_bytes < cluster_tmp_bytes(rows))
    return fail(MRG_ERR_ARG, "mrg_cluster_scan: buffers smaller than mrg_cluster_workspace_bytes");
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  const mrg::ClusterWork w = mrg::cluster_work(d_work, rows);
  HIP_TRY(mrg::cluster_rows_launch(d_keys, d_vals, (uint32_t)rows, d_owner, d_lens, n_entries, pos_bits, w, d_member, st));
  HIP_TRY(mrg::prims::segmented_inclusive_max_u32(w.end, w.lhead, w.runmax, rows, d_tmp, st));
  HIP_TRY(mrg::cluster_heads_launch(d_keys, (uint32_t)rows, n_entries, pos_bits, threshold, w, st));
  HIP_TRY(mrg::prims::inclusive_sum_u32(w.chead, w.cinc, rows, d_tmp, st));
  uint32_t last = 0;
  HIP_TRY(hipMemcpyAsync(n_valid, w.n_valid, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(&last, w.cinc + (rows - 1), sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  *n_clusters = last;
  return MRG_OK;
}

int mrg_cluster_bounds(mrg_ctx* ctx, const uint64_t* d_keys, uint64_t rows, uint64_t n_valid, uint64_t n_clusters, uint32_t pos_bits,
                       void* d_work, uint64_t work_bytes, void* d_tmp, uint64_t tmp_bytes, uint32_t* d_entry, uint8_t* d_strand,
                       uint32_t* d_start, uint32_t* d_end, uint32_t* d_member_off, uint32_t* d_len, uint64_t* d_seq_off,
                       uint64_t* total_len, void* stream) {
  int rc = cluster_check("mrg_cluster_bounds", ctx, rows, 0, pos_bits);
  if (rc != MRG_OK) return rc;
  if (!total_len) return fail(MRG_ERR_ARG, "mrg_cluster_bounds: null argument");
  if (n_valid > rows || n_clusters > n_valid) return fail(MRG_ERR_ARG, "mrg_cluster_bounds: more clusters than rows");
  if (!d_member_off || !d_len || !d_seq_off || (rows && (!d_keys || !d_work || !d_tmp)) ||
      (n_clusters && (!d_entry || !d_strand || !d_start || !d_end)))
    return fail(MRG_ERR_ARG, "mrg_cluster_bounds: null buffers");
  if (work_bytes < mrg::cluster_work_bytes(rows) || tmp_bytes < cluster_tmp_bytes(rows))
    return fail(MRG_ERR_ARG, "mrg_cluster_bounds: buffers smaller than mrg_cluster_workspace_bytes");
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  const mrg::ClusterWork w = mrg::cluster_work(d_work, rows);
  const mrg::ClusterTable c{(uint32_t)n_clusters, (uint32_t)n_valid, d_entry, d_strand, d_start, d_end, d_member_off, d_len};
  HIP_TRY(mrg::cluster_bounds_launch(d_keys, pos_bits, w, c, st));
  HIP_TRY(mrg::prims::exclusive_sum_u32_to_u64(d_len, d_seq_off, n_clusters + 1, d_tmp, st));
  HIP_TRY(hipMemcpyAsync(total_len, d_seq_off + n_clusters, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return MRG_OK;
}

int mrg_cluster_assemble(mrg_ctx* ctx, const uint64_t* d_keys, uint64_t rows, uint64_t n_valid, uint64_t n_clusters, uint32_t pos_bits,
                         void* d_work, uint64_t work_bytes, const uint32_t* d_member, const uint64_t* d_reads, uint32_t words_per_read,
                         const uint8_t* d_lens, const uint64_t* d_nmask, uint64_t n_reads, const uint32_t* d_counts,
                         const uint32_t* d_start, const uint64_t* d_seq_off, char* d_seq, uint64_t* d_sum, void* stream) {
  int rc = cluster_check("mrg_cluster_assemble", ctx, rows, 0, pos_bits);
  if (rc != MRG_OK) return rc;
  if (n_valid > rows || n_clusters > n_valid) return fail(MRG_ERR_ARG, "mrg_cluster_assemble: more clusters than rows");
  if (n_clusters == 0) return MRG_OK;
  if (!d_keys || !d_work || !d_member || !d_reads || !d_lens || !d_counts || !d_start || !d_seq_off || !d_seq || !d_sum)
    return fail(MRG_ERR_ARG, "mrg_cluster_assemble: null buffers");
  if (work_bytes < mrg::cluster_work_bytes(rows)) return fail(MRG_ERR_ARG, "mrg_cluster_assemble: buffer smaller than mrg_cluster_workspace_bytes");
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  const mrg::ClusterWork w = mrg::cluster_work(d_work, rows);
  const mrg::ClusterTable c{(uint32_t)n_clusters, (uint32_t)n_valid, nullptr, nullptr, const_cast<uint32_t*>(d_start), nullptr, nullptr, nullptr};
  HIP_TRY(hipMemsetAsync(d_sum, 0, n_clusters * sizeof(uint64_t), st));
  const mrg::ClusterAssembleArgs a{d_keys, pos_bits, d_member, d_reads, words_per_read, d_nmask, d_lens, n_reads, d_counts, d_seq_off, d_seq,
                                   reinterpret_cast<unsigned long long*>(d_sum)};
  HIP_TRY(mrg::cluster_assemble_launch(a, w, c, st));
  return MRG_OK;
}

int mrg_cluster_sorted_rows(mrg_ctx* ctx, const uint64_t* d_keys, const uint32_t* d_vals, uint64_t rows, uint32_t pos_bits, int32_t order,
                            const uint32_t* d_owner, const uint8_t* d_mm, uint32_t* d_read, int32_t* d_entry, int32_t* d_pos,
                            uint8_t* d_strand, uint8_t* d_mm_out, void* stream) {
  int rc = cluster_check("mrg_cluster_sorted_rows", ctx, rows, 0, pos_bits);
  if (rc != MRG_OK) return rc;
  if (order != MRG_CLUSTER_ORDER && order != MRG_SAM_ORDER) return fail(MRG_ERR_ARG, "mrg_cluster_sorted_rows: unknown key order %d", order);
  if (rows && (!d_keys || !d_vals || !d_owner || !d_mm || !d_read || !d_entry || !d_pos || !d_strand || !d_mm_out))
    return fail(MRG_ERR_ARG, "mrg_cluster_sorted_rows: null buffers");
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(mrg::cluster_gather_launch(d_keys, d_vals, (uint32_t)rows, pos_bits, order, d_owner, d_mm, d_read, d_entry, d_pos, d_strand,
                                     d_mm_out, (hipStream_t)stream));
  return MRG_OK;
}

// ------------------------------------------------- the primitives, directly (tests and diagnostics)
int mrg_prims_temp_bytes(int32_t kind, uint64_t n, uint64_t* bytes) {
  if (!bytes) return fail(MRG_ERR_ARG, "mrg_prims_temp_bytes: null argument");
  if (kind != MRG_PRIMS_SCAN && kind != MRG_PRIMS_SORT) return fail(MRG_ERR_ARG, "mrg_prims_temp_bytes: unknown kind %d", kind);
  *bytes = kind == MRG_PRIMS_SCAN ? mrg::prims::scan_temp_bytes(n) : mrg::prims::radix_temp_bytes(n);
  return MRG_OK;
}

int mrg_prims_scan(mrg_ctx* ctx, int32_t kind, const uint32_t* d_in, void* d_out, uint64_t n, void* d_tmp, uint64_t tmp_bytes,
                   void* stream) {
  if (kind != MRG_SCAN_EXCLUSIVE_U32 && kind != MRG_SCAN_INCLUSIVE_U32 && kind != MRG_SCAN_EXCLUSIVE_U64)
    return fail(MRG_ERR_ARG, "mrg_prims_scan: unknown kind %d", kind);
  if (!ctx) return fail(MRG_ERR_ARG, "mrg_prims_scan: null argument");
  if (n && (!d_in || !d_out || !d_tmp)) return fail(MRG_ERR_ARG, "mrg_prims_scan: null buffers");
  if (tmp_bytes < mrg::prims::scan_temp_bytes(n)) return fail(MRG_ERR_ARG, "mrg_prims_scan: scratch smaller than mrg_prims_temp_bytes");
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  if (kind == MRG_SCAN_EXCLUSIVE_U32)
    HIP_TRY(mrg::prims::exclusive_sum_u32(d_in, (uint32_t*)d_out, n, d_tmp, st));
  else if (kind == MRG_SCAN_INCLUSIVE_U32)
    HIP_TRY(mrg::prims::inclusive_sum_u32(d_in, (uint32_t*)d_out, n, d_tmp, st));
  else
    HIP_TRY(mrg::prims::exclusive_sum_u32_to_u64(d_in, (uint64_t*)d_out, n, d_tmp, st));
  return MRG_OK;
}

int mrg_prims_segmented_max(mrg_ctx* ctx, const uint32_t* d_in, const uint8_t* d_head, uint32_t* d_out, uint64_t n, void* d_tmp,
                            uint64_t tmp_bytes, void* stream) {
  if (!ctx) return fail(MRG_ERR_ARG, "mrg_prims_segmented_max: null argument");
  if (n && (!d_in || !d_head || !d_out || !d_tmp)) return fail(MRG_ERR_ARG, "mrg_prims_segmented_max: null buffers");
  if (tmp_bytes < mrg::prims::scan_temp_bytes(n))
    return fail(MRG_ERR_ARG, "mrg_prims_segmented_max: scratch smaller than mrg_prims_temp_bytes");
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(mrg::prims::segmented_inclusive_max_u32(d_in, d_head, d_out, n, d_tmp, (hipStream_t)stream));
  return MRG_OK;
}

int mrg_prims_radix_sort(mrg_ctx* ctx, uint32_t key_bytes, void* d_keys0, void* d_keys1, uint32_t* d_vals0, uint32_t* d_vals1,
                         uint64_t n, uint32_t bits, void* d_tmp, uint64_t tmp_bytes, int32_t* in_second, void* stream) {
  if (key_bytes != 4 && key_bytes != 8) return fail(MRG_ERR_ARG, "mrg_prims_radix_sort: keys of %u bytes (4 or 8)", key_bytes);
  if (bits > 8 * key_bytes) return fail(MRG_ERR_ARG, "mrg_prims_radix_sort: %u key bits of %u", bits, 8 * key_bytes);
  if (!ctx || !in_second) return fail(MRG_ERR_ARG, "mrg_prims_radix_sort: null argument");
  if (n >= 0xffffffffull) return fail(MRG_ERR_ARG, "mrg_prims_radix_sort: %llu keys; the limit is 2^32 - 2", (unsigned long long)n);
  if ((d_vals0 == nullptr) != (d_vals1 == nullptr)) return fail(MRG_ERR_ARG, "mrg_prims_radix_sort: one value buffer without the other");
  if (n && (!d_keys0 || !d_keys1 || !d_tmp)) return fail(MRG_ERR_ARG, "mrg_prims_radix_sort: null buffers");
  if (tmp_bytes < mrg::prims::radix_temp_bytes(n))
    return fail(MRG_ERR_ARG, "mrg_prims_radix_sort: scratch smaller than mrg_prims_temp_bytes");
  HIP_TRY(hipSetDevice(ctx->device));
  bool second = false;
  if (key_bytes == 8)
    HIP_TRY(mrg::prims::radix_sort_pairs_u64((uint64_t*)d_keys0, (uint64_t*)d_keys1, d_vals0, d_vals1, (uint32_t)n, bits, d_tmp,
                                             (hipStream_t)stream, &second));
  else
    HIP_TRY(mrg::prims::radix_sort_pairs_u32((uint32_t*)d_keys0, (uint32_t*)d_keys1, d_vals0, d_vals1, (uint32_t)n, bits, d_tmp,
                                             (hipStream_t)stream, &second));
  *in_second = second ? 1 : 0;
  return MRG_OK;
}

namespace {
int index_list(const char* who, const mrg_index* const* parts, uint32_t n_parts, std::vector<const mrg::FmIndex*>* ix) {
  if (n_parts && !parts) return fail(MRG_ERR_ARG, "%s: null argument", who);
  ix->resize(n_parts);
  for (uint32_t i = 0; i < n_parts; ++i) {
    if (!parts[i]) return fail(MRG_ERR_ARG, "%s: null index", who);
    (*ix)[i] = &parts[i]->ix;
  }
  return MRG_OK;
}
}  // namespace

int mrg_write_sorted_sam(const char* path, const mrg_index* const* parts, uint32_t n_parts, uint64_t n_reads, const char* names,
                         const uint64_t* names_off, const char* seqs, const uint64_t* seqs_off, uint64_t n_rows, const uint32_t* row_read,
                         const int32_t* entry, const int32_t* offset, const uint8_t* strand, const uint8_t* mm, const uint8_t* suppressed,
                         int32_t m, uint64_t* summary) {
  if (!path || !summary || (n_reads && (!names || !names_off || !seqs || !seqs_off)))
    return fail(MRG_ERR_ARG, "mrg_write_sorted_sam: null argument");
  if (n_rows && (!row_read || !entry || !offset || !strand || !mm)) return fail(MRG_ERR_ARG, "mrg_write_sorted_sam: null alignment arrays");
  std::vector<const mrg::FmIndex*> ix;
  int rc = index_list("mrg_write_sorted_sam", parts, n_parts, &ix);
  if (rc != MRG_OK) return rc;
  try {
    mrg::write_sorted_sam(path, ix, n_reads, names, names_off, seqs, seqs_off, n_rows, row_read, entry, offset, strand, mm, suppressed, m,
                          summary);
    return MRG_OK;
  } catch (const std::exception& e) {
    return fail(MRG_ERR_IO, "mrg_write_sorted_sam: %s", e.what());
  }
}

int mrg_write_clusters(const char* path, const char* sample, const mrg_index* const* parts, uint32_t n_parts, uint64_t n_clusters,
                       const uint32_t* entry, const uint8_t* strand, const uint32_t* start, const uint32_t* end, const uint64_t* seq_off,
                       const char* seq, const uint64_t* count_sum, const uint32_t* member_off, const uint32_t* members, uint64_t n_reads,
                       const char* names, const uint64_t* names_off, uint64_t* rows) {
  if (!path || !sample || !rows) return fail(MRG_ERR_ARG, "mrg_write_clusters: null argument");
  if (n_clusters && (!entry || !strand || !start || !end || !seq_off || !seq || !count_sum || !member_off || !members || !names || !names_off))
    return fail(MRG_ERR_ARG, "mrg_write_clusters: null cluster arrays");
  std::vector<const mrg::FmIndex*> ix;
  int rc = index_list("mrg_write_clusters", parts, n_parts, &ix);
  if (rc != MRG_OK) return rc;
  try {
    mrg::write_clusters(path, sample, ix, n_clusters, entry, strand, start, end, seq_off, seq, count_sum, member_off, members, n_reads,
                        names, names_off, rows);
    return MRG_OK;
  } catch (const std::exception& e) {
    return fail(MRG_ERR_IO, "mrg_write_clusters: %s", e.what());
  }
}

int mrg_read_counts_from_names(uint64_t n_reads, const char* names, const uint64_t* names_off, uint32_t* counts, int64_t* bad_read) {
  if (!bad_read || (n_reads && (!names || !names_off || !counts))) return fail(MRG_ERR_ARG, "mrg_read_counts_from_names: null argument");
  *bad_read = mrg::read_counts_from_names(n_reads, names, names_off, counts);
  if (*bad_read >= 0)
    return fail(MRG_ERR_FORMAT, "mrg_read_counts_from_names: read %lld has no `_<count>` field below 2^32 in its name", (long long)*bad_read);
  return MRG_OK;
}

// ------------------------------------------------- predict mode: the preliminary trim (csrc/predict_trim.hip)
namespace {
// mrg_predict_trim's scratch: the stat words, three uint32 arrays and one uint64 array of n + 1, the scans' own scratch
struct TrimScratch {
  Piece<uint32_t> stat, flag32, rank, keep_len;
  Piece<uint64_t> keep_off;
  Piece<char> scan;
  size_t total;
  explicit TrimScratch(uint64_t n) {
    Carver c(8);
    const uint64_t words = (n + 1 + 1) & ~1ull;  // (an even count: the uint64 array stays aligned)
    stat = c.take<uint32_t>(mrg::kTrimStatWords);
    flag32 = c.take<uint32_t>(words);
    rank = c.take<uint32_t>(words);
    keep_len = c.take<uint32_t>(words);
    keep_off = c.take<uint64_t>(n + 1);
    scan = c.take<char>(mrg::prims::scan_temp_bytes(n + 1));
    total = c.total();
  }
};
constexpr uint64_t kTrimMaxClusters = (1ull << 31) - 1, kTrimMaxBytes = (1ull << 38) - 1;
}  // namespace

int mrg_predict_trim_temp_bytes(uint64_t n_clusters, uint64_t* bytes) {
  if (!bytes) return fail(MRG_ERR_ARG, "mrg_predict_trim_temp_bytes: null argument");
  if (n_clusters > kTrimMaxClusters)
    return fail(MRG_ERR_ARG, "mrg_predict_trim_temp_bytes: %llu clusters; the limit is 2^31 - 1", (unsigned long long)n_clusters);
  *bytes = TrimScratch(n_clusters).total;
  return MRG_OK;
}

int mrg_predict_trim(mrg_ctx* ctx, uint64_t n_clusters, const uint32_t* d_entry, const uint8_t* d_strand, const uint32_t* d_start,
                     const uint32_t* d_end, const uint64_t* d_seq_off, const char* d_seq, uint64_t total_len, uint32_t n_entries,
                     const uint32_t* d_rep_off, const uint32_t* d_rep_start, const uint32_t* d_rep_end, uint64_t n_elements,
                     int32_t len_cutoff, uint8_t* d_flag, int32_t* d_rep, char* d_orig, uint32_t* d_kept, uint64_t* d_kept_seq_off,
                     char* d_kept_orig, uint64_t* n_kept, uint64_t* kept_len, void* d_tmp, uint64_t tmp_bytes, void* stream) {
  const char* fn = "mrg_predict_trim";
  if (!ctx || !n_kept || !kept_len) return fail(MRG_ERR_ARG, "%s: null argument", fn);
  *n_kept = *kept_len = 0;
  if (n_clusters > kTrimMaxClusters) return fail(MRG_ERR_ARG, "%s: %llu clusters; the limit is 2^31 - 1", fn, (unsigned long long)n_clusters);
  if (total_len > kTrimMaxBytes) return fail(MRG_ERR_ARG, "%s: %llu sequence bytes; the limit is 2^38 - 1", fn, (unsigned long long)total_len);
  if (n_elements >= 0xffffffffull) return fail(MRG_ERR_ARG, "%s: %llu repeat elements; the limit is 2^32 - 2", fn, (unsigned long long)n_elements);
  if (len_cutoff < 0) return fail(MRG_ERR_ARG, "%s: the length cutoff must not be negative (got %d)", fn, len_cutoff);
  if (!d_seq_off || !d_kept_seq_off || !d_tmp || !d_rep_off) return fail(MRG_ERR_ARG, "%s: null buffers", fn);
  if (n_clusters && (!d_entry || !d_strand || !d_start || !d_end || !d_flag || !d_rep || !d_kept))
    return fail(MRG_ERR_ARG, "%s: null cluster arrays", fn);
  if (total_len && (!n_clusters || !d_seq || !d_orig || !d_kept_orig)) return fail(MRG_ERR_ARG, "%s: null sequence buffers", fn);
  if (n_elements && (!d_rep_start || !d_rep_end)) return fail(MRG_ERR_ARG, "%s: null repeat table", fn);
  const TrimScratch sc(n_clusters);
  if (int rc = scratch_ok(fn, d_tmp, tmp_bytes, sc.total, "mrg_predict_trim_temp_bytes")) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  uint32_t *stat = sc.stat.at(d_tmp), *flag32 = sc.flag32.at(d_tmp), *rank = sc.rank.at(d_tmp), *keep_len = sc.keep_len.at(d_tmp);
  uint64_t* keep_off = sc.keep_off.at(d_tmp);
  void* scan_tmp = sc.scan.at(d_tmp);
  const mrg::TrimClusters c{(uint32_t)n_clusters, d_entry, d_strand, d_start, d_end, d_seq_off, d_seq, total_len};
  const mrg::TrimRepeats r{n_entries, (uint32_t)n_elements, d_rep_off, d_rep_start, d_rep_end};
  HIP_TRY(hipMemsetAsync(stat, 0, mrg::kTrimStatWords * sizeof(uint32_t), st));
  HIP_TRY(mrg::trim_orig_launch(c, d_orig, stat, st));
  HIP_TRY(mrg::trim_flags_launch(c, r, d_orig, (uint32_t)len_cutoff, d_flag, d_rep, flag32, keep_len, stat, st));
  HIP_TRY(mrg::prims::exclusive_sum_u32(flag32, rank, n_clusters + 1, scan_tmp, st));
  HIP_TRY(mrg::prims::exclusive_sum_u32_to_u64(keep_len, keep_off, n_clusters + 1, scan_tmp, st));
  HIP_TRY(mrg::trim_compact_launch((uint32_t)n_clusters, rank, keep_off, d_kept, d_kept_seq_off, st));
  HIP_TRY(mrg::trim_gather_launch(c, d_orig, rank, keep_off, d_kept_orig, st));
  uint32_t h_stat[mrg::kTrimStatWords] = {0, 0, 0, 0}, h_kept = 0;
  uint64_t h_len = 0;
  HIP_TRY(hipMemcpyAsync(&h_kept, rank + n_clusters, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(&h_len, keep_off + n_clusters, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  if (int rc = read_stat(stat, h_stat, mrg::kTrimStatWords, st)) return rc;
  if (h_stat[mrg::kTrimStatBadSeqOff]) return fail(MRG_ERR_ARG, "%s: d_seq_off does not ascend from 0 to total_len", fn);
  if (h_stat[mrg::kTrimStatBadEntry]) return fail(MRG_ERR_ARG, "%s: a cluster on an entry beyond the %u of the repeat table", fn, n_entries);
  if (h_stat[mrg::kTrimStatBadTable]) return fail(MRG_ERR_ARG, "%s: d_rep_off does not ascend inside the %llu elements", fn, (unsigned long long)n_elements);
  *n_kept = h_kept;
  *kept_len = h_len;
  return MRG_OK;
}

int mrg_write_trimmed_clusters(const char* tsv_path, const char* fa_path, const char* orig_fa_path, const char* sample,
                               const mrg_index* const* parts, uint32_t n_parts, uint64_t n_clusters, const uint32_t* entry,
                               const uint8_t* strand, const uint32_t* start, const uint32_t* end, const uint64_t* seq_off, const char* seq,
                               const uint64_t* count_sum, const uint32_t* member_off, const uint32_t* members, uint64_t n_reads,
                               const char* names, const uint64_t* names_off, const uint8_t* flag, const int32_t* rep, const char* orig,
                               uint64_t n_elements, const uint32_t* rep_name_id, uint64_t n_rep_names, const char* rep_names,
                               const uint64_t* rep_names_off, uint64_t* rows, uint64_t* kept) {
  const char* fn = "mrg_write_trimmed_clusters";
  if (!tsv_path || !fa_path || !orig_fa_path || !sample || !rows || !kept) return fail(MRG_ERR_ARG, "%s: null argument", fn);
  if (n_clusters && (!entry || !strand || !start || !end || !seq_off || !seq || !count_sum || !member_off || !members || !names ||
                     !names_off || !flag || !rep || !orig))
    return fail(MRG_ERR_ARG, "%s: null cluster arrays", fn);
  if (n_elements && (!rep_name_id || !rep_names || !rep_names_off)) return fail(MRG_ERR_ARG, "%s: null repeat names", fn);
  std::vector<const mrg::FmIndex*> ix;
  int rc = index_list(fn, parts, n_parts, &ix);
  if (rc != MRG_OK) return rc;
  return guarded(fn, [&] {
    const mrg::TrimmedClustersArgs a{tsv_path, fa_path,   orig_fa_path, sample,  &ix,   n_clusters, entry, strand,     start,
                                     end,      seq_off,   seq,          count_sum, member_off, members, n_reads, names, names_off,
                                     flag,     rep,       orig,         n_elements, rep_name_id, n_rep_names, rep_names, rep_names_off};
    mrg::write_trimmed_clusters(a, rows, kept);
    return MRG_OK;
  });
}

// ------------------------------------------------- predict mode: the second mapping (csrc/predict_remap.hip)
namespace {
constexpr uint64_t kRemapMaxReads = (1ull << 31) - 1, kRemapMaxRows = 0xfffffffeull;
// mrg_predict_trim_reads' scratch: two uint32 arrays of n + 1 and the scan's own
struct RemapTrimScratch {
  Piece<uint32_t> flag32, rank;
  Piece<char> scan;
  size_t total;
  explicit RemapTrimScratch(uint64_t n) {
    Carver c(8);
    flag32 = c.take<uint32_t>(n + 1);
    rank = c.take<uint32_t>(n + 1);
    scan = c.take<char>(mrg::prims::scan_temp_bytes(n + 1));
    total = c.total();
  }
};
// mrg_predict_remap_rows' scratch: the stat words, three uint64 and five uint32 arrays and two byte arrays of T, the sort's own
struct RemapRowsScratch {
  Piece<uint32_t> stat;
  Piece<uint64_t> key0, key1, ckey;
  Piece<uint32_t> vals0, vals1, read, cluster, offset;
  Piece<uint8_t> mm, pass;
  Piece<char> sort;
  size_t total;
  explicit RemapRowsScratch(uint64_t rows) {
    Carver c(8);
    stat = c.take<uint32_t>(mrg::kRemapStatWords);
    key0 = c.take<uint64_t>(rows);
    key1 = c.take<uint64_t>(rows);
    ckey = c.take<uint64_t>(rows);
    vals0 = c.take<uint32_t>(rows);
    vals1 = c.take<uint32_t>(rows);
    read = c.take<uint32_t>(rows);
    cluster = c.take<uint32_t>(rows);
    offset = c.take<uint32_t>(rows);
    mm = c.take<uint8_t>(rows);
    pass = c.take<uint8_t>(rows);
    sort = c.take<char>(mrg::prims::radix_temp_bytes(rows));
    total = c.total();
  }
};
}  // namespace

int mrg_predict_remap_temp_bytes(uint64_t n_reads, uint64_t n_rows, uint64_t* bytes) {
  const char* fn = "mrg_predict_remap_temp_bytes";
  if (!bytes) return fail(MRG_ERR_ARG, "%s: null argument", fn);
  if (n_reads > kRemapMaxReads) return fail(MRG_ERR_ARG, "%s: %llu reads; the limit is 2^31 - 1", fn, (unsigned long long)n_reads);
  if (n_rows > kRemapMaxRows) return fail(MRG_ERR_ARG, "%s: %llu rows; the limit is 2^32 - 2", fn, (unsigned long long)n_rows);
  *bytes = std::max(RemapTrimScratch(n_reads).total, RemapRowsScratch(n_rows).total);
  return MRG_OK;
}

int mrg_predict_trim_reads(mrg_ctx* ctx, const uint64_t* d_reads, uint32_t words_per_read, uint64_t stride, const uint8_t* d_lens,
                           const uint64_t* d_nmask, uint64_t n, const uint32_t* d_counts, uint32_t trim5, uint32_t trim3, uint32_t* d_sel,
                           uint64_t* d_out_reads, uint8_t* d_out_lens, uint64_t* d_out_nmask, uint64_t* n_sel, void* d_tmp,
                           uint64_t tmp_bytes, void* stream) {
  const char* fn = "mrg_predict_trim_reads";
  if (!ctx || !n_sel) return fail(MRG_ERR_ARG, "%s: null argument", fn);
  *n_sel = 0;
  if (n > kRemapMaxReads) return fail(MRG_ERR_ARG, "%s: %llu reads; the limit is 2^31 - 1", fn, (unsigned long long)n);
  if (words_per_read < 1 || words_per_read > 8) return fail(MRG_ERR_ARG, "%s: words_per_read must be 1 .. 8", fn);
  if (stride < n) return fail(MRG_ERR_ARG, "%s: a stride of %llu for %llu reads", fn, (unsigned long long)stride, (unsigned long long)n);
  if (trim5 > 255 || trim3 > 255) return fail(MRG_ERR_ARG, "%s: trims beyond the longest read (255)", fn);
  if (!d_tmp) return fail(MRG_ERR_ARG, "%s: null buffers", fn);
  if (n && (!d_reads || !d_lens || !d_counts || !d_sel || !d_out_reads || !d_out_lens || (d_nmask && !d_out_nmask)))
    return fail(MRG_ERR_ARG, "%s: null buffers", fn);
  const RemapTrimScratch sc(n);
  if (int rc = scratch_ok(fn, d_tmp, tmp_bytes, sc.total, "mrg_predict_remap_temp_bytes")) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  uint32_t *flag32 = sc.flag32.at(d_tmp), *rank = sc.rank.at(d_tmp);
  HIP_TRY(mrg::remap_mark_launch(d_counts, (uint32_t)n, flag32, st));
  HIP_TRY(mrg::prims::exclusive_sum_u32(flag32, rank, n + 1, sc.scan.at(d_tmp), st));
  HIP_TRY(mrg::remap_compact_launch((uint32_t)n, rank, d_sel, st));
  uint32_t k = 0;
  HIP_TRY(hipMemcpyAsync(&k, rank + n, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (k > n) return fail(MRG_ERR_HIP, "%s: %u reads picked of %llu", fn, k, (unsigned long long)n);
  const mrg::RemapReads in{d_reads, words_per_read, stride, d_lens, d_nmask, (uint32_t)n};
  HIP_TRY(mrg::remap_trim_launch(in, d_sel, k, trim5, trim3, d_out_reads, d_out_lens, d_out_nmask, st));
  *n_sel = k;
  return MRG_OK;
}

int mrg_predict_remap_rows(mrg_ctx* ctx, uint64_t n_reads, const uint32_t* d_numbers, uint64_t n_clusters, const uint32_t* d_kept,
                           const uint64_t* d_off1, uint64_t rows1, const int32_t* d_ref1, const int32_t* d_pos1, const uint8_t* d_mm1,
                           uint64_t n_sel, const uint32_t* d_sel, const uint64_t* d_off2, uint64_t rows2, const int32_t* d_ref2,
                           const int32_t* d_pos2, const uint8_t* d_mm2, uint32_t* d_read, uint32_t* d_cluster, uint32_t* d_offset,
                           uint8_t* d_mm, uint8_t* d_pass, void* d_tmp, uint64_t tmp_bytes, void* stream) {
  const char* fn = "mrg_predict_remap_rows";
  if (!ctx) return fail(MRG_ERR_ARG, "%s: null argument", fn);
  if (n_reads > kRemapMaxReads || n_sel > n_reads)
    return fail(MRG_ERR_ARG, "%s: %llu reads (the limit is 2^31 - 1), %llu of them in pass 2", fn, (unsigned long long)n_reads,
                (unsigned long long)n_sel);
  if (n_clusters > kRemapMaxReads) return fail(MRG_ERR_ARG, "%s: %llu clusters; the limit is 2^31 - 1", fn, (unsigned long long)n_clusters);
  if (rows1 > kRemapMaxRows || rows2 > kRemapMaxRows || rows1 + rows2 > kRemapMaxRows)
    return fail(MRG_ERR_ARG, "%s: %llu rows; the limit is 2^32 - 2", fn, (unsigned long long)(rows1 + rows2));
  const uint64_t T = rows1 + rows2;
  if (!d_tmp) return fail(MRG_ERR_ARG, "%s: null buffers", fn);
  if (rows1 && (!n_reads || !d_off1 || !d_ref1 || !d_pos1 || !d_mm1)) return fail(MRG_ERR_ARG, "%s: null pass-1 listing", fn);
  if (rows2 && (!n_sel || !d_sel || !d_off2 || !d_ref2 || !d_pos2 || !d_mm2)) return fail(MRG_ERR_ARG, "%s: null pass-2 listing", fn);
  if (T && (!n_clusters || !d_numbers || !d_kept || !d_read || !d_cluster || !d_offset || !d_mm || !d_pass))
    return fail(MRG_ERR_ARG, "%s: null row buffers", fn);
  const RemapRowsScratch sc(T);
  if (int rc = scratch_ok(fn, d_tmp, tmp_bytes, sc.total, "mrg_predict_remap_temp_bytes")) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  uint32_t* stat = sc.stat.at(d_tmp);
  uint64_t *key0 = sc.key0.at(d_tmp), *key1 = sc.key1.at(d_tmp), *ckey = sc.ckey.at(d_tmp);
  uint32_t *vals0 = sc.vals0.at(d_tmp), *vals1 = sc.vals1.at(d_tmp);
  void* sort_tmp = sc.sort.at(d_tmp);
  const mrg::RemapRows listed{sc.read.at(d_tmp), sc.cluster.at(d_tmp), sc.offset.at(d_tmp), sc.mm.at(d_tmp), sc.pass.at(d_tmp)};
  HIP_TRY(hipMemsetAsync(stat, 0, mrg::kRemapStatWords * sizeof(uint32_t), st));
  // a listing without rows has no say: its offsets are not read
  const mrg::RemapListing p1{d_off1, rows1 ? (uint32_t)n_reads : 0u, d_ref1, d_pos1, d_mm1, (uint32_t)rows1};
  const mrg::RemapListing p2{d_off2, rows2 ? (uint32_t)n_sel : 0u, d_ref2, d_pos2, d_mm2, (uint32_t)rows2};
  const mrg::RemapMergeArgs a{p1, p2, d_sel, (uint32_t)n_reads, d_numbers, (uint32_t)n_clusters, d_kept, listed, key0, ckey, vals0, stat};
  if (T) {
    HIP_TRY(mrg::remap_merge_launch(a, st));
    // by read name, then (stable) by cluster name: the order of `sort -k6,6 -k1,1` up to the rows equal in both
    bool second = false;
    HIP_TRY(mrg::prims::radix_sort_pairs_u64(key0, key1, vals0, vals1, (uint32_t)T, mrg::kRemapKeyBits, sort_tmp, st, &second));
    uint32_t* by_read = second ? vals1 : vals0;
    uint32_t* spare = second ? vals0 : vals1;
    HIP_TRY(mrg::remap_gather_keys_launch(ckey, by_read, (uint32_t)T, key0, st));
    HIP_TRY(mrg::prims::radix_sort_pairs_u64(key0, key1, by_read, spare, (uint32_t)T, mrg::kRemapKeyBits, sort_tmp, st, &second));
    const mrg::RemapRows out{d_read, d_cluster, d_offset, d_mm, d_pass};
    HIP_TRY(mrg::remap_gather_rows_launch(listed, second ? spare : by_read, (uint32_t)T, out, st));
  }
  uint32_t h_stat[mrg::kRemapStatWords] = {0, 0, 0, 0};
  if (int rc = read_stat(stat, h_stat, mrg::kRemapStatWords, st)) return rc;
  if (h_stat[mrg::kRemapStatBadOffsets]) return fail(MRG_ERR_ARG, "%s: a listing's offsets do not ascend from 0 to its rows", fn);
  if (h_stat[mrg::kRemapStatBadCluster]) return fail(MRG_ERR_ARG, "%s: a row on an entry beyond the %llu clusters, or at a negative offset", fn, (unsigned long long)n_clusters);
  if (h_stat[mrg::kRemapStatBadRead]) return fail(MRG_ERR_ARG, "%s: a pass-2 read beyond the %llu reads", fn, (unsigned long long)n_reads);
  return MRG_OK;
}

int mrg_write_remapped_rows(const char* path, const uint64_t* reads, uint32_t words_per_read, uint64_t stride, const uint8_t* lens,
                            const uint64_t* nmask, uint64_t n_reads, const uint32_t* numbers, const uint32_t* counts,
                            const mrg_index* clusters, uint64_t n_clusters, const uint64_t* kept_seq_off, const char* kept_orig,
                            uint64_t n_rows, const uint32_t* row_read, const uint32_t* row_cluster, const uint32_t* row_offset,
                            const uint8_t* row_mm, const uint8_t* row_pass, uint32_t trim5, uint32_t trim3, uint64_t* rows) {
  const char* fn = "mrg_write_remapped_rows";
  if (!path || !rows) return fail(MRG_ERR_ARG, "%s: null argument", fn);
  *rows = 0;
  if (n_reads && (!reads || !lens || !numbers || !counts)) return fail(MRG_ERR_ARG, "%s: null read arrays", fn);
  if (n_clusters && (!clusters || !kept_seq_off || !kept_orig)) return fail(MRG_ERR_ARG, "%s: null cluster arrays", fn);
  if (n_rows && (!row_read || !row_cluster || !row_offset || !row_mm || !row_pass)) return fail(MRG_ERR_ARG, "%s: null row arrays", fn);
  if (words_per_read < 1 || words_per_read > 8 || stride < n_reads) return fail(MRG_ERR_ARG, "%s: words_per_read must be 1 .. 8 and the stride cover the reads", fn);
  return guarded(fn, [&] {
    const mrg::RemappedRowsArgs a{path,      reads,        words_per_read, stride,   lens,     nmask,       n_reads,    numbers,
                                  counts,     clusters ? &clusters->ix : nullptr,     n_clusters, kept_seq_off, kept_orig, n_rows,
                                  row_read,   row_cluster,  row_offset,     row_mm,   row_pass, trim5,       trim3};
    *rows = mrg::write_remapped_rows(a);
    return MRG_OK;
  });
}

// ------------------------------------------------- predict mode: the cluster feature table (csrc/predict_features.hip)
namespace {
constexpr uint64_t kFeatMaxRows = 0xfffffffeull, kFeatMaxItems = (1ull << 31) - 1;
// mrg_predict_feature_groups' scratch: the stat words, two uint32 arrays of n_rows + 1 and the scan's own
struct FeatGroupScratch {
  Piece<uint32_t> stat, flag32, rank;
  Piece<char> scan;
  size_t total;
  explicit FeatGroupScratch(uint64_t rows) {
    Carver c(8);
    stat = c.take<uint32_t>(mrg::kFeatStatWords);
    flag32 = c.take<uint32_t>(rows + 1);
    rank = c.take<uint32_t>(rows + 1);
    scan = c.take<char>(mrg::prims::scan_temp_bytes(rows + 1));
    total = c.total();
  }
};
// mrg_predict_feature_neighbors' scratch: the stat words, five uint64 and two uint32 arrays of G, the sort's own
struct FeatNeighborScratch {
  Piece<uint32_t> stat;
  Piece<uint64_t> key_c, key_se, key_r, keys0, keys1;
  Piece<uint32_t> vals0, vals1;
  Piece<char> sort;
  size_t total;
  explicit FeatNeighborScratch(uint64_t G) {
    Carver c(8);
    stat = c.take<uint32_t>(mrg::kFeatStatWords);
    key_c = c.take<uint64_t>(G);
    key_se = c.take<uint64_t>(G);
    key_r = c.take<uint64_t>(G);
    keys0 = c.take<uint64_t>(G);
    keys1 = c.take<uint64_t>(G);
    vals0 = c.take<uint32_t>(G);
    vals1 = c.take<uint32_t>(G);
    sort = c.take<char>(mrg::prims::radix_temp_bytes(G));
    total = c.total();
  }
};
int feat_stat_error(const char* fn, const uint32_t* h_stat) {
  if (h_stat[mrg::kFeatStatBadRow]) return fail(MRG_ERR_ARG, "%s: a row names no read or no retained cluster", fn);
  if (h_stat[mrg::kFeatStatBadCluster])
    return fail(MRG_ERR_ARG, "%s: a cluster on no entry, or whose end - start + 1 is not its sequence length, or sequence offsets that do not ascend", fn);
  if (h_stat[mrg::kFeatStatBadGroups]) return fail(MRG_ERR_ARG, "%s: group offsets that do not ascend inside the rows, or a group of no cluster", fn);
  return MRG_OK;
}
}  // namespace

int mrg_predict_feature_temp_bytes(uint64_t n_rows, uint64_t* bytes) {
  const char* fn = "mrg_predict_feature_temp_bytes";
  if (!bytes) return fail(MRG_ERR_ARG, "%s: null argument", fn);
  if (n_rows > kFeatMaxRows) return fail(MRG_ERR_ARG, "%s: %llu rows; the limit is 2^32 - 2", fn, (unsigned long long)n_rows);
  *bytes = std::max(FeatGroupScratch(n_rows).total, FeatNeighborScratch(n_rows).total);
  return MRG_OK;
}

int mrg_predict_feature_groups(mrg_ctx* ctx, uint64_t n_rows, const uint32_t* d_row_read, const uint32_t* d_row_cluster, uint64_t n_reads,
                               const uint32_t* d_counts, uint64_t n_clusters, const uint32_t* d_cl_entry, const uint32_t* d_cl_start,
                               const uint32_t* d_cl_end, const uint64_t* d_kept_seq_off, uint64_t orig_len, uint64_t n_entries,
                               const uint32_t* d_entry_len, uint32_t* d_row_group, uint32_t* d_group_off, uint32_t* d_group_cluster,
                               uint64_t* d_group_sum, uint8_t* d_group_pass, uint64_t* n_groups, uint64_t* n_passed, void* d_tmp,
                               uint64_t tmp_bytes, void* stream) {
  const char* fn = "mrg_predict_feature_groups";
  if (!ctx || !n_groups || !n_passed) return fail(MRG_ERR_ARG, "%s: null argument", fn);
  *n_groups = *n_passed = 0;
  if (n_rows > kFeatMaxRows) return fail(MRG_ERR_ARG, "%s: %llu rows; the limit is 2^32 - 2", fn, (unsigned long long)n_rows);
  if (n_reads > kFeatMaxItems || n_clusters > kFeatMaxItems || n_entries > kFeatMaxItems)
    return fail(MRG_ERR_ARG, "%s: reads, clusters and entries are limited to 2^31 - 1 each", fn);
  if (!d_tmp) return fail(MRG_ERR_ARG, "%s: null buffers", fn);
  if (n_rows && (!d_row_read || !d_row_cluster || !d_counts || !d_cl_entry || !d_cl_start || !d_cl_end || !d_kept_seq_off || !d_entry_len ||
                 !d_row_group || !d_group_off || !d_group_cluster || !d_group_sum || !d_group_pass))
    return fail(MRG_ERR_ARG, "%s: null arrays", fn);
  if (n_rows && (!n_reads || !n_clusters || !n_entries)) return fail(MRG_ERR_ARG, "%s: rows without reads, clusters or entries", fn);
  const FeatGroupScratch sc(n_rows);
  if (int rc = scratch_ok(fn, d_tmp, tmp_bytes, sc.total, "mrg_predict_feature_temp_bytes")) return rc;
  if (n_rows == 0) return MRG_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  uint32_t *stat = sc.stat.at(d_tmp), *flag32 = sc.flag32.at(d_tmp), *rank = sc.rank.at(d_tmp);
  const mrg::FeatRows rows{(uint32_t)n_rows, d_row_read, d_row_cluster};
  const mrg::FeatReads reads{nullptr, nullptr, nullptr, d_counts, (uint32_t)n_reads};
  const mrg::FeatClusters cl{(uint32_t)n_clusters, d_cl_entry, nullptr, d_cl_start, d_cl_end, nullptr, d_kept_seq_off, nullptr, orig_len};
  HIP_TRY(hipMemsetAsync(stat, 0, mrg::kFeatStatWords * sizeof(uint32_t), st));
  HIP_TRY(mrg::feat_mark_launch(rows, (uint32_t)n_reads, (uint32_t)n_clusters, flag32, stat, st));
  HIP_TRY(mrg::prims::exclusive_sum_u32(flag32, rank, n_rows + 1, sc.scan.at(d_tmp), st));
  uint32_t h_stat[mrg::kFeatStatWords] = {0}, G = 0;
  HIP_TRY(hipMemcpyAsync(&G, rank + n_rows, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  if (int rc = read_stat(stat, h_stat, mrg::kFeatStatWords, st)) return rc;
  if (int rc = feat_stat_error(fn, h_stat)) return rc;   // (rows of no cluster: the groups would mean nothing)
  if (G == 0 || G > n_rows) return fail(MRG_ERR_HIP, "%s: %u groups of %llu rows", fn, G, (unsigned long long)n_rows);
  HIP_TRY(mrg::feat_starts_launch(rows, rank, d_row_group, d_group_off, d_group_cluster, st));
  HIP_TRY(mrg::feat_filter_launch(G, d_group_off, d_group_cluster, rows, reads, cl, (uint32_t)n_entries, d_entry_len, d_group_sum, d_group_pass,
                                  stat, st));
  if (int rc = read_stat(stat, h_stat, mrg::kFeatStatWords, st)) return rc;
  if (int rc = feat_stat_error(fn, h_stat)) return rc;
  *n_groups = G;
  *n_passed = h_stat[mrg::kFeatStatPassed];
  return MRG_OK;
}

int mrg_predict_feature_align(mrg_ctx* ctx, uint64_t n_rows, const uint32_t* d_row_read, const uint32_t* d_row_cluster,
                              const uint32_t* d_row_group, uint64_t n_groups, const uint8_t* d_group_pass, const uint64_t* d_reads,
                              const uint8_t* d_lens, const uint64_t* d_nmask, uint64_t n_reads, uint64_t n_clusters,
                              const uint64_t* d_kept_seq_off, const char* d_kept_orig, uint64_t orig_len, uint64_t* d_cl_word,
                              uint8_t* d_cl_len, uint8_t* d_row_status, int32_t* d_row_diag, uint8_t* d_row_ident, uint8_t* d_group_host,
                              void* d_tmp, uint64_t tmp_bytes, void* stream) {
  const char* fn = "mrg_predict_feature_align";
  if (!ctx) return fail(MRG_ERR_ARG, "%s: null argument", fn);
  if (n_rows > kFeatMaxRows || n_groups > n_rows) return fail(MRG_ERR_ARG, "%s: %llu groups of %llu rows (the limit is 2^32 - 2 rows)", fn,
                                                              (unsigned long long)n_groups, (unsigned long long)n_rows);
  if (n_reads > kFeatMaxItems || n_clusters > kFeatMaxItems) return fail(MRG_ERR_ARG, "%s: reads and clusters are limited to 2^31 - 1 each", fn);
  if (!d_tmp || tmp_bytes < stat_only_bytes(mrg::kFeatStatWords) || ((uintptr_t)d_tmp & 7))
    return fail(MRG_ERR_ARG, "%s: scratch smaller than mrg_predict_feature_temp_bytes, or unaligned", fn);
  if (n_clusters && (!d_kept_seq_off || (orig_len && !d_kept_orig) || !d_cl_word || !d_cl_len)) return fail(MRG_ERR_ARG, "%s: null cluster arrays", fn);
  if (n_rows && (!n_groups || !n_reads || !n_clusters || !d_row_read || !d_row_cluster || !d_row_group || !d_group_pass || !d_reads || !d_lens ||
                 !d_row_status || !d_row_diag || !d_row_ident || !d_group_host))
    return fail(MRG_ERR_ARG, "%s: null row arrays", fn);
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  uint32_t* stat = reinterpret_cast<uint32_t*>(d_tmp);
  const mrg::FeatClusters cl{(uint32_t)n_clusters, nullptr, nullptr, nullptr, nullptr, nullptr, d_kept_seq_off, d_kept_orig, orig_len};
  HIP_TRY(hipMemsetAsync(stat, 0, mrg::kFeatStatWords * sizeof(uint32_t), st));
  HIP_TRY(mrg::feat_pack_launch(cl, d_cl_word, d_cl_len, stat, st));
  if (n_rows) {
    HIP_TRY(hipMemsetAsync(d_group_host, 0, n_groups, st));
    mrg::FeatAlignArgs a;
    a.rows = mrg::FeatRows{(uint32_t)n_rows, d_row_read, d_row_cluster};
    a.row_group = d_row_group;
    a.n_groups = (uint32_t)n_groups;
    a.group_pass = d_group_pass;
    a.reads = mrg::FeatReads{d_reads, d_lens, d_nmask, nullptr, (uint32_t)n_reads};
    a.n_clusters = (uint32_t)n_clusters;
    a.cl_word = d_cl_word;
    a.cl_len = d_cl_len;
    a.row_status = d_row_status;
    a.row_diag = d_row_diag;
    a.row_ident = d_row_ident;
    a.group_host = d_group_host;
    HIP_TRY(mrg::feat_align_launch(a, st));
  }
  uint32_t h_stat[mrg::kFeatStatWords] = {0};
  if (int rc = read_stat(stat, h_stat, mrg::kFeatStatWords, st)) return rc;
  return feat_stat_error(fn, h_stat);
}

int mrg_predict_feature_tally(mrg_ctx* ctx, uint64_t n_groups, const uint32_t* d_group_off, const uint32_t* d_group_cluster,
                              const uint8_t* d_group_pass, const uint8_t* d_group_host, uint64_t n_rows, const uint32_t* d_row_read,
                              const int32_t* d_row_diag, const uint8_t* d_row_ident, const uint64_t* d_reads, const uint8_t* d_lens,
                              uint64_t n_reads, const uint32_t* d_counts, uint64_t n_clusters, const uint8_t* d_cl_len, uint8_t* d_valid,
                              int32_t* d_frame, uint64_t* d_exact, uint64_t* d_nine, void* stream) {
  const char* fn = "mrg_predict_feature_tally";
  if (!ctx) return fail(MRG_ERR_ARG, "%s: null argument", fn);
  if (n_rows > kFeatMaxRows || n_groups > n_rows) return fail(MRG_ERR_ARG, "%s: %llu groups of %llu rows (the limit is 2^32 - 2 rows)", fn,
                                                              (unsigned long long)n_groups, (unsigned long long)n_rows);
  if (n_reads > kFeatMaxItems || n_clusters > kFeatMaxItems) return fail(MRG_ERR_ARG, "%s: reads and clusters are limited to 2^31 - 1 each", fn);
  if (n_groups && (!d_group_off || !d_group_cluster || !d_group_pass || !d_group_host || !d_row_read || !d_row_diag || !d_row_ident || !d_reads ||
                   !d_lens || !d_counts || !d_cl_len || !d_valid || !d_frame || !d_exact || !d_nine))
    return fail(MRG_ERR_ARG, "%s: null arrays", fn);
  if (n_groups == 0) return MRG_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  mrg::FeatTallyArgs a;
  a.n_groups = (uint32_t)n_groups;
  a.group_off = d_group_off;
  a.group_cluster = d_group_cluster;
  a.group_pass = d_group_pass;
  a.group_host = d_group_host;
  a.rows = mrg::FeatRows{(uint32_t)n_rows, d_row_read, nullptr};
  a.row_diag = d_row_diag;
  a.row_ident = d_row_ident;
  a.reads = mrg::FeatReads{d_reads, d_lens, nullptr, d_counts, (uint32_t)n_reads};
  a.n_clusters = (uint32_t)n_clusters;
  a.cl_len = d_cl_len;
  a.valid = d_valid;
  a.frame = d_frame;
  a.exact = d_exact;
  a.nine = d_nine;
  HIP_TRY(mrg::feat_tally_launch(a, (hipStream_t)stream));
  return MRG_OK;
}

int mrg_predict_feature_neighbors(mrg_ctx* ctx, uint64_t n_groups, const uint32_t* d_group_cluster, const uint8_t* d_valid,
                                  const int32_t* d_frame, uint64_t n_clusters, const uint32_t* d_cl_entry, const uint8_t* d_cl_strand,
                                  const uint32_t* d_cl_start, const uint32_t* d_cl_end, const uint32_t* d_kept, uint64_t n_entries,
                                  const uint32_t* d_entry_rank, uint32_t* d_order, uint32_t* d_nb_t, int64_t* d_nb_up, int64_t* d_nb_down,
                                  uint8_t* d_nb_flags, uint64_t* n_sorted, void* d_tmp, uint64_t tmp_bytes, void* stream) {
  const char* fn = "mrg_predict_feature_neighbors";
  if (!ctx || !n_sorted) return fail(MRG_ERR_ARG, "%s: null argument", fn);
  *n_sorted = 0;
  if (n_groups > kFeatMaxRows) return fail(MRG_ERR_ARG, "%s: %llu groups; the limit is 2^32 - 2", fn, (unsigned long long)n_groups);
  if (n_clusters > kFeatMaxItems || n_entries > kFeatMaxItems) return fail(MRG_ERR_ARG, "%s: clusters and entries are limited to 2^31 - 1 each", fn);
  if (!d_tmp) return fail(MRG_ERR_ARG, "%s: null buffers", fn);
  if (n_groups && (!n_clusters || !n_entries || !d_group_cluster || !d_valid || !d_frame || !d_cl_entry || !d_cl_strand || !d_cl_start ||
                   !d_cl_end || !d_kept || !d_entry_rank || !d_order || !d_nb_t || !d_nb_up || !d_nb_down || !d_nb_flags))
    return fail(MRG_ERR_ARG, "%s: null arrays", fn);
  const FeatNeighborScratch sc(n_groups);
  if (int rc = scratch_ok(fn, d_tmp, tmp_bytes, sc.total, "mrg_predict_feature_temp_bytes")) return rc;
  if (n_groups == 0) return MRG_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  uint32_t* stat = sc.stat.at(d_tmp);
  uint64_t *key_c = sc.key_c.at(d_tmp), *key_se = sc.key_se.at(d_tmp), *key_r = sc.key_r.at(d_tmp);
  uint64_t* keys[2] = {sc.keys0.at(d_tmp), sc.keys1.at(d_tmp)};
  uint32_t* vals[2] = {sc.vals0.at(d_tmp), sc.vals1.at(d_tmp)};
  const uint32_t G = (uint32_t)n_groups;
  mrg::FeatNeighborArgs a;
  a.n_groups = G;
  a.group_cluster = d_group_cluster;
  a.valid = d_valid;
  a.frame = d_frame;
  a.cl = mrg::FeatClusters{(uint32_t)n_clusters, d_cl_entry, d_cl_strand, d_cl_start, d_cl_end, d_kept, nullptr, nullptr, 0};
  a.n_entries = (uint32_t)n_entries;
  a.entry_rank = d_entry_rank;
  HIP_TRY(hipMemsetAsync(stat, 0, mrg::kFeatStatWords * sizeof(uint32_t), st));
  HIP_TRY(mrg::feat_keys_launch(a, key_c, key_se, key_r, vals[0], stat, st));
  // stable passes from the last key to the first: cluster number, (start, end), chromosome rank
  HIP_TRY(hipMemcpyAsync(keys[0], key_c, (size_t)G * sizeof(uint64_t), hipMemcpyDeviceToDevice, st));
  uint32_t at = 0;  // which vals buffer holds the order so far
  const uint64_t* later[2] = {key_se, key_r};
  const uint32_t bits[3] = {mrg::kRemapKeyBits, 64u, 32u};
  for (uint32_t pass = 0; pass < 3; ++pass) {
    if (pass) HIP_TRY(mrg::feat_gather_keys_launch(later[pass - 1], vals[at], G, keys[0], st));
    bool second = false;
    HIP_TRY(mrg::prims::radix_sort_pairs_u64(keys[0], keys[1], vals[at], vals[at ^ 1u], G, bits[pass], sc.sort.at(d_tmp), st, &second));
    if (second) at ^= 1u;
    if (pass == 2 && second) std::swap(keys[0], keys[1]);
  }
  HIP_TRY(hipMemcpyAsync(d_order, vals[at], (size_t)G * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
  HIP_TRY(mrg::feat_neighbors_launch(a, keys[0], d_order, d_nb_t, d_nb_up, d_nb_down, d_nb_flags, stat, st));
  uint32_t h_stat[mrg::kFeatStatWords] = {0};
  if (int rc = read_stat(stat, h_stat, mrg::kFeatStatWords, st)) return rc;
  if (int rc = feat_stat_error(fn, h_stat)) return rc;
  *n_sorted = h_stat[mrg::kFeatStatSorted];
  return MRG_OK;
}

int mrg_write_predict_features(const char* features_path, const char* cluster_path, int mapped, const mrg_index* const* parts,
                               uint32_t n_parts, const mrg_index* clusters, uint64_t n_clusters, const uint32_t* cl_entry,
                               const uint8_t* cl_strand, const uint32_t* cl_start, const uint32_t* cl_end, const uint64_t* kept_seq_off,
                               const char* kept_orig, const uint64_t* reads, uint32_t words_per_read, uint64_t stride, const uint8_t* lens,
                               const uint64_t* nmask, const uint32_t* counts, uint64_t n_reads, uint64_t n_rows, const uint32_t* row_read,
                               const int32_t* row_diag, uint64_t n_groups, const uint32_t* group_off, const uint32_t* group_cluster,
                               const int32_t* frame, const uint64_t* exact, const uint64_t* nine, const uint32_t* nb_t, const int64_t* nb_up,
                               const int64_t* nb_down, const uint8_t* nb_flags, const char* const* group_text, uint64_t n_order,
                               const uint32_t* order, uint64_t* written) {
  const char* fn = "mrg_write_predict_features";
  if (!features_path || !cluster_path || !written || !kept_seq_off) return fail(MRG_ERR_ARG, "%s: null argument", fn);
  written[0] = written[1] = 0;
  if (n_clusters && (!clusters || !cl_entry || !cl_strand || !cl_start || !cl_end || !kept_orig)) return fail(MRG_ERR_ARG, "%s: null cluster arrays", fn);
  if (n_reads && (!reads || !lens || !counts)) return fail(MRG_ERR_ARG, "%s: null read arrays", fn);
  if (n_rows && (!row_read || !row_diag)) return fail(MRG_ERR_ARG, "%s: null row arrays", fn);
  if (n_groups && (!group_off || !group_cluster || !frame || !exact || !nine || !nb_t || !nb_up || !nb_down || !nb_flags))
    return fail(MRG_ERR_ARG, "%s: null group arrays", fn);
  if (n_order && (!order || !n_groups)) return fail(MRG_ERR_ARG, "%s: an order without groups", fn);
  std::vector<const mrg::FmIndex*> ix;
  int rc = index_list(fn, parts, n_parts, &ix);
  if (rc != MRG_OK) return rc;
  return guarded(fn, [&] {
    mrg::FeatWriteArgs a;
    a.features_path = features_path;
    a.cluster_path = cluster_path;
    a.mapped = mapped != 0;
    a.parts = &ix;
    a.clusters = clusters ? &clusters->ix : nullptr;
    a.n_clusters = n_clusters;
    a.cl_entry = cl_entry;
    a.cl_strand = cl_strand;
    a.cl_start = cl_start;
    a.cl_end = cl_end;
    a.kept_seq_off = kept_seq_off;
    a.kept_orig = kept_orig;
    a.reads = reads;
    a.W = words_per_read;
    a.stride = stride;
    a.lens = lens;
    a.nmask = nmask;
    a.counts = counts;
    a.n_reads = n_reads;
    a.n_rows = n_rows;
    a.row_read = row_read;
    a.row_diag = row_diag;
    a.n_groups = n_groups;
    a.group_off = group_off;
    a.group_cluster = group_cluster;
    a.frame = frame;
    a.exact = exact;
    a.nine = nine;
    a.nb_t = nb_t;
    a.nb_up = nb_up;
    a.nb_down = nb_down;
    a.nb_flags = nb_flags;
    a.group_text = group_text;
    a.n_order = n_order;
    a.order = order;
    mrg::write_predict_features(a, written);
    return MRG_OK;
  });
}

// ------------------------------------------------- predict mode: the precursor candidates (csrc/predict_precursors.hip)
namespace {
constexpr uint64_t kPrecMaxGroups = (1ull << 30) - 1, kPrecMaxBytes = (1ull << 38) - 1;
// mrg_predict_precursors' scratch: the stat words, two uint32 arrays of S + 1, the windows [4 S], the lengths [2 S + 1] and
// the scan's own; mrg_predict_precursor_bases reads the stat words alone
struct PrecScratch {
  Piece<uint32_t> stat, flag32, rank, win, len32;
  Piece<char> scan;
  size_t total;
  explicit PrecScratch(uint64_t S) {
    Carver c(8);
    stat = c.take<uint32_t>(mrg::kPrecStatWords);
    flag32 = c.take<uint32_t>(S + 1);
    rank = c.take<uint32_t>(S + 1);
    win = c.take<uint32_t>(4 * S);
    len32 = c.take<uint32_t>(2 * S + 1);
    scan = c.take<char>(mrg::prims::scan_temp_bytes(2 * S + 1));
    total = c.total();
  }
};
int prec_stat_error(const char* fn, const uint32_t* h_stat) {
  if (h_stat[mrg::kPrecStatBadGroup]) return fail(MRG_ERR_ARG, "%s: the order or a record names no group, or a group without a stable column", fn);
  if (h_stat[mrg::kPrecStatBadCluster]) return fail(MRG_ERR_ARG, "%s: a group of no retained cluster", fn);
  if (h_stat[mrg::kPrecStatBadEntry]) return fail(MRG_ERR_ARG, "%s: a cluster on no entry", fn);
  if (h_stat[mrg::kPrecStatBadWindow]) return fail(MRG_ERR_ARG, "%s: a window that ends at or before its chromosome's first base", fn);
  if (h_stat[mrg::kPrecStatBadRecord])
    return fail(MRG_ERR_ARG, "%s: record offsets that do not ascend from 0 to seq_len by hi - lo, or a record outside its entry", fn);
  return MRG_OK;
}
// first_seg of a resident library, built the first time a precursor call names it: the segment table is ordered by
// (entry, offset), so entry e's segments are the run of seg_ref == e
int ensure_first_seg(const char* fn, DevLib& l) {
  if (l.first_seg) return MRG_OK;
  std::vector<uint32_t> ref(l.n_seg), off(l.n_seg), first((size_t)l.n_ref + 1, 0u);
  if (l.n_seg) {
    HIP_TRY(hipMemcpy(ref.data(), l.seg_ref, (size_t)l.n_seg * sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(off.data(), l.seg_off, (size_t)l.n_seg * sizeof(uint32_t), hipMemcpyDeviceToHost));
  }
  for (uint32_t s = 0; s < l.n_seg; ++s) {
    if (ref[s] >= l.n_ref || (s && (ref[s] < ref[s - 1] || (ref[s] == ref[s - 1] && off[s] <= off[s - 1]))))
      return fail(MRG_ERR_ARG, "%s: the library's segments are not ordered by (entry, offset)", fn);
    ++first[ref[s] + 1];
  }
  for (uint32_t e = 0; e < l.n_ref; ++e) first[e + 1] += first[e];
  return upload(&l.first_seg, first);
}
}  // namespace

int mrg_predict_precursor_temp_bytes(uint64_t n_order, uint64_t* bytes) {
  const char* fn = "mrg_predict_precursor_temp_bytes";
  if (!bytes) return fail(MRG_ERR_ARG, "%s: null argument", fn);
  if (n_order > kPrecMaxGroups) return fail(MRG_ERR_ARG, "%s: %llu groups; the limit is 2^30 - 1", fn, (unsigned long long)n_order);
  *bytes = PrecScratch(n_order).total;
  return MRG_OK;
}

int mrg_predict_precursors(mrg_ctx* ctx, uint64_t n_order, const uint32_t* d_order, uint64_t n_groups, const uint32_t* d_group_cluster,
                           const int32_t* d_frame, const uint8_t* d_valid, uint64_t n_clusters, const uint32_t* d_cl_entry,
                           const uint8_t* d_cl_strand, const uint32_t* d_cl_start, const uint32_t* d_cl_end, uint64_t n_entries,
                           const uint32_t* d_entry_len, uint8_t* d_written, uint32_t* d_rec_group, uint32_t* d_rec_lo, uint32_t* d_rec_hi,
                           uint64_t* d_rec_off, uint64_t* n_written, uint64_t* seq_len, void* d_tmp, uint64_t tmp_bytes, void* stream) {
  const char* fn = "mrg_predict_precursors";
  if (!ctx || !n_written || !seq_len) return fail(MRG_ERR_ARG, "%s: null argument", fn);
  *n_written = *seq_len = 0;
  if (n_order > kPrecMaxGroups || n_groups > kPrecMaxGroups || n_order > n_groups)
    return fail(MRG_ERR_ARG, "%s: %llu positions of %llu groups (the limit is 2^30 - 1)", fn, (unsigned long long)n_order, (unsigned long long)n_groups);
  if (n_clusters > kFeatMaxItems || n_entries > kFeatMaxItems) return fail(MRG_ERR_ARG, "%s: clusters and entries are limited to 2^31 - 1 each", fn);
  if (!d_tmp || !d_rec_off) return fail(MRG_ERR_ARG, "%s: null buffers", fn);
  if (n_order && (!d_order || !d_group_cluster || !d_frame || !d_valid || !d_cl_entry || !d_cl_strand || !d_cl_start || !d_cl_end || !d_entry_len ||
                  !d_written || !d_rec_group || !d_rec_lo || !d_rec_hi))
    return fail(MRG_ERR_ARG, "%s: null arrays", fn);
  const PrecScratch sc(n_order);
  if (int rc = scratch_ok(fn, d_tmp, tmp_bytes, sc.total, "mrg_predict_precursor_temp_bytes")) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  if (n_order == 0) {
    HIP_TRY(hipMemsetAsync(d_rec_off, 0, sizeof(uint64_t), st));
    HIP_TRY(hipStreamSynchronize(st));
    return MRG_OK;
  }
  uint32_t *stat = sc.stat.at(d_tmp), *flag32 = sc.flag32.at(d_tmp), *rank = sc.rank.at(d_tmp), *win = sc.win.at(d_tmp),
           *len32 = sc.len32.at(d_tmp);
  const mrg::PrecGroups g{(uint32_t)n_order, d_order, (uint32_t)n_groups, d_group_cluster, d_frame, d_valid};
  const mrg::PrecClusters cl{(uint32_t)n_clusters, d_cl_entry, d_cl_strand, d_cl_start, d_cl_end, (uint32_t)n_entries, d_entry_len};
  HIP_TRY(hipMemsetAsync(stat, 0, mrg::kPrecStatWords * sizeof(uint32_t), st));
  HIP_TRY(mrg::prec_windows_launch(g, cl, d_written, flag32, win, stat, st));
  HIP_TRY(mrg::prims::exclusive_sum_u32(flag32, rank, n_order + 1, sc.scan.at(d_tmp), st));
  uint32_t h_stat[mrg::kPrecStatWords] = {0}, W = 0;
  HIP_TRY(hipMemcpyAsync(&W, rank + n_order, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  if (int rc = read_stat(stat, h_stat, mrg::kPrecStatWords, st)) return rc;
  if (int rc = prec_stat_error(fn, h_stat)) return rc;
  if (W > n_order) return fail(MRG_ERR_HIP, "%s: %u groups written of %llu", fn, W, (unsigned long long)n_order);
  HIP_TRY(mrg::prec_compact_launch(g, rank, win, d_rec_group, d_rec_lo, d_rec_hi, len32, st));
  HIP_TRY(mrg::prims::exclusive_sum_u32_to_u64(len32, d_rec_off, 2ull * W + 1, sc.scan.at(d_tmp), st));
  uint64_t total = 0;
  HIP_TRY(hipMemcpyAsync(&total, d_rec_off + 2ull * W, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (total > kPrecMaxBytes) return fail(MRG_ERR_ARG, "%s: %llu sequence bytes; the limit is 2^38 - 1", fn, (unsigned long long)total);
  *n_written = W;
  *seq_len = total;
  return MRG_OK;
}

int mrg_predict_precursor_bases(mrg_ctx* ctx, uint64_t n_rec, const uint32_t* d_rec_group, const uint32_t* d_rec_lo, const uint32_t* d_rec_hi,
                                const uint64_t* d_rec_off, uint64_t n_groups, const uint32_t* d_group_cluster, uint64_t n_clusters,
                                const uint32_t* d_cl_entry, const uint8_t* d_cl_strand, uint64_t n_entries, const uint32_t* d_entry_len,
                                uint32_t n_parts, const int32_t* libs, const uint32_t* entry_base, char* d_seq, uint64_t seq_len, void* d_tmp,
                                uint64_t tmp_bytes, void* stream) {
  const char* fn = "mrg_predict_precursor_bases";
  if (!ctx) return fail(MRG_ERR_ARG, "%s: null argument", fn);
  if (n_rec > 2 * kPrecMaxGroups || n_groups > kPrecMaxGroups) return fail(MRG_ERR_ARG, "%s: records and groups are limited to 2^31 - 2 and 2^30 - 1", fn);
  if (n_clusters > kFeatMaxItems || n_entries > kFeatMaxItems) return fail(MRG_ERR_ARG, "%s: clusters and entries are limited to 2^31 - 1 each", fn);
  if (seq_len > kPrecMaxBytes) return fail(MRG_ERR_ARG, "%s: %llu sequence bytes; the limit is 2^38 - 1", fn, (unsigned long long)seq_len);
  if (!d_tmp || !d_rec_off || tmp_bytes < stat_only_bytes(mrg::kPrecStatWords) || ((uintptr_t)d_tmp & 7))
    return fail(MRG_ERR_ARG, "%s: scratch smaller than mrg_predict_precursor_temp_bytes, unaligned, or null offsets", fn);
  if (n_rec && (!d_rec_group || !d_rec_lo || !d_rec_hi || !d_group_cluster || !d_cl_entry || !d_cl_strand || !d_entry_len)) return fail(MRG_ERR_ARG, "%s: null arrays", fn);
  if (seq_len && (!n_rec || !d_seq)) return fail(MRG_ERR_ARG, "%s: sequence bytes without records or buffer", fn);
  if (n_parts > mrg::kPrecMaxParts || (n_parts && (!libs || !entry_base)))
    return fail(MRG_ERR_ARG, "%s: %u genome parts (the limit is %u), or null part tables", fn, n_parts, mrg::kPrecMaxParts);
  HIP_TRY(hipSetDevice(ctx->device));
  mrg::PrecGenome genome;
  std::memset(&genome, 0, sizeof genome);
  genome.n_parts = n_parts;
  uint64_t next = 0;
  for (uint32_t k = 0; k < n_parts; ++k) {
    if (libs[k] < 0 || (size_t)libs[k] >= ctx->libs.size()) return fail(MRG_ERR_ARG, "%s: unknown library %d", fn, libs[k]);
    DevLib& l = ctx->libs[libs[k]];
    if (entry_base[k] != next) return fail(MRG_ERR_ARG, "%s: part %u starts at entry %u, the parts before it hold %llu", fn, k, entry_base[k], (unsigned long long)next);
    next += l.n_ref;
    if (int rc = ensure_first_seg(fn, l)) return rc;
    genome.part[k] = mrg::PrecPart{l.text, l.seg_start, l.seg_off, l.first_seg, entry_base[k], l.n_ref};
  }
  if (n_rec && next != n_entries) return fail(MRG_ERR_ARG, "%s: the parts hold %llu entries, not the %llu given", fn, (unsigned long long)next, (unsigned long long)n_entries);
  hipStream_t st = (hipStream_t)stream;
  uint32_t* stat = reinterpret_cast<uint32_t*>(d_tmp);
  const mrg::PrecRecords r{(uint32_t)n_rec, d_rec_group, d_rec_lo, d_rec_hi, d_rec_off};
  const mrg::PrecGroups g{0u, nullptr, (uint32_t)n_groups, d_group_cluster, nullptr, nullptr};
  const mrg::PrecClusters cl{(uint32_t)n_clusters, d_cl_entry, d_cl_strand, nullptr, nullptr, (uint32_t)n_entries, d_entry_len};
  HIP_TRY(hipMemsetAsync(stat, 0, mrg::kPrecStatWords * sizeof(uint32_t), st));
  HIP_TRY(mrg::prec_check_launch(r, g, cl, seq_len, stat, st));
  uint32_t h_stat[mrg::kPrecStatWords] = {0};
  if (int rc = read_stat(stat, h_stat, mrg::kPrecStatWords, st)) return rc;
  if (int rc = prec_stat_error(fn, h_stat)) return rc;  // (before a byte is written: the bases kernel trusts the records)
  HIP_TRY(mrg::prec_bases_launch(r, g, cl, genome, seq_len, d_seq, st));
  HIP_TRY(hipStreamSynchronize(st));
  return MRG_OK;
}

int mrg_write_precursors(const char* path, const mrg_index* const* parts, uint32_t n_parts, const mrg_index* clusters, uint64_t n_clusters,
                         const uint32_t* cl_entry, uint64_t n_groups, const uint32_t* group_cluster, uint64_t n_rec, const uint32_t* rec_group,
                         const uint32_t* rec_lo, const uint32_t* rec_hi, const uint64_t* rec_off, const char* seq, uint64_t seq_len,
                         uint64_t* written) {
  const char* fn = "mrg_write_precursors";
  if (!path || !written || !rec_off) return fail(MRG_ERR_ARG, "%s: null argument", fn);
  written[0] = written[1] = 0;
  if (n_clusters && (!clusters || !cl_entry)) return fail(MRG_ERR_ARG, "%s: null cluster arrays", fn);
  if (n_groups && !group_cluster) return fail(MRG_ERR_ARG, "%s: null group arrays", fn);
  if (n_rec && (!rec_group || !rec_lo || !rec_hi)) return fail(MRG_ERR_ARG, "%s: null record arrays", fn);
  if (seq_len && !seq) return fail(MRG_ERR_ARG, "%s: null sequence bytes", fn);
  std::vector<const mrg::FmIndex*> ix;
  int rc = index_list(fn, parts, n_parts, &ix);
  if (rc != MRG_OK) return rc;
  return guarded(fn, [&] {
    const mrg::PrecWriteArgs a{path, &ix, clusters ? &clusters->ix : nullptr, n_clusters, cl_entry, n_groups, group_cluster, n_rec, rec_group,
                               rec_lo, rec_hi, rec_off, seq, seq_len};
    mrg::write_precursors(a, written);
    return MRG_OK;
  });
}

// ------------------------------------------- predict mode: screening the folded candidates (csrc/predict_screen.hip)
namespace {
constexpr uint64_t kScreenMaxLines = (1ull << 28) - 1, kScreenMaxItems = (1ull << 31) - 1;
// the screen calls' scratch: the stat words, the slices' lengths [n_cand + 1] and the scan's own
struct ScreenScratch {
  Piece<uint32_t> stat, len32;
  Piece<char> scan;
  size_t total;
  explicit ScreenScratch(uint64_t n_cand) {
    Carver c(8);
    stat = c.take<uint32_t>(mrg::kScreenStatWords);
    len32 = c.take<uint32_t>(n_cand + 1);
    scan = c.take<char>(mrg::prims::scan_temp_bytes(n_cand + 1));
    total = c.total();
  }
};
int screen_scratch_ok(const char* fn, void* d_tmp, uint64_t tmp_bytes, uint64_t n_cand) {
  if (!d_tmp || tmp_bytes < ScreenScratch(n_cand).total || ((uintptr_t)d_tmp & 7))
    return fail(MRG_ERR_ARG, "%s: scratch smaller than mrg_predict_screen_temp_bytes, unaligned or null", fn);
  return MRG_OK;
}
// the first candidate of a state, for the message (n > 0)
int screen_first_of(const uint8_t* d_state, size_t stride, uint64_t n, uint8_t what, hipStream_t st, uint64_t* first) {
  std::vector<uint8_t> h((size_t)n * stride);
  HIP_TRY(hipMemcpyAsync(h.data(), d_state, h.size(), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  *first = n;
  for (uint64_t i = 0; i < n; ++i)
    if (h[(size_t)i * stride] == what) {
      *first = i;
      break;
    }
  return MRG_OK;
}
int screen_read_stat(const uint32_t* stat, uint32_t* h_stat, hipStream_t st) { return read_stat(stat, h_stat, mrg::kScreenStatWords, st); }
}  // namespace

int mrg_predict_screen_temp_bytes(uint64_t n_cand, uint64_t* bytes) {
  const char* fn = "mrg_predict_screen_temp_bytes";
  if (!bytes) return fail(MRG_ERR_ARG, "%s: null argument", fn);
  if (n_cand > 4 * kScreenMaxLines) return fail(MRG_ERR_ARG, "%s: %llu candidates; the limit is 2^30 - 4", fn, (unsigned long long)n_cand);
  *bytes = ScreenScratch(n_cand).total;
  return MRG_OK;
}

int mrg_predict_screen_candidates(mrg_ctx* ctx, uint64_t n_lines, const uint32_t* d_line_group, uint64_t n_groups, const uint8_t* d_nb_flags,
                                  const int64_t* d_nb_up, const int64_t* d_nb_down, uint8_t* d_cand_n, uint32_t* d_cand_rec,
                                  uint32_t* d_cand_mir, void* d_tmp, uint64_t tmp_bytes, void* stream) {
  const char* fn = "mrg_predict_screen_candidates";
  if (!ctx) return fail(MRG_ERR_ARG, "%s: null argument", fn);
  if (n_lines > kScreenMaxLines || n_groups > kScreenMaxItems)
    return fail(MRG_ERR_ARG, "%s: lines are limited to 2^28 - 1, groups to 2^31 - 1", fn);
  if (int rc = screen_scratch_ok(fn, d_tmp, tmp_bytes, 0)) return rc;
  if (n_lines == 0) return MRG_OK;
  if (!d_line_group || !d_nb_flags || !d_nb_up || !d_nb_down || !d_cand_n || !d_cand_rec || !d_cand_mir) return fail(MRG_ERR_ARG, "%s: null arrays", fn);
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  uint32_t* stat = reinterpret_cast<uint32_t*>(d_tmp);
  HIP_TRY(hipMemsetAsync(stat, 0, mrg::kScreenStatWords * sizeof(uint32_t), st));
  HIP_TRY(mrg::screen_candidates_launch((uint32_t)n_lines, d_line_group, (uint32_t)n_groups, d_nb_flags, d_nb_up, d_nb_down, d_cand_n, d_cand_rec,
                                        d_cand_mir, stat, st));
  uint32_t h_stat[mrg::kScreenStatWords] = {0};
  if (int rc = screen_read_stat(stat, h_stat, st)) return rc;
  if (h_stat[mrg::kScreenStatBadGroup]) return fail(MRG_ERR_ARG, "%s: a line names no group", fn);
  if (h_stat[mrg::kScreenStatBadLine]) {
    uint64_t first = 0;
    if (int rc = screen_first_of(d_cand_n, 1, n_lines, 0, st, &first)) return rc;
    return fail(MRG_ERR_ARG, "%s: line %llu is Good, but its distances name no neighbour, or one before the first or behind the last line "
                "(the reference dies of an IndexError there)", fn, (unsigned long long)first);
  }
  return MRG_OK;
}

int mrg_predict_screen_prune(mrg_ctx* ctx, uint64_t n_cand, const uint32_t* d_cand_rec, const uint32_t* d_cand_mir, uint64_t n_rec,
                             const uint64_t* d_rec_off, const char* d_seq, const char* d_str, uint64_t seq_len, uint64_t n_mir,
                             const uint64_t* d_mir_off, const char* d_mir, uint64_t mir_len, int32_t pruned_length, uint8_t* d_status,
                             uint32_t* d_lo, uint32_t* d_hi, uint64_t* d_pruned_off, char* d_pruned, uint64_t pruned_cap, uint64_t* pruned_len,
                             void* d_tmp, uint64_t tmp_bytes, void* stream) {
  const char* fn = "mrg_predict_screen_prune";
  if (!ctx || !pruned_len) return fail(MRG_ERR_ARG, "%s: null argument", fn);
  *pruned_len = 0;
  if (n_cand > 4 * kScreenMaxLines || n_rec > kScreenMaxItems || n_mir > kScreenMaxItems)
    return fail(MRG_ERR_ARG, "%s: candidates are limited to 2^30 - 4, records and miRNAs to 2^31 - 1", fn);
  if (pruned_length < 0 || pruned_length > 1000) return fail(MRG_ERR_ARG, "%s: a pruned length of %d", fn, pruned_length);
  if (int rc = screen_scratch_ok(fn, d_tmp, tmp_bytes, n_cand)) return rc;
  if (!d_rec_off || !d_mir_off || !d_pruned_off) return fail(MRG_ERR_ARG, "%s: null offsets", fn);
  if ((seq_len && (!d_seq || !d_str)) || (mir_len && !d_mir)) return fail(MRG_ERR_ARG, "%s: null text", fn);
  if (n_cand && (!d_cand_rec || !d_cand_mir || !d_status || !d_lo || !d_hi)) return fail(MRG_ERR_ARG, "%s: null arrays", fn);
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  const ScreenScratch sc(n_cand);
  uint32_t *stat = sc.stat.at(d_tmp), *len32 = sc.len32.at(d_tmp);
  const mrg::ScreenBlob rec{(uint32_t)n_rec, d_rec_off, d_seq, d_str, seq_len}, mir{(uint32_t)n_mir, d_mir_off, d_mir, nullptr, mir_len};
  HIP_TRY(hipMemsetAsync(stat, 0, mrg::kScreenStatWords * sizeof(uint32_t), st));
  HIP_TRY(hipMemsetAsync(len32 + n_cand, 0, sizeof(uint32_t), st));
  HIP_TRY(mrg::screen_check_offsets_launch(rec, stat, st));
  HIP_TRY(mrg::screen_check_offsets_launch(mir, stat, st));
  HIP_TRY(mrg::screen_check_cands_launch((uint32_t)n_cand, d_cand_rec, nullptr, d_cand_mir, (uint32_t)n_rec, (uint32_t)n_mir, stat, st));
  uint32_t h_stat[mrg::kScreenStatWords] = {0};
  if (int rc = screen_read_stat(stat, h_stat, st)) return rc;   // (before a byte is read through them: the kernels trust the arrays)
  if (h_stat[mrg::kScreenStatBadOffsets]) return fail(MRG_ERR_ARG, "%s: offsets that do not ascend from 0 to the length of their text", fn);
  if (h_stat[mrg::kScreenStatBadCand]) return fail(MRG_ERR_ARG, "%s: a candidate names no record or no miRNA", fn);
  HIP_TRY(mrg::screen_prune_launch((uint32_t)n_cand, d_cand_rec, d_cand_mir, rec, mir, pruned_length, d_status, d_lo, d_hi, len32, stat, st));
  HIP_TRY(mrg::prims::exclusive_sum_u32_to_u64(len32, d_pruned_off, n_cand + 1, sc.scan.at(d_tmp), st));
  uint64_t total = 0;
  HIP_TRY(hipMemcpyAsync(&total, d_pruned_off + n_cand, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  if (int rc = screen_read_stat(stat, h_stat, st)) return rc;
  if (h_stat[mrg::kScreenStatRefused]) {
    uint64_t first = 0;
    if (int rc = screen_first_of(d_status, 1, n_cand, mrg::kScreenRefused, st, &first)) return rc;
    return fail(MRG_ERR_ARG, "%s: candidate %llu: a structure whose brackets do not balance, or an absent miRNA longer than the sequence "
                "(the reference dies of an IndexError there)", fn, (unsigned long long)first);
  }
  if (total > pruned_cap || (total && !d_pruned))
    return fail(MRG_ERR_ARG, "%s: %llu pruned bytes, room for %llu", fn, (unsigned long long)total, (unsigned long long)pruned_cap);
  HIP_TRY(mrg::screen_copy_launch((uint32_t)n_cand, d_cand_rec, rec, d_status, d_lo, d_hi, d_pruned_off, d_pruned, st));
  HIP_TRY(hipStreamSynchronize(st));
  *pruned_len = total;
  return MRG_OK;
}

int mrg_predict_screen_features(mrg_ctx* ctx, uint64_t n_cand, const uint8_t* d_status, const uint32_t* d_cand_mir, const uint64_t* d_p_off,
                                const char* d_p_seq, const char* d_p_str, uint64_t p_len, uint64_t n_mir, const uint64_t* d_mir_off,
                                const char* d_mir, uint64_t mir_len, int32_t* d_feat, void* d_tmp, uint64_t tmp_bytes, void* stream) {
  const char* fn = "mrg_predict_screen_features";
  if (!ctx) return fail(MRG_ERR_ARG, "%s: null argument", fn);
  if (n_cand > 4 * kScreenMaxLines || n_mir > kScreenMaxItems) return fail(MRG_ERR_ARG, "%s: candidates are limited to 2^30 - 4, miRNAs to 2^31 - 1", fn);
  if (int rc = screen_scratch_ok(fn, d_tmp, tmp_bytes, n_cand)) return rc;
  if (!d_p_off || !d_mir_off) return fail(MRG_ERR_ARG, "%s: null offsets", fn);
  if ((p_len && (!d_p_seq || !d_p_str)) || (mir_len && !d_mir)) return fail(MRG_ERR_ARG, "%s: null text", fn);
  if (n_cand && (!d_status || !d_cand_mir || !d_feat)) return fail(MRG_ERR_ARG, "%s: null arrays", fn);
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  uint32_t* stat = reinterpret_cast<uint32_t*>(d_tmp);
  const mrg::ScreenBlob text{(uint32_t)n_cand, d_p_off, d_p_seq, d_p_str, p_len}, mir{(uint32_t)n_mir, d_mir_off, d_mir, nullptr, mir_len};
  HIP_TRY(hipMemsetAsync(stat, 0, mrg::kScreenStatWords * sizeof(uint32_t), st));
  HIP_TRY(mrg::screen_check_offsets_launch(text, stat, st));
  HIP_TRY(mrg::screen_check_offsets_launch(mir, stat, st));
  HIP_TRY(mrg::screen_check_cands_launch((uint32_t)n_cand, nullptr, d_status, d_cand_mir, 0u, (uint32_t)n_mir, stat, st));
  uint32_t h_stat[mrg::kScreenStatWords] = {0};
  if (int rc = screen_read_stat(stat, h_stat, st)) return rc;
  if (h_stat[mrg::kScreenStatBadOffsets]) return fail(MRG_ERR_ARG, "%s: offsets that do not ascend from 0 to the length of their text", fn);
  if (h_stat[mrg::kScreenStatBadCand]) return fail(MRG_ERR_ARG, "%s: a candidate names no miRNA", fn);
  HIP_TRY(mrg::screen_features_launch((uint32_t)n_cand, d_status, d_cand_mir, text, mir, d_feat, stat, st));
  if (int rc = screen_read_stat(stat, h_stat, st)) return rc;
  if (h_stat[mrg::kScreenStatRefused]) {
    uint64_t first = 0;
    if (int rc = screen_first_of(reinterpret_cast<const uint8_t*>(d_feat), mrg::kScreenFeatWords * sizeof(int32_t), n_cand, mrg::kScreenRefused, st,
                                 &first))
      return rc;
    return fail(MRG_ERR_ARG, "%s: record %llu of the pruned structures: brackets that do not balance, or a hairpin loop under 3", fn,
                (unsigned long long)first);
  }
  return MRG_OK;
}

int mrg_predict_screen_select(mrg_ctx* ctx, uint64_t n_lines, const uint8_t* d_cand_n, const uint32_t* d_cand_rec, uint64_t n_rec,
                              const double* d_rec_mfe, const int32_t* d_feat, int32_t threshold, int32_t* d_best, void* d_tmp,
                              uint64_t tmp_bytes, void* stream) {
  const char* fn = "mrg_predict_screen_select";
  if (!ctx) return fail(MRG_ERR_ARG, "%s: null argument", fn);
  if (n_lines > kScreenMaxLines || n_rec > kScreenMaxItems) return fail(MRG_ERR_ARG, "%s: lines are limited to 2^28 - 1, records to 2^31 - 1", fn);
  if (int rc = screen_scratch_ok(fn, d_tmp, tmp_bytes, 0)) return rc;
  if (n_lines == 0) return MRG_OK;
  if (n_rec != 2 * n_lines) return fail(MRG_ERR_ARG, "%s: %llu records for %llu lines; every line has two", fn, (unsigned long long)n_rec, (unsigned long long)n_lines);
  if (!d_cand_n || !d_cand_rec || !d_rec_mfe || !d_feat || !d_best) return fail(MRG_ERR_ARG, "%s: null arrays", fn);
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  uint32_t* stat = reinterpret_cast<uint32_t*>(d_tmp);
  HIP_TRY(hipMemsetAsync(stat, 0, mrg::kScreenStatWords * sizeof(uint32_t), st));
  HIP_TRY(mrg::screen_select_launch((uint32_t)n_lines, d_cand_n, d_cand_rec, (uint32_t)n_rec, d_rec_mfe, d_feat, threshold, d_best, stat, st));
  uint32_t h_stat[mrg::kScreenStatWords] = {0};
  if (int rc = screen_read_stat(stat, h_stat, st)) return rc;
  if (h_stat[mrg::kScreenStatBadLine]) return fail(MRG_ERR_ARG, "%s: a line with neither two nor four candidates", fn);
  if (h_stat[mrg::kScreenStatBadCand])
    return fail(MRG_ERR_ARG, "%s: a candidate of no record, or a feature row left to the host and not filled in", fn);
  return MRG_OK;
}

int mrg_read_str_file(const char* path, uint64_t expected, uint64_t* n_rec, uint64_t* text_len, void** handle) {
  const char* fn = "mrg_read_str_file";
  if (!path || !n_rec || !text_len || !handle) return fail(MRG_ERR_ARG, "%s: null argument", fn);
  *handle = nullptr;
  *n_rec = *text_len = 0;
  return guarded(fn, [&] {
    std::unique_ptr<mrg::StrRecords> r(new mrg::StrRecords);
    mrg::read_str_file(path, expected, r.get());
    *n_rec = r->mfe.size();
    *text_len = r->seq.size();
    *handle = r.release();
    return MRG_OK;
  });
}

int mrg_str_file_copy(void* handle, uint64_t* off, char* seq, char* structure, double* mfe) {
  const char* fn = "mrg_str_file_copy";
  if (!handle || !off || !mfe) return fail(MRG_ERR_ARG, "%s: null argument", fn);
  const mrg::StrRecords* r = static_cast<const mrg::StrRecords*>(handle);
  if (r->seq.size() && (!seq || !structure)) return fail(MRG_ERR_ARG, "%s: null text buffers", fn);
  std::memcpy(off, r->off.data(), r->off.size() * sizeof(uint64_t));
  if (r->seq.size()) {
    std::memcpy(seq, r->seq.data(), r->seq.size());
    std::memcpy(structure, r->structure.data(), r->structure.size());
  }
  if (r->mfe.size()) std::memcpy(mfe, r->mfe.data(), r->mfe.size() * sizeof(double));
  return MRG_OK;
}

void mrg_str_file_free(void* handle) { delete static_cast<mrg::StrRecords*>(handle); }

int mrg_write_pruned_fasta(const char* path, uint64_t n, const uint64_t* off, const char* seq, const uint8_t* keep, uint64_t* written) {
  const char* fn = "mrg_write_pruned_fasta";
  if (!path || !off || !written || (n && !keep)) return fail(MRG_ERR_ARG, "%s: null argument", fn);
  *written = 0;
  return guarded(fn, [&] {
    *written = mrg::write_pruned_fasta(path, n, off, seq, keep);
    return MRG_OK;
  });
}

int mrg_write_screened_features(const char* features_path, const char* out_path, uint64_t n_lines, const int32_t* best, const int32_t* feat,
                                const uint64_t* p_off, const char* p_seq, const char* p_str, const double* p_mfe, uint64_t* written) {
  const char* fn = "mrg_write_screened_features";
  if (!features_path || !out_path || !written || !p_off) return fail(MRG_ERR_ARG, "%s: null argument", fn);
  *written = 0;
  if (n_lines && (!best || !feat || !p_mfe)) return fail(MRG_ERR_ARG, "%s: null arrays", fn);
  return guarded(fn, [&] {
    const mrg::ScreenWriteArgs a{features_path, out_path, n_lines, best, feat, p_off, p_seq, p_str, p_mfe};
    *written = mrg::write_screened_features(a);
    return MRG_OK;
  });
}

// ------------------------------------------- predict mode: the SVM (csrc/predict_svm.hip, csrc/predict_model_write.cpp)
int mrg_predict_model_filter(const char* table_path, const char* dataset_path, const char* refined_tmp_path, const char* refined_path,
                             const char* namelist, const char* features, uint32_t nf, uint64_t* counts, void** handle) {
  const char* fn = "mrg_predict_model_filter";
  if (!table_path || !dataset_path || !refined_tmp_path || !refined_path || !namelist || !features || !counts || !handle)
    return fail(MRG_ERR_ARG, "%s: null argument", fn);
  *handle = nullptr;
  counts[0] = counts[1] = counts[2] = counts[3] = 0;
  return guarded(fn, [&] {
    std::unique_ptr<mrg::ModelTable> t(new mrg::ModelTable);
    const mrg::ModelFilterArgs a{table_path, dataset_path, refined_tmp_path, refined_path, namelist, features};
    mrg::filter_model_table(a, t.get());
    if (t->nf != nf) return fail(MRG_ERR_ARG, "%s: %u selected names for nf = %u", fn, t->nf, nf);
    counts[0] = t->n_table;
    counts[1] = t->n_dataset;
    counts[2] = t->n_refined;
    counts[3] = t->n_stray;
    *handle = t.release();
    return MRG_OK;
  });
}

int mrg_predict_model_rows(void* handle, double* x) {
  const char* fn = "mrg_predict_model_rows";
  if (!handle) return fail(MRG_ERR_ARG, "%s: null argument", fn);
  const mrg::ModelTable* t = static_cast<const mrg::ModelTable*>(handle);
  if (t->x.size() && !x) return fail(MRG_ERR_ARG, "%s: null buffer", fn);
  if (t->x.size()) std::memcpy(x, t->x.data(), t->x.size() * sizeof(double));
  return MRG_OK;
}

int mrg_predict_svm(mrg_ctx* ctx, uint64_t n_rows, const double* d_x, uint32_t nf, const double* d_mean, const double* d_scale,
                    const double* d_sv, const double* d_coef, uint64_t n_sv, double intercept, double gamma, double prob_a, double prob_b,
                    int8_t* d_pred, double* d_dec, double* d_prob, void* stream) {
  const char* fn = "mrg_predict_svm";
  if (!ctx) return fail(MRG_ERR_ARG, "%s: null argument", fn);
  if (nf < 1 || nf > mrg::kSvmMaxFeatures) return fail(MRG_ERR_ARG, "%s: nf = %u; 1 to %u features are taken", fn, nf, mrg::kSvmMaxFeatures);
  if (n_sv < 1 || n_sv > 0x7fffffffull / nf) return fail(MRG_ERR_ARG, "%s: n_sv = %llu; at least one, and n_sv nf below 2^31", fn, (unsigned long long)n_sv);
  if (n_rows > 0x7fffffffull / nf) return fail(MRG_ERR_ARG, "%s: n_rows = %llu; n_rows nf must stay below 2^31", fn, (unsigned long long)n_rows);
  if (!(gamma > 0.0) || !std::isfinite(gamma) || !std::isfinite(intercept) || !std::isfinite(prob_a) || !std::isfinite(prob_b))
    return fail(MRG_ERR_ARG, "%s: gamma must be positive, and gamma, intercept, prob_a and prob_b finite", fn);
  if (n_rows == 0) return MRG_OK;
  if (!d_x || !d_mean || !d_scale || !d_sv || !d_coef || !d_pred || !d_dec || !d_prob) return fail(MRG_ERR_ARG, "%s: null arrays", fn);
  HIP_TRY(hipSetDevice(ctx->device));
  const mrg::SvmModelDev m{nf, (uint32_t)n_sv, d_mean, d_scale, d_sv, d_coef, intercept, gamma, prob_a, prob_b};
  HIP_TRY(mrg::predict_svm_launch(n_rows, d_x, m, d_pred, d_dec, d_prob, (hipStream_t)stream));
  return MRG_OK;
}

int mrg_predict_model_write(void* handle, const int8_t* pred, const double* prob, const char* detailed_path, const char* novel_path,
                            uint64_t* predicted, uint64_t* kept) {
  const char* fn = "mrg_predict_model_write";
  if (!handle || !detailed_path || !novel_path || !predicted || !kept) return fail(MRG_ERR_ARG, "%s: null argument", fn);
  const mrg::ModelTable* t = static_cast<const mrg::ModelTable*>(handle);
  *predicted = *kept = 0;
  if (t->n_refined && (!pred || !prob)) return fail(MRG_ERR_ARG, "%s: null arrays", fn);
  return guarded(fn, [&] {
    mrg::write_model_results(*t, pred, prob, detailed_path, novel_path, predicted, kept);
    return MRG_OK;
  });
}

void mrg_predict_model_free(void* handle) { delete static_cast<mrg::ModelTable*>(handle); }

int mrg_format_repr(double v, char* buf, uint32_t cap) {
  const char* fn = "mrg_format_repr";
  if (!buf) return fail(MRG_ERR_ARG, "%s: null argument", fn);
  std::string s;
  mrg::append_repr(s, v);
  if (s.size() + 1 > cap) return fail(MRG_ERR_ARG, "%s: %zu characters do not fit", fn, s.size());
  std::memcpy(buf, s.c_str(), s.size() + 1);
  return MRG_OK;
}

// ------------------------------------------- predict mode: the report (csrc/predict_report.hip, csrc/predict_report_write.cpp)
namespace {
constexpr uint64_t kReportMaxLines = (1ull << 28) - 1;
// the entry pass's scratch: the entry count, two sorts' buffer pairs, the chunks' columns, the sizes the offsets are summed from
struct ReportScratch {
  Piece<uint32_t> stat, key0, key1, val0, val1, ckey0, ckey1, cval0, cval1, cm, emit, num, rows32, len32;
  Piece<int32_t> cp;
  Piece<char> sort, scan;
  size_t total;
  explicit ReportScratch(uint64_t n) {
    Carver c(8);
    stat = c.take<uint32_t>(2);
    for (Piece<uint32_t>* p : {&key0, &key1, &val0, &val1, &ckey0, &ckey1, &cval0, &cval1, &cm, &emit, &num}) *p = c.take<uint32_t>(n);
    rows32 = c.take<uint32_t>(n + 1);
    len32 = c.take<uint32_t>(n + 1);
    cp = c.take<int32_t>(n);
    sort = c.take<char>(mrg::prims::radix_temp_bytes(n));
    scan = c.take<char>(mrg::prims::scan_temp_bytes(n + 1));
    total = c.total();
  }
};
}  // namespace

int mrg_predict_report_read(const char* novel_path, const char* table_path, const char* cluster_path, uint64_t* counts, void** handle) {
  const char* fn = "mrg_predict_report_read";
  if (!novel_path || !table_path || !cluster_path || !counts || !handle) return fail(MRG_ERR_ARG, "%s: null argument", fn);
  *handle = nullptr;
  counts[0] = counts[1] = counts[2] = 0;
  return guarded(fn, [&] {
    std::unique_ptr<mrg::ReportTable> t(new mrg::ReportTable);
    mrg::read_report_inputs(novel_path, table_path, cluster_path, t.get());
    counts[0] = t->n;
    counts[1] = t->n_listed;
    counts[2] = t->n_rows;
    *handle = t.release();
    return MRG_OK;
  });
}

int mrg_predict_report_array(void* handle, uint32_t which, const void** data, uint64_t* bytes) {
  const char* fn = "mrg_predict_report_array";
  if (!handle || !data || !bytes) return fail(MRG_ERR_ARG, "%s: null argument", fn);
  const mrg::ReportTable* t = static_cast<const mrg::ReportTable*>(handle);
  auto give = [&](const auto& v) {
    *data = v.data();
    *bytes = v.size() * sizeof(v[0]);
    return MRG_OK;
  };
  switch (which) {
    case MRG_REPORT_FLAGS: return give(t->flags);
    case MRG_REPORT_RANK: return give(t->rank);
    case MRG_REPORT_UP: return give(t->up);
    case MRG_REPORT_DOWN: return give(t->down);
    case MRG_REPORT_POS: return give(t->pos);
    case MRG_REPORT_ADJ: return give(t->adj);
    case MRG_REPORT_READS: return give(t->reads);
    case MRG_REPORT_GID3: return give(t->gid3);
    case MRG_REPORT_T_OFF: return give(t->t_off);
    case MRG_REPORT_TEXT: return give(t->text);
    case MRG_REPORT_BLK: return give(t->blk);
    case MRG_REPORT_R_OFF: return give(t->r_off);
    case MRG_REPORT_ROW_START: return give(t->row_start);
    case MRG_REPORT_ROW_END: return give(t->row_end);
    case MRG_REPORT_ROW_COUNT: return give(t->row_count);
    case MRG_REPORT_ROW_SOFF: return give(t->row_soff);
    case MRG_REPORT_ROW_TEXT: return give(t->row_text);
  }
  return fail(MRG_ERR_ARG, "%s: no array %u", fn, which);
}

int mrg_predict_report_temp_bytes(uint64_t n_lines, uint64_t* bytes) {
  const char* fn = "mrg_predict_report_temp_bytes";
  if (!bytes) return fail(MRG_ERR_ARG, "%s: null argument", fn);
  if (n_lines > kReportMaxLines) return fail(MRG_ERR_ARG, "%s: %llu lines; the limit is 2^28 - 1", fn, (unsigned long long)n_lines);
  *bytes = ReportScratch(n_lines).total;
  return MRG_OK;
}

int mrg_predict_report_correct(mrg_ctx* ctx, uint64_t n_lines, const uint8_t* d_flags, const int64_t* d_up, const int64_t* d_down,
                               const int64_t* d_pos, const int32_t* d_adj, const uint32_t* d_gid3, const uint64_t* d_t_off, const char* d_text,
                               uint64_t text_len, uint32_t* d_src, uint8_t* d_state, uint8_t* d_err, int64_t* d_pos_adj, int32_t* d_stable_idx,
                               uint32_t* d_gid, void* stream) {
  const char* fn = "mrg_predict_report_correct";
  if (!ctx) return fail(MRG_ERR_ARG, "%s: null argument", fn);
  if (n_lines > kReportMaxLines) return fail(MRG_ERR_ARG, "%s: %llu lines; the limit is 2^28 - 1", fn, (unsigned long long)n_lines);
  if (n_lines == 0) return MRG_OK;
  if (!d_flags || !d_up || !d_down || !d_pos || !d_adj || !d_gid3 || !d_t_off || (text_len && !d_text) || !d_src || !d_state || !d_err ||
      !d_pos_adj || !d_stable_idx || !d_gid)
    return fail(MRG_ERR_ARG, "%s: null arrays", fn);
  HIP_TRY(hipSetDevice(ctx->device));
  const mrg::ReportLines in{(uint32_t)n_lines, d_flags, nullptr, d_up, d_down, d_pos, d_adj, nullptr, d_gid3, d_t_off, d_text, text_len};
  const mrg::ReportLineOut out{d_src, d_state, d_err, d_pos_adj, d_stable_idx, d_gid};
  HIP_TRY(mrg::report_correct_launch(in, out, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  return MRG_OK;
}

int mrg_predict_report_entries(mrg_ctx* ctx, uint64_t n_lines, const uint8_t* d_flags, const uint32_t* d_rank, const int64_t* d_reads,
                               const uint64_t* d_t_off, const uint32_t* d_src, const uint8_t* d_state, const int32_t* d_stable_idx,
                               const uint32_t* d_gid, const uint8_t* d_blk, const uint64_t* d_r_off, uint32_t* d_ent_m, int32_t* d_ent_p,
                               uint8_t* d_chunk_err, uint32_t* d_chunk_line, uint64_t* d_row_off, uint64_t* d_prof_off, uint64_t* totals,
                               void* d_tmp, uint64_t tmp_bytes, void* stream) {
  const char* fn = "mrg_predict_report_entries";
  if (!ctx || !totals) return fail(MRG_ERR_ARG, "%s: null argument", fn);
  totals[0] = totals[1] = totals[2] = 0;
  if (n_lines > kReportMaxLines) return fail(MRG_ERR_ARG, "%s: %llu lines; the limit is 2^28 - 1", fn, (unsigned long long)n_lines);
  const ReportScratch sc(n_lines);
  if (!d_tmp) return fail(MRG_ERR_ARG, "%s: null scratch", fn);
  if (int rc = scratch_ok(fn, d_tmp, tmp_bytes, sc.total, "mrg_predict_report_temp_bytes")) return rc;
  if (!d_row_off || !d_prof_off || !d_r_off) return fail(MRG_ERR_ARG, "%s: null offsets", fn);
  if (n_lines && (!d_flags || !d_rank || !d_reads || !d_t_off || !d_src || !d_state || !d_stable_idx || !d_gid || !d_blk || !d_ent_m || !d_ent_p ||
                  !d_chunk_err || !d_chunk_line))
    return fail(MRG_ERR_ARG, "%s: null arrays", fn);
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  const mrg::ReportLines in{(uint32_t)n_lines, d_flags, d_rank, nullptr, nullptr, nullptr, nullptr, d_reads, nullptr, d_t_off, nullptr, 0};
  const mrg::ReportLineOut lines{const_cast<uint32_t*>(d_src), const_cast<uint8_t*>(d_state), nullptr, nullptr, const_cast<int32_t*>(d_stable_idx),
                                 const_cast<uint32_t*>(d_gid)};
  const mrg::ReportEntryScratch es{sc.key0.at(d_tmp), sc.key1.at(d_tmp), sc.val0.at(d_tmp), sc.val1.at(d_tmp), sc.ckey0.at(d_tmp), sc.ckey1.at(d_tmp),
                                   sc.cval0.at(d_tmp), sc.cval1.at(d_tmp), sc.cm.at(d_tmp), sc.emit.at(d_tmp), sc.num.at(d_tmp), sc.rows32.at(d_tmp),
                                   sc.len32.at(d_tmp), sc.cp.at(d_tmp), sc.sort.at(d_tmp), sc.scan.at(d_tmp)};
  const mrg::ReportEntryOut out{d_ent_m, d_ent_p, d_chunk_err, d_chunk_line, d_row_off, d_prof_off, sc.stat.at(d_tmp)};
  HIP_TRY(mrg::report_entries_launch(in, lines, d_blk, d_r_off, es, out, st));
  uint32_t n_entries = 0;
  uint64_t sums[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(&n_entries, sc.stat.at(d_tmp), sizeof n_entries, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(&sums[0], d_row_off + n_lines, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(&sums[1], d_prof_off + n_lines, sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  totals[0] = n_entries;
  totals[1] = sums[0];
  totals[2] = sums[1];
  return MRG_OK;
}

int mrg_predict_report_profile(mrg_ctx* ctx, uint64_t n_lines, const uint8_t* d_flags, const uint64_t* d_t_off, const char* d_text, uint64_t text_len,
                               const uint32_t* d_src, const int64_t* d_pos_adj, const int32_t* d_stable_idx, const uint64_t* d_r_off,
                               uint64_t n_rows, const int64_t* d_row_start, const int64_t* d_row_end, const int64_t* d_row_count,
                               const uint64_t* d_row_soff, const char* d_row_text, uint64_t row_text_len, uint64_t n_entries,
                               const uint32_t* d_ent_m, const int32_t* d_ent_p, const uint64_t* d_row_off, const uint64_t* d_prof_off,
                               int32_t* d_lead, int32_t* d_trail, uint64_t* d_prof, uint64_t* d_total, uint8_t* d_flag, void* stream) {
  const char* fn = "mrg_predict_report_profile";
  if (!ctx) return fail(MRG_ERR_ARG, "%s: null argument", fn);
  if (n_lines > kReportMaxLines || n_entries > n_lines) return fail(MRG_ERR_ARG, "%s: lines are limited to 2^28 - 1, entries to the lines", fn);
  if (n_entries == 0) return MRG_OK;
  if (!d_flags || !d_t_off || (text_len && !d_text) || !d_src || !d_pos_adj || !d_stable_idx || !d_r_off || !d_row_soff || !d_ent_m || !d_ent_p ||
      !d_row_off || !d_prof_off || !d_total || !d_flag)
    return fail(MRG_ERR_ARG, "%s: null arrays", fn);
  if (n_rows && (!d_row_start || !d_row_end || !d_row_count || !d_lead || !d_trail || (row_text_len && !d_row_text)))
    return fail(MRG_ERR_ARG, "%s: null row arrays", fn);
  HIP_TRY(hipSetDevice(ctx->device));
  const mrg::ReportLines in{(uint32_t)n_lines, d_flags, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, d_t_off, d_text, text_len};
  const mrg::ReportLineOut lines{const_cast<uint32_t*>(d_src), nullptr, nullptr, const_cast<int64_t*>(d_pos_adj), const_cast<int32_t*>(d_stable_idx), nullptr};
  const mrg::ReportRows rows{nullptr, d_r_off, n_rows, d_row_start, d_row_end, d_row_count, d_row_soff, d_row_text, row_text_len};
  const mrg::ReportProfileOut out{d_lead, d_trail, d_prof, d_total, d_flag};
  HIP_TRY(mrg::report_profile_launch(in, lines, rows, (uint32_t)n_entries, d_ent_m, d_ent_p, d_row_off, d_prof_off, out, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  return MRG_OK;
}

int mrg_predict_report_write(void* handle, const uint32_t* src, const uint8_t* state, const int64_t* pos_adj, uint64_t n_entries,
                             const uint32_t* ent_m, const int32_t* ent_p, const uint64_t* row_off, const int32_t* lead, const int32_t* trail,
                             const uint64_t* prof_off, const uint64_t* prof, const uint64_t* total, const uint8_t* flag, const char* corrected_path,
                             const char* report_path, const char* profiles_path) {
  const char* fn = "mrg_predict_report_write";
  if (!handle || !corrected_path || !report_path || !profiles_path) return fail(MRG_ERR_ARG, "%s: null argument", fn);
  const mrg::ReportTable* t = static_cast<const mrg::ReportTable*>(handle);
  return guarded(fn, [&] {
    const mrg::ReportWriteArgs a{src, state, pos_adj, n_entries, ent_m, ent_p, row_off, lead, trail, prof_off, prof, total, flag,
                                 corrected_path, report_path, profiles_path};
    mrg::write_report(*t, a);
    return MRG_OK;
  });
}

void mrg_predict_report_free(void* handle) { delete static_cast<mrg::ReportTable*>(handle); }

// ----------------------------------------------------- host convenience
int mrg_annotate_host(mrg_ctx* ctx, const uint64_t* reads, uint32_t words_per_read,
                      const uint8_t* lens, const uint64_t* nmask, uint64_t n,
                      const mrg_pass_cfg* passes, uint32_t n_pass, int8_t* pass_id, int32_t* ref_id,
                      int32_t* pos, uint8_t* mm, mrg_pass_stats* stats, const uint32_t* quant,
                      uint32_t n_samples, uint32_t n_mirna, int32_t canon_pass, int32_t isomir_pass,
                      uint64_t* counts) {
  if (!ctx || !passes) return fail(MRG_ERR_ARG, "mrg_annotate_host: null argument");
  if (n && (!reads || !lens || !pass_id || !ref_id || !pos || !mm))
    return fail(MRG_ERR_ARG, "mrg_annotate_host: null read/output buffers");
  HIP_TRY(hipSetDevice(ctx->device));
  struct Bufs {
    std::vector<void*> v;
    ~Bufs() {
      for (void* p : v) (void)hipFree(p);
    }
    int get(void** p, size_t bytes) {
      hipError_t e = hipMalloc(p, bytes ? bytes : 16);
      if (e != hipSuccess) return fail(MRG_ERR_NOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
      v.push_back(*p);
      return MRG_OK;
    }
  } bufs;
  int rc;
  uint64_t *d_reads = nullptr, *d_nmask = nullptr, *d_counts = nullptr, *d_pc = nullptr;
  uint8_t *d_lens = nullptr, *d_mm = nullptr;
  int8_t* d_pass = nullptr;
  int32_t *d_ref = nullptr, *d_pos = nullptr;
  uint32_t* d_quant = nullptr;
  void* d_ws = nullptr;
  uint64_t ws_bytes = 0;
  mrg_cascade_workspace_bytes(n, &ws_bytes);
  const size_t rbytes = (size_t)n * words_per_read * 8;
  if ((rc = bufs.get((void**)&d_reads, rbytes))) return rc;
  if ((rc = bufs.get((void**)&d_lens, n))) return rc;
  if (nmask && (rc = bufs.get((void**)&d_nmask, rbytes))) return rc;
  if ((rc = bufs.get((void**)&d_pass, n))) return rc;
  if ((rc = bufs.get((void**)&d_ref, n * 4))) return rc;
  if ((rc = bufs.get((void**)&d_pos, n * 4))) return rc;
  if ((rc = bufs.get((void**)&d_mm, n))) return rc;
  if ((rc = bufs.get((void**)&d_pc, 2 * MRG_MAX_PASSES * 8))) return rc;
  if ((rc = bufs.get(&d_ws, ws_bytes))) return rc;
  if (n) {
    HIP_TRY(hipMemcpy(d_reads, reads, rbytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_lens, lens, n, hipMemcpyHostToDevice));
    if (nmask) HIP_TRY(hipMemcpy(d_nmask, nmask, rbytes, hipMemcpyHostToDevice));
  }
  {
    // the lengths are on the host here: give the cascade the exact range of this batch (and put
    // the caller's own hints back afterwards)
    uint8_t lo = 255, hi = 0;
    for (uint64_t r = 0; r < n; ++r) {
      lo = std::min(lo, lens[r]);
      hi = std::max(hi, lens[r]);
    }
    ctx->hint_min_len = n ? lo : 0;
    ctx->hint_max_len = n ? hi : 255;
    rc = mrg_cascade_run(ctx, d_reads, words_per_read, d_lens, d_nmask, n, passes, n_pass, d_pass, d_ref,
                         d_pos, d_mm, d_pc, d_ws, ws_bytes, nullptr);
  }
  if (rc) return rc;
  std::vector<mrg_pass_stats> st(n_pass);
  if ((rc = mrg_cascade_stats(ctx, st.data(), n_pass))) return rc;
  if (stats) std::memcpy(stats, st.data(), n_pass * sizeof(mrg_pass_stats));
  if (counts) {
    if (!quant || n_samples == 0) return fail(MRG_ERR_ARG, "mrg_annotate_host: counts requested without quant");
    uint64_t clen = 0;
    mrg_tally_counts_len(n_mirna, n_samples, n_pass, &clen);
    if ((rc = bufs.get((void**)&d_counts, clen * 8))) return rc;
    if ((rc = bufs.get((void**)&d_quant, n * n_samples * 4))) return rc;
    HIP_TRY(hipMemset(d_counts, 0, clen * 8));
    if (n) HIP_TRY(hipMemcpy(d_quant, quant, n * n_samples * 4, hipMemcpyHostToDevice));
    if ((rc = mrg_tally_run(ctx, d_pass, d_ref, d_quant, n, n_samples, n_mirna, n_pass, canon_pass,
                            isomir_pass, d_counts, nullptr)))
      return rc;
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(counts, d_counts, clen * 8, hipMemcpyDeviceToHost));
  }
  if (n) {
    HIP_TRY(hipMemcpy(pass_id, d_pass, n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(ref_id, d_ref, n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(pos, d_pos, n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(mm, d_mm, n, hipMemcpyDeviceToHost));
  }
  return MRG_OK;
}

// the long-read lane for a caller without a device allocator (the ctypes stub of INTEGRATION.md)
int mrg_annotate_long_host(mrg_ctx* ctx, const uint64_t* words, const uint64_t* nmask, const uint64_t* word_off, const uint32_t* lens,
                           uint64_t n, const mrg_pass_cfg* passes, uint32_t n_pass, int8_t* pass_id, int32_t* ref_id, int32_t* pos,
                           uint8_t* mm, mrg_pass_stats* stats) {
  if (!ctx || !passes) return fail(MRG_ERR_ARG, "mrg_annotate_long_host: null argument");
  if (n && (!words || !word_off || !lens || !pass_id || !ref_id || !pos || !mm))
    return fail(MRG_ERR_ARG, "mrg_annotate_long_host: null read/output buffers");
  if (n == 0) return MRG_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  struct Bufs {
    std::vector<void*> v;
    ~Bufs() {
      for (void* p : v) (void)hipFree(p);
    }
    int get(void** p, size_t bytes) {
      hipError_t e = hipMalloc(p, bytes ? bytes : 16);
      if (e != hipSuccess) return fail(MRG_ERR_NOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
      v.push_back(*p);
      return MRG_OK;
    }
  } bufs;
  const size_t wbytes = (size_t)word_off[n] * 8;
  uint64_t *d_words = nullptr, *d_nmask = nullptr, *d_off = nullptr;
  uint32_t* d_lens = nullptr;
  int8_t* d_pass = nullptr;
  int32_t *d_ref = nullptr, *d_pos = nullptr;
  uint8_t* d_mm = nullptr;
  int rc;
  if ((rc = bufs.get((void**)&d_words, wbytes))) return rc;
  if (nmask && (rc = bufs.get((void**)&d_nmask, wbytes))) return rc;
  if ((rc = bufs.get((void**)&d_off, (n + 1) * 8))) return rc;
  if ((rc = bufs.get((void**)&d_lens, n * 4))) return rc;
  if ((rc = bufs.get((void**)&d_pass, n))) return rc;
  if ((rc = bufs.get((void**)&d_ref, n * 4))) return rc;
  if ((rc = bufs.get((void**)&d_pos, n * 4))) return rc;
  if ((rc = bufs.get((void**)&d_mm, n))) return rc;
  if (wbytes) HIP_TRY(hipMemcpy(d_words, words, wbytes, hipMemcpyHostToDevice));
  if (nmask && wbytes) HIP_TRY(hipMemcpy(d_nmask, nmask, wbytes, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_off, word_off, (n + 1) * 8, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_lens, lens, n * 4, hipMemcpyHostToDevice));
  if ((rc = mrg_cascade_run_long(ctx, d_words, d_nmask, d_off, d_lens, n, passes, n_pass, d_pass, d_ref, d_pos, d_mm, nullptr, stats,
                                 nullptr)))
    return rc;
  HIP_TRY(hipMemcpy(pass_id, d_pass, n, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(ref_id, d_ref, n * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(pos, d_pos, n * 4, hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(mm, d_mm, n, hipMemcpyDeviceToHost));
  return MRG_OK;
}

// -------------------------------------------------------------- ingest
int mrg_adapter_locate(const char* adapter, const char* read, double max_error_rate, int32_t min_overlap,
                       int32_t* out6) {
  if (!adapter || !read || !out6) return fail(MRG_ERR_ARG, "mrg_adapter_locate: null argument");
  try {
    const mrg::AdapterMatch m =
        mrg::locate_adapter_3p(adapter, read, std::strlen(read), max_error_rate, min_overlap);
    out6[0] = m.found ? 1 : 0;
    out6[1] = (int32_t)m.read_start;
    out6[2] = (int32_t)m.read_stop;
    out6[3] = m.adapter_stop;
    out6[4] = m.matches;
    out6[5] = m.errors;
    return MRG_OK;
  } catch (const std::exception& e) {
    return fail(MRG_ERR_NOMEM, "mrg_adapter_locate: %s", e.what());
  }
}

int mrg_fastq_load(const char* path, int32_t qual_cutoff, int32_t min_len, const char* adapter, int32_t threads,
                   mrg_fastq** out) {
  if (!path || !out) return fail(MRG_ERR_ARG, "mrg_fastq_load: null argument");
  try {
    auto h = std::make_unique<mrg_fastq>();
    mrg::load_fastq(path, qual_cutoff, min_len, adapter, threads, h->d);
    *out = h.release();
    return MRG_OK;
  } catch (const std::bad_alloc&) {
    return fail(MRG_ERR_NOMEM, "mrg_fastq_load: out of memory");
  } catch (const std::exception& e) {
    return fail(MRG_ERR_IO, "mrg_fastq_load: %s", e.what());
  }
}

int mrg_fastq_load_part(const char* path, int32_t qual_cutoff, int32_t min_len, const char* adapter, int32_t threads, int32_t part,
                        int32_t n_parts, mrg_fastq** out) {
  if (!path || !out) return fail(MRG_ERR_ARG, "mrg_fastq_load_part: null argument");
  if (n_parts < 1 || part < 0 || part >= n_parts) return fail(MRG_ERR_ARG, "mrg_fastq_load_part: part %d of %d", part, n_parts);
  try {
    auto h = std::make_unique<mrg_fastq>();
    mrg::load_fastq(path, qual_cutoff, min_len, adapter, threads, h->d, part, n_parts);
    *out = h.release();
    return MRG_OK;
  } catch (const std::bad_alloc&) {
    return fail(MRG_ERR_NOMEM, "mrg_fastq_load_part: out of memory");
  } catch (const std::exception& e) {
    return fail(MRG_ERR_IO, "mrg_fastq_load_part: %s", e.what());
  }
}

int mrg_fastq_get_info(const mrg_fastq* fq, mrg_fastq_info* info) {
  if (!fq || !info) return fail(MRG_ERR_ARG, "mrg_fastq_get_info: null argument");
  info->n_total = fq->d.n_total;
  info->n_kept = fq->d.n_kept;
  info->phred = fq->d.phred;
  info->words_per_read = fq->d.words_per_read;
  info->max_len = fq->d.max_len;
  info->has_n = fq->d.has_n ? 1 : 0;
  info->n_long = fq->d.long_reads.size();
  return MRG_OK;
}

int mrg_fastq_long_read(const mrg_fastq* fq, uint64_t i, const char** seq) {
  if (!fq || !seq) return fail(MRG_ERR_ARG, "mrg_fastq_long_read: null argument");
  if (i >= fq->d.long_reads.size()) return fail(MRG_ERR_ARG, "mrg_fastq_long_read: index out of range");
  *seq = fq->d.long_reads[i].c_str();
  return MRG_OK;
}

int mrg_fastq_copy(const mrg_fastq* fq, uint32_t words_per_read, uint64_t* words, uint8_t* lens,
                   uint64_t* nmask) {
  if (!fq || (fq->d.n_kept && (!words || !lens))) return fail(MRG_ERR_ARG, "mrg_fastq_copy: null argument");
  const mrg::FastqData& d = fq->d;
  if (words_per_read < d.words_per_read || words_per_read > MRG_MAX_WORDS)
    return fail(MRG_ERR_ARG, "mrg_fastq_copy: words_per_read %u, file needs %u", words_per_read, d.words_per_read);
  if (d.has_n && !nmask) return fail(MRG_ERR_ARG, "mrg_fastq_copy: the file has N bases, nmask is required");
  const size_t n = d.n_kept;
  for (uint32_t w = 0; w < words_per_read; ++w) {
    if (w < d.words_per_read) {
      std::memcpy(words + (size_t)w * n, d.words.data() + (size_t)w * n, n * 8);
      if (nmask) std::memcpy(nmask + (size_t)w * n, d.nmask.data() + (size_t)w * n, n * 8);
    } else {
      std::memset(words + (size_t)w * n, 0, n * 8);
      if (nmask) std::memset(nmask + (size_t)w * n, 0, n * 8);
    }
  }
  if (n) std::memcpy(lens, d.lens.data(), n);
  return MRG_OK;
}

void mrg_fastq_free(mrg_fastq* fq) { delete fq; }

int mrg_gz_open(const char* path, int32_t threads, mrg_gz** out) {
  if (!path || !out) return fail(MRG_ERR_ARG, "mrg_gz_open: null argument");
  try {
    std::unique_ptr<mrg_gz> h(new mrg_gz());
    h->rd.reset(new mrg::GzipReader(path, threads));
    *out = h.release();
  } catch (const std::bad_alloc&) {
    return fail(MRG_ERR_NOMEM, "mrg_gz_open: out of memory");
  } catch (const std::exception& e) {
    return fail(MRG_ERR_IO, "mrg_gz_open: %s", e.what());
  }
  return MRG_OK;
}

int mrg_gz_read(mrg_gz* gz, void* buf, uint64_t len, uint64_t* got) {
  if (!gz || !got || (len && !buf)) return fail(MRG_ERR_ARG, "mrg_gz_read: null argument");
  try {
    *got = gz->rd->read(static_cast<char*>(buf), (size_t)len);
  } catch (const std::bad_alloc&) {
    return fail(MRG_ERR_NOMEM, "mrg_gz_read: out of memory");
  } catch (const std::exception& e) {
    return fail(MRG_ERR_IO, "mrg_gz_read: %s", e.what());
  }
  return MRG_OK;
}

int mrg_gz_info(const mrg_gz* gz, int32_t* parallel, uint64_t* merged) {
  if (!gz) return fail(MRG_ERR_ARG, "mrg_gz_info: null argument");
  if (parallel) *parallel = gz->rd->parallel() ? 1 : 0;
  if (merged) *merged = gz->rd->chunks_merged();
  return MRG_OK;
}

void mrg_gz_close(mrg_gz* gz) { delete gz; }

int mrg_fastq_block_cut(const char* buf, uint64_t len, int32_t at_eof, uint64_t* cut) {
  if (!buf || !cut) return fail(MRG_ERR_ARG, "mrg_fastq_block_cut: null argument");
  *cut = mrg::fastq_block_cut(buf, (size_t)len, at_eof != 0);
  return MRG_OK;
}

int mrg_fastq_parse_device(mrg_ctx* ctx, const char* d_text, uint64_t n_bytes, int32_t phred, int32_t qual_cutoff, int32_t min_len,
                           int32_t cut, uint32_t words_per_read, uint64_t cap, uint64_t* d_words, uint8_t* d_lens, uint64_t* d_nmask,
                           mrg_fastq_device_info* info, void* stream) {
  return mrg_fastq_parse_device_ad(ctx, d_text, n_bytes, phred, qual_cutoff, min_len, cut, nullptr, words_per_read, cap, d_words, d_lens,
                                   d_nmask, info, stream);
}

int mrg_fastq_parse_device_ad(mrg_ctx* ctx, const char* d_text, uint64_t n_bytes, int32_t phred, int32_t qual_cutoff, int32_t min_len,
                              int32_t cut, const char* adapters, uint32_t words_per_read, uint64_t cap, uint64_t* d_words,
                              uint8_t* d_lens, uint64_t* d_nmask, mrg_fastq_device_info* info, void* stream) {
  if (!ctx || !info) return fail(MRG_ERR_ARG, "mrg_fastq_parse_device: null argument");
  mrg::AdapterSet ads;
  std::memset(&ads, 0, sizeof ads);
  if (adapters && *adapters) {
    mrg::TrimSpec spec;
    try {
      spec = mrg::parse_trim_spec(adapters);
    } catch (const std::exception& e) {
      return fail(MRG_ERR_ARG, "mrg_fastq_parse_device_ad: %s", e.what());
    }
    if (spec.cut) return fail(MRG_ERR_ARG, "mrg_fastq_parse_device_ad: `+N` goes in `cut`, adapters takes sequences");
    if (spec.adapters.size() > mrg::kAdapterMax)
      return fail(MRG_ERR_ARG, "mrg_fastq_parse_device_ad: at most %u adapter sequences", mrg::kAdapterMax);
    for (const std::string& a : spec.adapters) {
      if (a.size() > mrg::kAdapterMaxLen)
        return fail(MRG_ERR_ARG, "mrg_fastq_parse_device_ad: adapters of at most %u bases", mrg::kAdapterMaxLen);
      const uint32_t q = ads.n++;
      ads.len[q] = (uint8_t)a.size();
      ads.k[q] = (uint8_t)(int)(0.12 * (double)a.size());
      std::memcpy(ads.seq[q], a.data(), a.size());
    }
  }
  if (n_bytes && (!d_text || !d_words || !d_lens)) return fail(MRG_ERR_ARG, "mrg_fastq_parse_device: null buffers");
  if (words_per_read != 1 && words_per_read != 2 && words_per_read != 4 && words_per_read != 8)
    return fail(MRG_ERR_ARG, "mrg_fastq_parse_device: words_per_read must be 1, 2, 4 or 8");
  if (phred != 33 && phred != 64) return fail(MRG_ERR_ARG, "mrg_fastq_parse_device: phred must be 33 or 64");
  if (n_bytes >= 0x7fffffffull) return fail(MRG_ERR_ARG, "mrg_fastq_parse_device: at most 2^31 - 2 bytes of text per call");
  HIP_TRY(hipSetDevice(ctx->device));
  uint64_t h[7];
  HIP_TRY(mrg::fastq_parse_device(d_text, n_bytes, phred, qual_cutoff, min_len, cut, ads, words_per_read, cap, d_words, d_lens, d_nmask, h,
                                  (hipStream_t)stream));
  info->n_records = h[0];
  info->n_kept = h[1];
  info->n_long = h[2];
  info->max_len = (uint32_t)h[3];
  info->has_n = (int32_t)h[4];
  info->status = (int32_t)h[5];
  info->bad_record = h[6];
  return MRG_OK;
}

int mrg_expand_compact(mrg_ctx* ctx, const uint64_t* d_bits, uint64_t n_words, const uint32_t* runs, uint32_t n_runs,
                       const uint8_t* d_quant8, const uint32_t* d_esc, uint64_t n_esc, uint64_t n, uint32_t n_samples, uint64_t* d_reads,
                       uint8_t* d_lens, uint32_t* d_quant, void* stream) {
  if (!ctx) return fail(MRG_ERR_ARG, "mrg_expand_compact: null argument");
  if (n && (!d_bits || !runs || !d_reads || !d_lens)) return fail(MRG_ERR_ARG, "mrg_expand_compact: null buffers");
  if (d_quant8 && (!d_quant || !n_samples || (n_esc && !d_esc))) return fail(MRG_ERR_ARG, "mrg_expand_compact: null count buffers");
  if (n >= 0xfffffff0ull || n * (uint64_t)(n_samples ? n_samples : 1u) >= 0xfffffff0ull)
    return fail(MRG_ERR_ARG, "mrg_expand_compact: at most 2^32-16 reads (and counts) per call");
  if (n_runs > mrg::kCompactMaxRuns || (n && !n_runs))
    return fail(MRG_ERR_ARG, "mrg_expand_compact: 1..%u length runs (got %u)", mrg::kCompactMaxRuns, n_runs);
  if (((uintptr_t)d_bits % 8) || ((uintptr_t)d_quant8 % 4) || ((uintptr_t)d_quant % 16))
    return fail(MRG_ERR_ARG, "mrg_expand_compact: buffers must be aligned (bits 8, quant8 4, quant 16 bytes)");
  mrg::CompactRuns cr;
  std::memset(&cr, 0, sizeof cr);
  cr.n = n_runs;
  uint64_t end = 0, base = 0;
  for (uint32_t r = 0; r < n_runs; ++r) {
    const uint32_t len = runs[2 * r], count = runs[2 * r + 1];
    if (len > 32u) return fail(MRG_ERR_ARG, "mrg_expand_compact: run %u has reads of %u nt (one-word reads only)", r, len);
    end += count;
    if (end > n) break;
    cr.end[r] = (uint32_t)end;
    cr.base[r] = (uint32_t)base;
    cr.len[r] = (uint8_t)len;
    base += ((uint64_t)count * 2u * len + 63u) / 64u;  // every run starts a word
  }
  if (end != n) return fail(MRG_ERR_ARG, "mrg_expand_compact: the runs count %llu reads, n is %llu", (unsigned long long)end, (unsigned long long)n);
  // (the kernel may read one word past a run's last read)
  if (base + 1 > n_words || base >= 0xffffffffull)
    return fail(MRG_ERR_ARG, "mrg_expand_compact: the runs need %llu + 1 words of bit stream, %llu were given", (unsigned long long)base,
                (unsigned long long)n_words);
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(mrg::expand_compact(d_bits, cr, d_quant8, d_esc, n_esc, n, n_samples, d_reads, d_lens, d_quant, (hipStream_t)stream));
  return MRG_OK;
}

int mrg_collapse_run(mrg_ctx* ctx, const uint64_t* d_reads, uint32_t words_per_read, const uint8_t* d_lens,
                     const uint64_t* d_nmask, const uint16_t* d_sample, uint64_t n, uint32_t n_samples,
                     uint32_t max_len, uint64_t cap, uint64_t* d_u_reads, uint8_t* d_u_lens,
                     uint64_t* d_u_nmask, uint32_t* d_quant, uint64_t* d_len_hist, uint64_t* n_unique,
                     void* stream) {
  if (!ctx || !n_unique || !d_len_hist) return fail(MRG_ERR_ARG, "mrg_collapse_run: null argument");
  if (n && (!d_reads || !d_lens || !d_u_reads || !d_u_lens || !d_quant))
    return fail(MRG_ERR_ARG, "mrg_collapse_run: null buffers");
  if (n_samples == 0 || n_samples > 65535) return fail(MRG_ERR_ARG, "mrg_collapse_run: n_samples out of range");
  if (n_samples > 1 && n && !d_sample) return fail(MRG_ERR_ARG, "mrg_collapse_run: d_sample required for >1 samples");
  if (words_per_read == 0 || words_per_read > MRG_MAX_WORDS)
    return fail(MRG_ERR_ARG, "mrg_collapse_run: bad words_per_read");
  if (n >= 0x7fffffffull) return fail(MRG_ERR_ARG, "mrg_collapse_run: at most 2^31-2 reads per call");
  if (d_nmask && !d_u_nmask) return fail(MRG_ERR_ARG, "mrg_collapse_run: d_u_nmask required with d_nmask");
  HIP_TRY(hipSetDevice(ctx->device));
  uint32_t nu = 0;
  mrg::CollapseInfo info;
  // temporaries of the keys-only path (3 x 8 B per read + the sort's own) out of the context's
  // scratch, grown on demand and kept: per-call hipMalloc / hipFree of gigabytes costs milliseconds
  const uint64_t want = n * 40ull + (64ull << 20);
  if (ctx->scratch_bytes < want) {
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));  // (nothing queued may still use the old arena)
    (void)hipFree(ctx->scratch);
    ctx->scratch = nullptr;
    ctx->scratch_bytes = 0;
    if (hipMalloc(&ctx->scratch, want) == hipSuccess) ctx->scratch_bytes = want;
    else (void)hipGetLastError();  // (the collapse then allocates per call)
  }
  hipError_t e = mrg::collapse_reads(d_reads, words_per_read, d_lens, d_nmask, d_sample, (uint32_t)n, n_samples,
                                     max_len, cap, d_u_reads, d_u_lens, d_u_nmask, d_quant, d_len_hist, &nu,
                                     (hipStream_t)stream, ctx->scratch, ctx->scratch_bytes, ctx->n_cu, ctx->collapse_fast != 0, &info);
  if (e == hipErrorInvalidValue)
    return fail(MRG_ERR_ARG, "mrg_collapse_run: cap %llu is smaller than the number of unique reads",
                (unsigned long long)cap);
  if (e == hipErrorInvalidDevicePointer)
    return fail(MRG_ERR_ARG, "mrg_collapse_run: a sample id is not below n_samples (%u)", n_samples);
  if (e != hipSuccess) return fail(MRG_ERR_HIP, "mrg_collapse_run: %s", hipGetErrorString(e));
  *n_unique = nu;
  ctx->last_collapse = info;  // (a call that failed leaves the record alone)
  return MRG_OK;
}

int mrg_ctx_last_collapse(const mrg_ctx* ctx, uint32_t* out8) {
  if (!ctx || !out8) return fail(MRG_ERR_ARG, "mrg_ctx_last_collapse: null argument");
  const mrg::CollapseInfo& c = ctx->last_collapse;
  const uint32_t v[8] = {c.path, c.reason, c.n_chunks, c.chunk, c.n_hot, c.n_pairs, c.n_buckets, c.n_unique};
  for (int i = 0; i < 8; ++i) out8[i] = v[i];
  return MRG_OK;
}

// ------------------------------------------------------------- table writers
int mrg_write_read_table(const char* path, int32_t mapped, const char* header, int32_t append, const uint64_t* reads,
                         uint32_t words_per_read, uint64_t stride, const uint8_t* lens, const uint64_t* nmask,
                         uint64_t n, const int8_t* pass_id, const int32_t* ref_id, const uint32_t* quant,
                         uint32_t n_samples, uint32_t n_slots, const char* const* names, const uint64_t* names_off,
                         uint64_t* rows) {
  if (!path || (n && (!reads || !lens || !pass_id || !ref_id || (n_samples && !quant))))
    return fail(MRG_ERR_ARG, "mrg_write_read_table: null argument");
  if (mapped && (!names || !names_off)) return fail(MRG_ERR_ARG, "mrg_write_read_table: mapped rows need the entry names");
  if (words_per_read == 0 || words_per_read > MRG_MAX_WORDS || stride < n || n_slots > MRG_MAX_PASSES)
    return fail(MRG_ERR_ARG, "mrg_write_read_table: bad words_per_read / stride / n_slots");
  try {
    const uint64_t k = mrg::write_read_table(path, mapped != 0, header, append != 0, reads, words_per_read, stride, lens,
                                             nmask, n, pass_id, ref_id, quant, n_samples, n_slots, names, names_off);
    if (rows) *rows = k;
    return MRG_OK;
  } catch (const std::exception& e) {
    return fail(MRG_ERR_IO, "mrg_write_read_table: %s", e.what());
  }
}

int mrg_write_isomir_tables(const char* isomirs_path, const char* samples_path, const char* header1, const char* header2,
                            const uint64_t* reads, uint32_t words_per_read, uint64_t stride, const uint8_t* lens,
                            const uint64_t* nmask, uint64_t n, const int8_t* pass_id, const int32_t* ref_id, const uint32_t* quant,
                            uint32_t n_samples, int32_t canon_pass, int32_t isomir_pass, const int32_t* group_of_entry,
                            uint64_t n_entries, const char* const* group_names, uint32_t n_groups, const double* filtered,
                            uint64_t* rows) {
  if (!isomirs_path || !samples_path || !header1 || !header2 || !filtered || !n_samples ||
      (n && (!reads || !lens || !pass_id || !ref_id || !quant || !group_of_entry || !group_names)))
    return fail(MRG_ERR_ARG, "mrg_write_isomir_tables: null argument");
  if (words_per_read == 0 || words_per_read > MRG_MAX_WORDS || stride < n)
    return fail(MRG_ERR_ARG, "mrg_write_isomir_tables: bad words_per_read / stride");
  try {
    const uint64_t k = mrg::write_isomir_tables(isomirs_path, samples_path, header1, header2, reads, words_per_read, stride, lens, nmask, n,
                                                pass_id, ref_id, quant, n_samples, canon_pass, isomir_pass, group_of_entry, n_entries,
                                                group_names, n_groups, filtered);
    if (rows) *rows = k;
    return MRG_OK;
  } catch (const std::exception& e) {
    return fail(MRG_ERR_IO, "mrg_write_isomir_tables: %s", e.what());
  }
}

// ------------------------------------------------------------- -gff
int mrg_isomir_classify(mrg_ctx* ctx, const uint64_t* d_reads, uint32_t words_per_read, uint64_t stride, const uint8_t* d_lens,
                        const uint64_t* d_nmask, uint64_t n, const int8_t* d_pass_id, const int32_t* d_ref_id, const int32_t* d_pos,
                        int32_t canon_pass, int32_t isomir_pass, const int32_t* desc, uint64_t n_entries, const uint64_t* text,
                        const uint64_t* nplane, uint64_t text_words, uint64_t cap, uint32_t* d_idx, int32_t* d_rec, uint64_t* d_mask,
                        uint64_t* counts, float* kernel_ms, void* stream) {
  if (!ctx || !counts) return fail(MRG_ERR_ARG, "mrg_isomir_classify: null argument");
  if (kernel_ms) *kernel_ms = 0.0f;
  if (n && (!d_reads || !d_lens || !d_pass_id || !d_ref_id || !d_pos)) return fail(MRG_ERR_ARG, "mrg_isomir_classify: null buffers");
  if ((n_entries && !desc) || (text_words && (!text || !nplane))) return fail(MRG_ERR_ARG, "mrg_isomir_classify: null tables");
  if (cap && (!d_idx || !d_rec || !d_mask)) return fail(MRG_ERR_ARG, "mrg_isomir_classify: null output buffers");
  if (words_per_read != 1 && words_per_read != 2 && words_per_read != 4 && words_per_read != 8)
    return fail(MRG_ERR_ARG, "mrg_isomir_classify: words_per_read must be 1, 2, 4 or 8");
  if (stride < n || n >= (1ull << 31)) return fail(MRG_ERR_ARG, "mrg_isomir_classify: bad stride / n");
  if (canon_pass == isomir_pass || canon_pass < 0 || isomir_pass < 0 || canon_pass > 127 || isomir_pass > 127)
    return fail(MRG_ERR_ARG, "mrg_isomir_classify: the two passes must differ and lie in 0..127");
  if (n_entries >= (1ull << 31) || text_words >= (1ull << 31)) return fail(MRG_ERR_ARG, "mrg_isomir_classify: tables too large");
  // the kernel trusts the table: every resolvable entry's precursor lies inside the text, its mature inside the precursor
  for (uint64_t e = 0; e < n_entries; ++e) {
    const int32_t* d = desc + e * mrg::kIsoDescInts;
    if (d[mrg::kIsoDescStatus] < 0 || d[mrg::kIsoDescStatus] > 2)
      return fail(MRG_ERR_ARG, "mrg_isomir_classify: entry %llu has status %d", (unsigned long long)e, d[mrg::kIsoDescStatus]);
    if (d[mrg::kIsoDescStatus] != 0) continue;
    const int64_t off = d[mrg::kIsoDescOff], len = d[mrg::kIsoDescLen], m0 = d[mrg::kIsoDescM0], mat = d[mrg::kIsoDescMat];
    if (off < 0 || len < 0 || len > (1 << 24) || m0 < 0 || mat < 0 || m0 + mat > len || off + (len + 31) / 32 > (int64_t)text_words)
      return fail(MRG_ERR_ARG, "mrg_isomir_classify: entry %llu lies outside the precursor table", (unsigned long long)e);
  }
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  counts[0] = counts[1] = 0;
  if (n == 0) return MRG_OK;
  // context scratch: [entry table | text | N plane | flags -> offsets (2n + 1) | scan scratch], 256-byte aligned pieces
  auto up = [](uint64_t b) { return (b + 255) & ~255ull; };
  const uint64_t n_flags = 2 * n + 1;
  const uint64_t o_desc = 0, o_text = o_desc + up(n_entries * mrg::kIsoDescInts * sizeof(int32_t)),
                 o_npl = o_text + up(text_words * sizeof(uint64_t)), o_flags = o_npl + up(text_words * sizeof(uint64_t)),
                 o_tmp = o_flags + up(n_flags * sizeof(uint32_t)), need_bytes = o_tmp + up(mrg::prims::scan_temp_bytes(n_flags));
  if (ctx->scratch_bytes < need_bytes) {
    HIP_TRY(hipStreamSynchronize(st));
    (void)hipFree(ctx->scratch);
    ctx->scratch = nullptr;
    ctx->scratch_bytes = 0;
    HIP_TRY(hipMalloc(&ctx->scratch, need_bytes));
    ctx->scratch_bytes = need_bytes;
  }
  char* base = (char*)ctx->scratch;
  uint32_t* flags = (uint32_t*)(base + o_flags);
  // select and order: the exclusive sums of [canon flags | isomiR flags | 0] are the rows.  (A caller that counts first and
  // fills then, as Engine.isomir_classify does, runs this stage twice: two launches and a scan over 2n + 1 flags, small next
  // to the download of the rows; the offsets are not kept between calls because another call may use the scratch.)
  HIP_TRY(mrg::iso_flags_launch(d_pass_id, n, canon_pass, isomir_pass, flags, st));
  HIP_TRY(mrg::prims::exclusive_sum_u32(flags, flags, n_flags, base + o_tmp, st));
  uint32_t ends[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(&ends[0], flags + n, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(&ends[1], flags + 2 * n, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  counts[0] = ends[0];
  counts[1] = ends[1] - ends[0];
  const uint64_t rows = std::min<uint64_t>(ends[1], cap);
  if (rows == 0) return MRG_OK;
  HIP_TRY(mrg::iso_scatter_launch(d_pass_id, n, canon_pass, isomir_pass, flags, cap, d_idx, st));
  if (n_entries) HIP_TRY(hipMemcpyAsync(base + o_desc, desc, n_entries * mrg::kIsoDescInts * sizeof(int32_t), hipMemcpyHostToDevice, st));
  if (text_words) {
    HIP_TRY(hipMemcpyAsync(base + o_text, text, text_words * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(base + o_npl, nplane, text_words * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  }
  mrg::IsoClassifyParams p;
  p.reads = d_reads;
  p.nmask = d_nmask;
  p.lens = d_lens;
  p.ref_id = d_ref_id;
  p.pos = d_pos;
  p.stride = stride;
  p.W = words_per_read;
  p.idx = d_idx;
  p.rows = (uint32_t)rows;
  p.n_canon = ends[0];
  p.desc = (const int32_t*)(base + o_desc);
  p.n_entries = (uint32_t)n_entries;
  p.text = (const uint64_t*)(base + o_text);
  p.nplane = (const uint64_t*)(base + o_npl);
  p.text_words = (uint32_t)text_words;
  p.rec = d_rec;
  p.mask = (uint32_t*)d_mask;
  p.mask_words = (words_per_read + 1) / 2;
  // kernel_ms: classify_kernel alone, between two events on the stream
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  hipError_t e = hipSuccess;
  if (kernel_ms) {
    e = hipEventCreate(&ev0);
    if (e == hipSuccess) e = hipEventCreate(&ev1);
    if (e == hipSuccess) e = hipEventRecord(ev0, st);
  }
  if (e == hipSuccess) e = mrg::iso_classify_launch(p, st);
  if (e == hipSuccess && kernel_ms) e = hipEventRecord(ev1, st);
  // (the tables were copied from pageable host memory, which the caller may free on return)
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e == hipSuccess && kernel_ms) e = hipEventElapsedTime(kernel_ms, ev0, ev1);
  if (ev0) (void)hipEventDestroy(ev0);
  if (ev1) (void)hipEventDestroy(ev1);
  HIP_TRY(e);
  return MRG_OK;
}

int mrg_write_isomir_gff(const char* const* paths, const char* const* coldata, uint32_t n_samples, const char* source,
                         const uint64_t* reads, uint32_t words_per_read, uint64_t stride, const uint8_t* lens, const uint64_t* nmask,
                         uint64_t n, const uint32_t* quant, const uint32_t* idx, const int32_t* rec, const uint64_t* mask, uint64_t k,
                         const char* const* entry_names, const char* const* pre_names, uint64_t n_entries, uint64_t* rows) {
  if (!paths || !coldata || !source || !n_samples) return fail(MRG_ERR_ARG, "mrg_write_isomir_gff: null argument");
  for (uint32_t s = 0; s < n_samples; ++s)
    if (!paths[s] || !coldata[s]) return fail(MRG_ERR_ARG, "mrg_write_isomir_gff: null argument");
  if (k && (!reads || !lens || !quant || !idx || !rec || !mask || !entry_names || !pre_names))
    return fail(MRG_ERR_ARG, "mrg_write_isomir_gff: null buffers");
  if ((words_per_read != 1 && words_per_read != 2 && words_per_read != 4 && words_per_read != 8) || stride < n)
    return fail(MRG_ERR_ARG, "mrg_write_isomir_gff: bad words_per_read / stride");
  return guarded("mrg_write_isomir_gff", [&] {
    mrg::write_isomir_gff(paths, coldata, n_samples, source, reads, words_per_read, stride, lens, nmask, n, quant, idx, rec, mask, k,
                          entry_names, pre_names, n_entries, rows);
    return MRG_OK;
  });
}

// ------------------------------------------------------------- -trf
extern "C++" {
namespace {

struct TrfBuf {  // the carver with a device allocation of its own: 256-byte aligned pieces, freed on return
  Carver c{256, 1};
  char* p = nullptr;
  ~TrfBuf() {
    if (p) (void)hipFree(p);
  }
  uint64_t reserve(uint64_t bytes) { return c.take<char>(bytes).off; }
  hipError_t alloc() { return hipMalloc((void**)&p, std::max<size_t>(c.total(), 256)); }
  template <class T>
  T* at(uint64_t off) const { return Piece<T>{off}.at(p); }
};

uint32_t bits_for(uint64_t v) {  // the smallest b with v < 2^b
  uint32_t b = 0;
  while (b < 64 && (v >> b)) ++b;
  return b;
}

}  // namespace
}  // extern "C++"

int mrg_trf_classify(mrg_ctx* ctx, const uint64_t* d_reads, uint32_t words_per_read, uint64_t stride, const uint8_t* d_lens,
                     const uint64_t* d_nmask, uint64_t n, const int8_t* d_pass_id, int32_t mature_pass, int32_t trailer_pass,
                     int32_t mature_lib, int32_t pre_lib, const int32_t* desc, uint64_t n_entries, const int32_t* clusters,
                     uint64_t n_clusters, const uint64_t* text, const uint64_t* plane, uint64_t text_words, uint64_t cap_rows,
                     uint64_t cap_hits, int32_t* d_rec, int32_t* d_hits, uint64_t* counts, float* kernel_ms, void* stream) {
  if (!ctx || !counts) return fail(MRG_ERR_ARG, "mrg_trf_classify: null argument");
  if (kernel_ms) kernel_ms[0] = kernel_ms[1] = 0.0f;
  if (n && (!d_reads || !d_lens || !d_pass_id)) return fail(MRG_ERR_ARG, "mrg_trf_classify: null buffers");
  if ((n_entries && !desc) || (n_clusters && !clusters) || (text_words && (!text || !plane)))
    return fail(MRG_ERR_ARG, "mrg_trf_classify: null tables");
  if ((cap_rows && !d_rec) || (cap_hits && !d_hits)) return fail(MRG_ERR_ARG, "mrg_trf_classify: null output buffers");
  if (words_per_read != 1 && words_per_read != 2 && words_per_read != 4 && words_per_read != 8)
    return fail(MRG_ERR_ARG, "mrg_trf_classify: words_per_read must be 1, 2, 4 or 8");
  if (stride < n || n >= (1ull << 31)) return fail(MRG_ERR_ARG, "mrg_trf_classify: bad stride / n");
  if (mature_pass == trailer_pass || mature_pass < 0 || trailer_pass < 0 || mature_pass > 127 || trailer_pass > 127)
    return fail(MRG_ERR_ARG, "mrg_trf_classify: the two passes must differ and lie in 0..127");
  if (mature_lib < 0 || (size_t)mature_lib >= ctx->libs.size() || pre_lib < 0 || (size_t)pre_lib >= ctx->libs.size())
    return fail(MRG_ERR_ARG, "mrg_trf_classify: unknown library");
  const uint64_t n_mature_entries = ctx->libs[mature_lib].n_ref;
  if (n_entries != n_mature_entries + ctx->libs[pre_lib].n_ref || n_entries >= (1ull << 30) || n_clusters >= (1ull << 30) ||
      text_words >= (1ull << 31))
    return fail(MRG_ERR_ARG, "mrg_trf_classify: the entry table must hold the entries of the two libraries, in that order");
  // the kernels trust the tables: a representative is an entry, the predefined tRFs of an entry and their strings lie inside
  // the tables
  for (uint64_t e = 0; e < n_entries; ++e) {
    const int32_t* d = desc + e * mrg::kTrfDescInts;
    const int64_t rep = d[mrg::kTrfDescRep], first = d[mrg::kTrfDescFirst], cnt = d[mrg::kTrfDescCount];
    const bool same_lib = rep < 0 || ((uint64_t)rep < n_mature_entries) == (e < n_mature_entries);
    if (rep < -1 || rep >= (int64_t)n_entries || !same_lib || cnt < 0 || (cnt && (first < 0 || first + cnt > (int64_t)n_clusters)))
      return fail(MRG_ERR_ARG, "mrg_trf_classify: entry %llu points outside the tables", (unsigned long long)e);
  }
  for (uint64_t t = 0; t < n_clusters; ++t) {
    const int32_t* c = clusters + t * mrg::kTrfClusterInts;
    const int64_t len = c[mrg::kTrfClusterLen], word = c[mrg::kTrfClusterWord];
    if (len < 0 || len > (1 << 20) || word < 0 || word + (len + 31) / 32 > (int64_t)text_words)
      return fail(MRG_ERR_ARG, "mrg_trf_classify: predefined tRF %llu lies outside the text table", (unsigned long long)t);
  }
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  counts[0] = counts[1] = counts[2] = 0;
  if (n == 0) return MRG_OK;
  const uint32_t W = words_per_read;

  // ---- select and order: the exclusive sums of [mature flags | trailer flags | 0] are the rows (as mrg_isomir_classify)
  const uint64_t n_flags = 2 * n + 1;
  TrfBuf sel;
  const uint64_t o_flags = sel.reserve(n_flags * sizeof(uint32_t)), o_scan = sel.reserve(mrg::prims::scan_temp_bytes(n_flags));
  HIP_TRY(sel.alloc());
  uint32_t* flags = sel.at<uint32_t>(o_flags);
  HIP_TRY(mrg::iso_flags_launch(d_pass_id, n, mature_pass, trailer_pass, flags, st));
  HIP_TRY(mrg::prims::exclusive_sum_u32(flags, flags, n_flags, sel.p + o_scan, st));
  uint32_t ends[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(&ends[0], flags + n, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(&ends[1], flags + 2 * n, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  counts[0] = ends[0];
  counts[1] = ends[1] - ends[0];
  const uint32_t k = (uint32_t)std::min<uint64_t>(ends[1], cap_rows);
  if (k == 0) return MRG_OK;
  const uint32_t n_a = std::min(ends[0], k), n_b = k - n_a;

  // ---- the selected reads as two contiguous read sets, the tables
  TrfBuf rs;
  const uint64_t set_a = (uint64_t)W * n_a * sizeof(uint64_t), set_b = (uint64_t)W * n_b * sizeof(uint64_t);
  const uint64_t o_idx = rs.reserve(k * sizeof(uint32_t)), o_sub = rs.reserve(k), o_tail = rs.reserve(k), o_wa = rs.reserve(set_a),
                 o_wb = rs.reserve(set_b), o_na = rs.reserve(d_nmask ? set_a : 0), o_nb = rs.reserve(d_nmask ? set_b : 0),
                 o_mm = rs.reserve(k), o_offa = rs.reserve((n_a + 1ull) * sizeof(uint64_t)),
                 o_offb = rs.reserve((n_b + 1ull) * sizeof(uint64_t)), o_h0 = rs.reserve(k * sizeof(uint32_t)),
                 o_h1 = rs.reserve(k * sizeof(uint32_t)), o_desc = rs.reserve(n_entries * mrg::kTrfDescInts * sizeof(int32_t)),
                 o_cl = rs.reserve(n_clusters * mrg::kTrfClusterInts * sizeof(int32_t)), o_text = rs.reserve(text_words * sizeof(uint64_t)),
                 o_plane = rs.reserve(text_words * sizeof(uint64_t));
  HIP_TRY(rs.alloc());
  uint32_t* idx = rs.at<uint32_t>(o_idx);
  HIP_TRY(mrg::iso_scatter_launch(d_pass_id, n, mature_pass, trailer_pass, flags, k, idx, st));
  if (n_entries) HIP_TRY(hipMemcpyAsync(rs.p + o_desc, desc, n_entries * mrg::kTrfDescInts * sizeof(int32_t), hipMemcpyHostToDevice, st));
  if (n_clusters)
    HIP_TRY(hipMemcpyAsync(rs.p + o_cl, clusters, n_clusters * mrg::kTrfClusterInts * sizeof(int32_t), hipMemcpyHostToDevice, st));
  if (text_words) {
    HIP_TRY(hipMemcpyAsync(rs.p + o_text, text, text_words * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(rs.p + o_plane, plane, text_words * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  }
  HIP_TRY(hipMemsetAsync(rs.p + o_h0, 0, k * sizeof(uint32_t), st));
  HIP_TRY(hipMemsetAsync(rs.p + o_h1, 0, k * sizeof(uint32_t), st));
  mrg::TrfGatherParams g;
  g.reads = d_reads;
  g.nmask = d_nmask;
  g.lens = d_lens;
  g.stride = stride;
  g.W = W;
  g.idx = idx;
  g.k = k;
  g.n_mature = n_a;
  g.words_a = rs.at<uint64_t>(o_wa);
  g.words_b = rs.at<uint64_t>(o_wb);
  g.nmask_a = d_nmask ? rs.at<uint64_t>(o_na) : nullptr;
  g.nmask_b = d_nmask ? rs.at<uint64_t>(o_nb) : nullptr;
  g.sub_len = rs.at<uint8_t>(o_sub);
  g.tail = rs.at<uint8_t>(o_tail);
  HIP_TRY(mrg::trf_gather_launch(g, st));

  // ---- list: -v 1 against the mature tRNAs, -v 0 against the pre-tRNAs (`-a --best --strata`, the whole read is seed)
  constexpr int32_t kVModeSeed = 1024;
  uint64_t total_a = 0, total_b = 0;
  int rc = MRG_OK;
  if (n_a)
    rc = mrg_list_best_count(ctx, g.words_a, W, g.sub_len, g.nmask_a, n_a, mature_lib, kVModeSeed, 1, 1, rs.at<uint8_t>(o_mm),
                             rs.at<uint64_t>(o_offa), &total_a, stream);
  if (rc != MRG_OK) return rc;
  if (n_b)
    rc = mrg_list_best_count(ctx, g.words_b, W, g.sub_len + n_a, g.nmask_b, n_b, pre_lib, kVModeSeed, 0, 0, rs.at<uint8_t>(o_mm) + n_a,
                             rs.at<uint64_t>(o_offb), &total_b, stream);
  if (rc != MRG_OK) return rc;
  const uint64_t H = total_a + total_b;
  const uint32_t owner_bits = bits_for(k), entry_bits = bits_for(n_entries),
                 pos_bits = bits_for(std::max(ctx->libs[mature_lib].n, ctx->libs[pre_lib].n));
  if (H >= (1ull << 32) - 1 || pos_bits > 30 || owner_bits + entry_bits + pos_bits > 64)
    return fail(MRG_ERR_ARG, "mrg_trf_classify: too many alignments for one call (split the reads)");
  TrfBuf al;
  const uint64_t o_ref = al.reserve(H * sizeof(int32_t)), o_pos = al.reserve(H * sizeof(int32_t)), o_k0 = al.reserve(H * sizeof(uint64_t)),
                 o_k1 = al.reserve(H * sizeof(uint64_t)), o_head = al.reserve((H + 1) * sizeof(uint32_t)),
                 o_tmp = al.reserve(std::max<uint64_t>(mrg::prims::radix_temp_bytes(H + 1), mrg::prims::scan_temp_bytes(H + 1)));
  HIP_TRY(al.alloc());
  int32_t *ref = al.at<int32_t>(o_ref), *pos = al.at<int32_t>(o_pos);
  uint64_t* keys[2] = {al.at<uint64_t>(o_k0), al.at<uint64_t>(o_k1)};
  if (total_a) {
    rc = mrg_list_best_fill(ctx, g.words_a, W, g.sub_len, g.nmask_a, n_a, mature_lib, kVModeSeed, 1, 1, rs.at<uint8_t>(o_mm),
                            rs.at<uint64_t>(o_offa), total_a, ref, pos, stream);
    if (rc != MRG_OK) return rc;
    HIP_TRY(mrg::trf_keys_launch(rs.at<uint64_t>(o_offa), ref, pos, n_a, 0u, 0u, entry_bits, pos_bits, 0, keys[0], st));
  }
  if (total_b) {
    rc = mrg_list_best_fill(ctx, g.words_b, W, g.sub_len + n_a, g.nmask_b, n_b, pre_lib, kVModeSeed, 0, 0, rs.at<uint8_t>(o_mm) + n_a,
                            rs.at<uint64_t>(o_offb), total_b, ref + total_a, pos + total_a, stream);
    if (rc != MRG_OK) return rc;
    HIP_TRY(mrg::trf_keys_launch(rs.at<uint64_t>(o_offb), ref + total_a, pos + total_a, n_b, n_a, (uint32_t)n_mature_entries, entry_bits,
                                 pos_bits, total_a, keys[0], st));
  }
  // ---- order by (owner, entry, offset); the first alignment of an (owner, entry) run is kept (the lowest offset)
  bool second = false;
  if (H) HIP_TRY(mrg::prims::radix_sort_pairs_u64(keys[0], keys[1], nullptr, nullptr, (uint32_t)H, owner_bits + entry_bits + pos_bits,
                                                  al.p + o_tmp, st, &second));
  const uint64_t* sorted = keys[second ? 1 : 0];
  uint32_t* head = al.at<uint32_t>(o_head);
  HIP_TRY(mrg::trf_heads_launch(sorted, (uint32_t)H, pos_bits, head, st));
  HIP_TRY(mrg::prims::exclusive_sum_u32(head, head, H + 1, al.p + o_tmp, st));
  uint32_t kept = 0;
  HIP_TRY(hipMemcpyAsync(&kept, head + H, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  counts[2] = kept;

  TrfBuf hb;
  const uint64_t o_hits = hb.reserve((uint64_t)kept * mrg::kTrfHitInts * sizeof(int32_t));
  HIP_TRY(hb.alloc());
  mrg::TrfTypeParams tp;
  tp.keys = sorted;
  tp.slot = head;
  tp.n_keys = (uint32_t)H;
  tp.entry_bits = entry_bits;
  tp.pos_bits = pos_bits;
  tp.lens = d_lens;
  tp.idx = idx;
  tp.tail = g.tail;
  tp.k = k;
  tp.desc = rs.at<int32_t>(o_desc);
  tp.n_entries = (uint32_t)n_entries;
  tp.hits = hb.at<int32_t>(o_hits);
  tp.hit0 = rs.at<uint32_t>(o_h0);
  tp.hit1 = rs.at<uint32_t>(o_h1);
  mrg::TrfAssignParams ap;
  ap.reads = d_reads;
  ap.nmask = d_nmask;
  ap.lens = d_lens;
  ap.stride = stride;
  ap.W = W;
  ap.idx = idx;
  ap.sub_len = g.sub_len;
  ap.tail = g.tail;
  ap.k = k;
  ap.n_mature = n_a;
  ap.hits = tp.hits;
  ap.hit0 = tp.hit0;
  ap.hit1 = tp.hit1;
  ap.desc = tp.desc;
  ap.n_entries = tp.n_entries;
  ap.clusters = rs.at<int32_t>(o_cl);
  ap.n_clusters = (uint32_t)n_clusters;
  ap.text = rs.at<uint64_t>(o_text);
  ap.plane = rs.at<uint64_t>(o_plane);
  ap.rec = d_rec;
  // kernel_ms: trf_type_kernel and trf_assign_kernel alone, between events on the stream
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  hipError_t e = hipSuccess;
  if (kernel_ms)
    for (int i = 0; i < 3 && e == hipSuccess; ++i) e = hipEventCreate(&ev[i]);
  if (e == hipSuccess && kernel_ms) e = hipEventRecord(ev[0], st);
  if (e == hipSuccess) e = mrg::trf_type_launch(tp, st);
  if (e == hipSuccess && kernel_ms) e = hipEventRecord(ev[1], st);
  if (e == hipSuccess) e = mrg::trf_assign_launch(ap, st);
  if (e == hipSuccess && kernel_ms) e = hipEventRecord(ev[2], st);
  const uint64_t out_hits = std::min<uint64_t>(kept, cap_hits);
  if (e == hipSuccess && out_hits)
    e = hipMemcpyAsync(d_hits, tp.hits, out_hits * mrg::kTrfHitInts * sizeof(int32_t), hipMemcpyDeviceToDevice, st);
  // (the tables were copied from pageable host memory, and the buffers above are freed on return)
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e == hipSuccess && kernel_ms) e = hipEventElapsedTime(&kernel_ms[0], ev[0], ev[1]);
  if (e == hipSuccess && kernel_ms) e = hipEventElapsedTime(&kernel_ms[1], ev[1], ev[2]);
  for (hipEvent_t x : ev)
    if (x) (void)hipEventDestroy(x);
  HIP_TRY(e);
  return MRG_OK;
}

int mrg_write_trf_tables(const char* const* paths, const char* const* samples, uint32_t n_samples, const uint64_t* denom,
                         const uint64_t* reads, uint32_t words_per_read, uint64_t stride, const uint8_t* lens, const uint64_t* nmask,
                         uint64_t n, const uint32_t* quant, const int32_t* rec, uint64_t k, const int32_t* hits, uint64_t h,
                         const int32_t* desc, const char* const* entry_names, const char* const* aa_types, const char* const* anticodons,
                         uint64_t n_entries, const int32_t* clusters, uint64_t n_clusters, const char* const* merged_names,
                         uint64_t n_merged, uint64_t* rows) {
  if (!paths || !samples || !denom || !n_samples) return fail(MRG_ERR_ARG, "mrg_write_trf_tables: null argument");
  for (int i = 0; i < 4; ++i)
    if (!paths[i]) return fail(MRG_ERR_ARG, "mrg_write_trf_tables: null argument");
  for (uint32_t s = 0; s < n_samples; ++s)
    if (!samples[s]) return fail(MRG_ERR_ARG, "mrg_write_trf_tables: null argument");
  if (k && (!reads || !lens || !quant || !rec || !desc || !entry_names || !aa_types || !anticodons))
    return fail(MRG_ERR_ARG, "mrg_write_trf_tables: null buffers");
  if ((h && !hits) || (n_clusters && !clusters) || (n_merged && !merged_names)) return fail(MRG_ERR_ARG, "mrg_write_trf_tables: null buffers");
  if ((words_per_read != 1 && words_per_read != 2 && words_per_read != 4 && words_per_read != 8) || stride < n)
    return fail(MRG_ERR_ARG, "mrg_write_trf_tables: bad words_per_read / stride");
  return guarded("mrg_write_trf_tables", [&] {
    const mrg::TrfWriteArgs a{paths, samples, n_samples, denom, reads, words_per_read, stride, lens, nmask, n, quant, rec, k, hits, h,
                              desc, entry_names, aa_types, anticodons, n_entries, clusters, n_clusters, merged_names, n_merged};
    mrg::write_trf_tables(a, rows);
    return MRG_OK;
  });
}

// ------------------------------------------------------------- -trf: the per-sample blocks (csrc/trf_groups.hip)
double mrg_trf_rp100k_text(uint64_t count, uint64_t denom) { return mrg::trf_rp100k_text(count, denom); }

int mrg_trf_sample_groups(mrg_ctx* ctx, const uint64_t* d_reads, uint32_t words_per_read, uint64_t stride, const uint8_t* d_lens,
                          const uint64_t* d_nmask, uint64_t n, const uint32_t* d_quant, uint32_t n_samples, const int32_t* d_rec,
                          uint64_t k, const uint64_t* denom, const int32_t* entries, uint64_t n_entries, uint32_t n_names,
                          uint64_t cap_blocks, uint64_t cap_rows, int32_t* blocks, uint64_t* block_sums, uint32_t* off, int32_t* groups,
                          uint64_t* d_codes, uint64_t* d_nmask_out, uint16_t* d_span, double* d_rpm, uint32_t* d_rows, uint64_t* counts,
                          float* kernel_ms, void* stream) {
  const char* fn = "mrg_trf_sample_groups";
  if (!ctx || !counts || !denom || !n_samples) return fail(MRG_ERR_ARG, "%s: null argument", fn);
  if (kernel_ms) kernel_ms[0] = kernel_ms[1] = kernel_ms[2] = kernel_ms[3] = 0.0f;
  if (k && (!d_reads || !d_lens || !d_quant || !d_rec)) return fail(MRG_ERR_ARG, "%s: null buffers", fn);
  if (n_entries && !entries) return fail(MRG_ERR_ARG, "%s: null tables", fn);
  if (cap_blocks && (!blocks || !block_sums || !off || !groups)) return fail(MRG_ERR_ARG, "%s: null output buffers", fn);
  if (cap_rows && (!d_codes || !d_span || !d_rpm || !d_rows)) return fail(MRG_ERR_ARG, "%s: null output buffers", fn);
  if (words_per_read != 1 && words_per_read != 2 && words_per_read != 4 && words_per_read != 8)
    return fail(MRG_ERR_ARG, "%s: words_per_read must be 1, 2, 4 or 8", fn);
  if (stride < n || n >= (1ull << 31)) return fail(MRG_ERR_ARG, "%s: bad stride / n", fn);
  // (a printed row's number is an int32 of the block table, and every (row, sample) pair may be one)
  if (n_samples > (1u << 16) || k * n_samples >= (1ull << 31))
    return fail(MRG_ERR_ARG, "%s: rows x samples must stay below 2^31 (split the samples)", fn);
  // (the cells are ordered into blocks on the host: a table for tRNA names, not for reads)
  if (n_entries >= (1ull << 30) || (uint64_t)n_names * n_samples > (1ull << 22))
    return fail(MRG_ERR_ARG, "%s: too many entries, or more than 2^22 (sample, name) cells", fn);
  // the kernels trust the entry table: a name id is a name, a template is -1 or a length
  for (uint64_t e = 0; e < n_entries; ++e) {
    const int32_t* d = entries + e * mrg::kTrfSampleInts;
    if (d[mrg::kTrfSampleName] < 0 || (uint32_t)d[mrg::kTrfSampleName] >= n_names || d[mrg::kTrfSampleTemplate] < -1)
      return fail(MRG_ERR_ARG, "%s: entry %llu: name id or template length out of range", fn, (unsigned long long)e);
  }
  for (int i = 0; i < 8; ++i) counts[i] = 0;
  counts[6] = mrg::kTrfNone;
  if (cap_blocks) off[0] = 0;
  if (k == 0) return MRG_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  const uint32_t S = n_samples, K = (uint32_t)k;
  const uint64_t total = (uint64_t)S * K, cells = (uint64_t)S * n_names;

  // ---- items: flags of the printed rows, the dense [S][names] sums
  TrfBuf ib;
  const uint64_t o_flags = ib.reserve((total + 1) * sizeof(uint32_t)), o_scan = ib.reserve(mrg::prims::scan_temp_bytes(total + 1)),
                 o_sums = ib.reserve(cells * sizeof(uint64_t)), o_np = ib.reserve(cells * sizeof(uint32_t)),
                 o_rep = ib.reserve(cells * sizeof(int32_t)), o_stat = ib.reserve(mrg::kTrfStatWords * sizeof(uint32_t)),
                 o_ent = ib.reserve(n_entries * mrg::kTrfSampleInts * sizeof(int32_t)), o_den = ib.reserve(S * sizeof(uint64_t)),
                 o_cb = ib.reserve(cells * sizeof(uint32_t));
  HIP_TRY(ib.alloc());
  uint32_t* flags = ib.at<uint32_t>(o_flags);
  uint32_t stat[mrg::kTrfStatWords] = {mrg::kTrfNone, mrg::kTrfNone, 0, 0, 0, 0, 0, 0};
  HIP_TRY(hipMemcpyAsync(ib.p + o_stat, stat, sizeof stat, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(ib.p + o_ent, entries, n_entries * mrg::kTrfSampleInts * sizeof(int32_t), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(ib.p + o_den, denom, S * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(ib.p + o_sums, 0, cells * sizeof(uint64_t), st));
  HIP_TRY(hipMemsetAsync(ib.p + o_np, 0, cells * sizeof(uint32_t), st));
  HIP_TRY(hipMemsetAsync(ib.p + o_rep, 0x7F, cells * sizeof(int32_t), st));  // (0x7F7F7F7F: above every entry)
  HIP_TRY(hipMemsetAsync(flags + total, 0, sizeof(uint32_t), st));
  mrg::TrfGroupParams p;
  p.reads = d_reads;
  p.nmask = d_nmask;
  p.lens = d_lens;
  p.stride = stride;
  p.n = n;
  p.W = words_per_read;
  p.quant = d_quant;
  p.S = S;
  p.rec = d_rec;
  p.k = K;
  p.entries = ib.at<int32_t>(o_ent);
  p.n_entries = (uint32_t)n_entries;
  p.n_names = n_names;
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  struct EventGuard {
    hipEvent_t* ev;
    ~EventGuard() {
      for (int i = 0; i < 5; ++i)
        if (ev[i]) (void)hipEventDestroy(ev[i]);
    }
  } guard{ev};
  if (kernel_ms)
    for (int i = 0; i < 5; ++i) HIP_TRY(hipEventCreate(&ev[i]));
  if (kernel_ms) HIP_TRY(hipEventRecord(ev[0], st));
  HIP_TRY(mrg::trf_items_launch(p, flags, ib.at<uint64_t>(o_sums), ib.at<uint32_t>(o_np), ib.at<int32_t>(o_rep), ib.at<uint32_t>(o_stat), st));
  HIP_TRY(mrg::prims::exclusive_sum_u32(flags, flags, total + 1, ib.p + o_scan, st));
  if (kernel_ms) HIP_TRY(hipEventRecord(ev[1], st));
  std::vector<uint64_t> h_sums(cells);
  std::vector<uint32_t> h_np(cells);
  std::vector<int32_t> h_rep(cells);
  uint32_t n_rows = 0;
  HIP_TRY(hipMemcpyAsync(stat, ib.p + o_stat, sizeof stat, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(&n_rows, flags + total, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  if (cells) {
    HIP_TRY(hipMemcpyAsync(h_sums.data(), ib.p + o_sums, cells * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h_np.data(), ib.p + o_np, cells * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h_rep.data(), ib.p + o_rep, cells * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(hipStreamSynchronize(st));
  if (stat[mrg::kTrfStatBadRow] != mrg::kTrfNone)
    return fail(MRG_ERR_ARG, "%s: row %u: read, entry or start out of range", fn, stat[mrg::kTrfStatBadRow]);

  // ---- blocks, on the host (S x names cells): per sample by read_sum descending, then name descending; a group is a block
  // with a printed row, and the k-th group of a sample is paired with the name of the sample's k-th block
  struct Blk {
    uint32_t s, name, printed;
    int32_t rep;
    uint64_t sum;
  };
  std::vector<Blk> blk;
  for (uint32_t s = 0; s < S; ++s) {
    const size_t first = blk.size();
    for (uint32_t name = 0; name < n_names; ++name) {
      const uint64_t c = (uint64_t)s * n_names + name;
      if (h_rep[c] != 0x7F7F7F7F) blk.push_back(Blk{s, name, h_np[c], h_rep[c], h_sums[c]});
    }
    std::sort(blk.begin() + first, blk.end(), [](const Blk& a, const Blk& b) { return a.sum != b.sum ? a.sum > b.sum : a.name > b.name; });
  }
  const uint64_t B = blk.size();
  uint64_t G = 0, max_len = 0;
  for (const Blk& b : blk)
    if (b.printed) {
      ++G;
      max_len = std::max<uint64_t>(max_len, (uint64_t)std::max(entries[(uint64_t)b.rep * mrg::kTrfSampleInts + mrg::kTrfSampleTemplate], 0));
    }
  counts[0] = stat[mrg::kTrfStatItems];
  counts[1] = B;
  counts[2] = G;
  counts[3] = n_rows;
  counts[4] = G ? max_len : 1;   // (trf_samples.layout: max over the groups and 1)
  counts[5] = stat[mrg::kTrfStatHasN];
  counts[6] = stat[mrg::kTrfStatNoTemplate];
  counts[7] = stat[mrg::kTrfStatMaxLen];
  if (cap_blocks == 0) return MRG_OK;
  if (cap_blocks < B || cap_rows < n_rows)
    return fail(MRG_ERR_ARG, "%s: %llu blocks and %llu rows do not fit the buffers (count first)", fn, (unsigned long long)B,
                (unsigned long long)n_rows);
  if (stat[mrg::kTrfStatNoTemplate] != mrg::kTrfNone)
    return fail(MRG_ERR_ARG, "%s: row %u: the selected tRNA has no template", fn, stat[mrg::kTrfStatNoTemplate]);
  if (max_len > mrg::kTrfMaxTemplate)
    return fail(MRG_ERR_ARG, "%s: a template of %llu nt: density peaks take templates of at most %u nt", fn,
                (unsigned long long)max_len, mrg::kTrfMaxTemplate);
  if (counts[5] && !d_nmask_out) return fail(MRG_ERR_ARG, "%s: null output buffers", fn);
  std::vector<uint32_t> cell_block(cells, 0);
  {
    uint64_t g = 0, row = 0, b0 = 0, g_in_sample = 0;
    for (uint64_t b = 0; b < B; ++b) {
      if (b == 0 || blk[b].s != blk[b - 1].s) {
        b0 = b;
        g_in_sample = 0;
      }
      cell_block[(uint64_t)blk[b].s * n_names + blk[b].name] = (uint32_t)b;
      int32_t* o = blocks + b * 6;
      o[0] = (int32_t)blk[b].s;
      o[1] = blk[b].rep;
      o[2] = (int32_t)row;
      o[3] = (int32_t)blk[b].printed;
      o[4] = blk[b].printed ? (int32_t)g : -1;
      o[5] = 0;
      block_sums[b] = blk[b].sum;
      if (blk[b].printed) {
        groups[2 * g] = (int32_t)b;
        groups[2 * g + 1] = (int32_t)(b0 + g_in_sample);
        row += blk[b].printed;
        off[++g] = (uint32_t)row;
        ++g_in_sample;
      }
    }
    if (row != n_rows) return fail(MRG_ERR_HIP, "%s: the blocks hold %llu printed rows, the flags %u", fn, (unsigned long long)row, n_rows);
  }
  if (n_rows == 0) return MRG_OK;
  HIP_TRY(hipMemcpyAsync(ib.p + o_cb, cell_block.data(), cells * sizeof(uint32_t), hipMemcpyHostToDevice, st));

  // ---- the reads in Python string order: stable sorts of the rows by 21-base chunks, the last chunk first
  const uint32_t chunks = (stat[mrg::kTrfStatMaxLen] + 20) / 21, rank_bits = bits_for(K), block_bits = bits_for(B);
  if (8 + rank_bits > 64 || 32 + block_bits > 64) return fail(MRG_ERR_ARG, "%s: the sort keys do not fit 64 bits", fn);
  const uint64_t m = std::max<uint64_t>(K, n_rows);
  TrfBuf sb;
  const uint64_t o_k0 = sb.reserve(m * sizeof(uint64_t)), o_k1 = sb.reserve(m * sizeof(uint64_t)), o_v0 = sb.reserve(m * sizeof(uint32_t)),
                 o_v1 = sb.reserve(m * sizeof(uint32_t)), o_rank = sb.reserve((uint64_t)K * sizeof(uint32_t)),
                 o_item = sb.reserve((uint64_t)n_rows * sizeof(uint32_t)), o_tmp = sb.reserve(mrg::prims::radix_temp_bytes(m));
  HIP_TRY(sb.alloc());
  uint64_t* keys[2] = {sb.at<uint64_t>(o_k0), sb.at<uint64_t>(o_k1)};
  uint32_t* vals[2] = {sb.at<uint32_t>(o_v0), sb.at<uint32_t>(o_v1)};
  uint32_t *rank = sb.at<uint32_t>(o_rank), *item = sb.at<uint32_t>(o_item);
  HIP_TRY(mrg::trf_item_scatter_launch(flags, total, item, st));
  int cur = 0;
  auto sort = [&](uint32_t count, uint32_t bits) -> hipError_t {  // keys[cur], vals[cur] -> keys[cur], vals[cur] of the new cur
    bool second = false;
    const hipError_t e = mrg::prims::radix_sort_pairs_u64(keys[cur], keys[cur ^ 1], vals[cur], vals[cur ^ 1], count, bits, sb.p + o_tmp, st, &second);
    if (second) cur ^= 1;
    return e;
  };
  HIP_TRY(mrg::trf_iota_launch(vals[cur], K, st));
  for (uint32_t c = chunks; c-- > 0;) {
    HIP_TRY(mrg::trf_chunk_keys_launch(p, vals[cur], c, keys[cur], st));
    HIP_TRY(sort(K, 63));
  }
  HIP_TRY(mrg::trf_rank_scatter_launch(vals[cur], K, rank, st));
  if (kernel_ms) HIP_TRY(hipEventRecord(ev[2], st));

  // ---- the printed rows by (block, count descending, start descending, read descending): two stable passes
  HIP_TRY(mrg::trf_order_keys_a_launch(p, item, n_rows, rank, rank_bits, keys[cur], vals[cur], st));
  HIP_TRY(sort(n_rows, 8 + rank_bits));
  HIP_TRY(mrg::trf_order_keys_b_launch(p, item, vals[cur], n_rows, ib.at<uint32_t>(o_cb), keys[cur], st));
  HIP_TRY(sort(n_rows, 32 + block_bits));
  if (kernel_ms) HIP_TRY(hipEventRecord(ev[3], st));

  // ---- pack
  mrg::TrfPackOut out;
  out.words = (uint32_t)((counts[4] + 31) / 32);
  out.row_stride = cap_rows;
  out.codes = d_codes;
  out.nmask = counts[5] ? d_nmask_out : nullptr;
  out.span = d_span;
  out.rpm = d_rpm;
  out.row = d_rows;
  HIP_TRY(mrg::trf_pack_launch(p, item, vals[cur], n_rows, ib.at<uint64_t>(o_den), out, st));
  if (kernel_ms) HIP_TRY(hipEventRecord(ev[4], st));
  // (the tables were copied from pageable host memory, and the buffers above are freed on return)
  HIP_TRY(hipStreamSynchronize(st));
  if (kernel_ms)
    for (int i = 0; i < 4; ++i) HIP_TRY(hipEventElapsedTime(&kernel_ms[i], ev[i], ev[i + 1]));
  return MRG_OK;
}

int mrg_trf_rank(mrg_ctx* ctx, const uint32_t* off, uint32_t n_groups, const float* d_rho, uint32_t* d_rank, void* stream) {
  if (!ctx || !off || !n_groups) return fail(MRG_ERR_ARG, "mrg_trf_rank: null argument");
  if (n_groups > (1u << 24) || off[0] != 0) return fail(MRG_ERR_ARG, "mrg_trf_rank: 1..2^24 groups, off[0] = 0");
  for (uint32_t g = 0; g < n_groups; ++g)
    if (off[g + 1] < off[g]) return fail(MRG_ERR_ARG, "mrg_trf_rank: offsets decrease at group %u", g);
  const uint32_t n = off[n_groups];
  if (n && (!d_rho || !d_rank)) return fail(MRG_ERR_ARG, "mrg_trf_rank: null row buffers");
  if (n == 0) return MRG_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  TrfBuf b;
  const uint64_t o_off = b.reserve((n_groups + 1ull) * sizeof(uint32_t)), o_k0 = b.reserve((uint64_t)n * sizeof(uint64_t)),
                 o_k1 = b.reserve((uint64_t)n * sizeof(uint64_t)), o_v0 = b.reserve((uint64_t)n * sizeof(uint32_t)),
                 o_v1 = b.reserve((uint64_t)n * sizeof(uint32_t)), o_tmp = b.reserve(mrg::prims::radix_temp_bytes(n));
  HIP_TRY(b.alloc());
  HIP_TRY(hipMemcpyAsync(b.p + o_off, off, (n_groups + 1ull) * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  HIP_TRY(mrg::trf_rank_keys_launch(b.at<uint32_t>(o_off), n_groups, d_rho, n, b.at<uint64_t>(o_k0), b.at<uint32_t>(o_v0), st));
  bool second = false;
  HIP_TRY(mrg::prims::radix_sort_pairs_u64(b.at<uint64_t>(o_k0), b.at<uint64_t>(o_k1), b.at<uint32_t>(o_v0), b.at<uint32_t>(o_v1), n,
                                           32 + bits_for(n_groups), b.p + o_tmp, st, &second));
  HIP_TRY(mrg::trf_rank_local_launch(b.at<uint32_t>(o_off), b.at<uint64_t>(second ? o_k1 : o_k0), b.at<uint32_t>(second ? o_v1 : o_v0), n,
                                     d_rank, st));
  HIP_TRY(hipStreamSynchronize(st));
  return MRG_OK;
}

int mrg_write_trf_sample_reports(const char* const* paths, uint32_t n_samples, const uint64_t* denom, const uint64_t* reads,
                                 uint32_t words_per_read, uint64_t stride, const uint8_t* lens, const uint64_t* nmask, uint64_t n,
                                 const uint32_t* quant, const int32_t* rec, uint64_t k, const int32_t* entries,
                                 const char* const* entry_names, const char* const* templates, const char* const* aa_types,
                                 uint64_t n_entries, uint32_t n_names, const int32_t* blocks, const uint64_t* block_sums,
                                 uint64_t n_blocks, const uint32_t* rows, uint64_t n_rows) {
  const char* fn = "mrg_write_trf_sample_reports";
  if (!paths || !denom || !n_samples) return fail(MRG_ERR_ARG, "%s: null argument", fn);
  for (uint32_t s = 0; s < 2 * n_samples; ++s)
    if (!paths[s]) return fail(MRG_ERR_ARG, "%s: null argument", fn);
  if (k && (!reads || !lens || !quant || !rec)) return fail(MRG_ERR_ARG, "%s: null buffers", fn);
  if ((n_entries && (!entries || !entry_names || !templates || !aa_types)) || (n_blocks && (!blocks || !block_sums)) || (n_rows && !rows))
    return fail(MRG_ERR_ARG, "%s: null buffers", fn);
  if ((words_per_read != 1 && words_per_read != 2 && words_per_read != 4 && words_per_read != 8) || stride < n)
    return fail(MRG_ERR_ARG, "%s: bad words_per_read / stride", fn);
  return guarded(fn, [&] {
    const mrg::TrfSampleWriteArgs a{paths, n_samples, denom, reads, words_per_read, stride, lens, nmask, n, quant, rec, k, entries,
                                    entry_names, templates, aa_types, n_entries, n_names, blocks, block_sums, n_blocks, rows, n_rows};
    mrg::write_trf_sample_reports(a);
    return MRG_OK;
  });
}

// ------------------------------------------------------------- -tcf (csrc/collapsed_order.hip)
extern "C++" {
namespace {

struct SeqScratch {  // the caller's scratch, carved into 256-byte aligned pieces
  Piece<uint64_t> k0, k1;
  Piece<uint32_t> v0, v1, flags, stat;
  Piece<char> scan, sort;
  size_t total;
  // with_flags: the flags of a sample column and their scan (mrg_collapsed_order)
  SeqScratch(uint64_t n, bool with_flags) {
    Carver c(256, 1);
    k0 = c.take<uint64_t>(n);
    k1 = c.take<uint64_t>(n);
    v0 = c.take<uint32_t>(n);
    v1 = c.take<uint32_t>(n);
    if (with_flags) {
      flags = c.take<uint32_t>(n + 1);
      scan = c.take<char>(mrg::prims::scan_temp_bytes(n + 1));
    }
    sort = c.take<char>(mrg::prims::radix_temp_bytes(n));
    stat = c.take<uint32_t>(mrg::kSeqStatWords);
    total = c.total();
  }
};

}  // namespace
}  // extern "C++"

int mrg_collapsed_order_temp_bytes(uint64_t n, uint64_t* rank_bytes, uint64_t* order_bytes) {
  if (!rank_bytes || !order_bytes) return fail(MRG_ERR_ARG, "mrg_collapsed_order_temp_bytes: null argument");
  if (n >= (1ull << 31)) return fail(MRG_ERR_ARG, "mrg_collapsed_order_temp_bytes: %llu reads; the limit is 2^31 - 1", (unsigned long long)n);
  *rank_bytes = SeqScratch(n, false).total;
  *order_bytes = SeqScratch(n, true).total;
  return MRG_OK;
}

int mrg_seq_rank(mrg_ctx* ctx, const uint64_t* d_reads, uint32_t words_per_read, uint64_t stride, const uint8_t* d_lens,
                 const uint64_t* d_nmask, uint64_t n, uint32_t max_len, uint32_t* d_rank, void* d_tmp, uint64_t tmp_bytes, void* stream) {
  const char* fn = "mrg_seq_rank";
  if (!ctx || !d_reads || !d_lens || !d_rank || !d_tmp) return fail(MRG_ERR_ARG, "%s: null argument", fn);
  if (n == 0) return fail(MRG_ERR_ARG, "%s: no reads", fn);
  if (words_per_read != 1 && words_per_read != 2 && words_per_read != 4 && words_per_read != 8)
    return fail(MRG_ERR_ARG, "%s: words_per_read must be 1, 2, 4 or 8", fn);
  if (stride < n || n >= (1ull << 31)) return fail(MRG_ERR_ARG, "%s: bad stride / n", fn);
  if (max_len > 255 || max_len > 32 * words_per_read)
    return fail(MRG_ERR_ARG, "%s: max_len %u: at most 255 and what %u words hold", fn, max_len, words_per_read);
  const SeqScratch sc((uint64_t)n, false);
  if (int rc = scratch_ok(fn, d_tmp, tmp_bytes, sc.total, "mrg_collapsed_order_temp_bytes")) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  uint64_t* keys[2] = {sc.k0.at(d_tmp), sc.k1.at(d_tmp)};
  uint32_t* vals[2] = {sc.v0.at(d_tmp), sc.v1.at(d_tmp)};
  uint32_t* stat = sc.stat.at(d_tmp);
  HIP_TRY(hipMemsetAsync(stat, 0, mrg::kSeqStatWords * sizeof(uint32_t), st));
  mrg::SeqRankParams p;
  p.reads = d_reads;
  p.nmask = d_nmask;
  p.lens = d_lens;
  p.stride = stride;
  p.n = (uint32_t)n;
  p.W = words_per_read;
  p.max_len = max_len;
  // stable sorts by 21-base chunks, the last chunk first: as many launches as max_len asks for, whatever the reads hold
  const uint32_t chunks = std::max(1u, (max_len + mrg::kSeqChunkBases - 1) / mrg::kSeqChunkBases);
  int cur = 0;
  HIP_TRY(mrg::seq_iota_launch(vals[cur], p.n, st));
  for (uint32_t c = chunks; c-- > 0;) {
    const uint32_t width = std::min(mrg::kSeqChunkBases, max_len - mrg::kSeqChunkBases * c);
    HIP_TRY(mrg::seq_chunk_keys_launch(p, vals[cur], c, keys[cur], stat, st));
    bool second = false;
    HIP_TRY(mrg::prims::radix_sort_pairs_u64(keys[cur], keys[cur ^ 1], vals[cur], vals[cur ^ 1], p.n, 3 * width, sc.sort.at(d_tmp), st, &second));
    if (second) cur ^= 1;
  }
  HIP_TRY(mrg::seq_rank_scatter_launch(vals[cur], p.n, d_rank, st));
  uint32_t h_stat[mrg::kSeqStatWords] = {0, 0, 0, 0};
  if (int rc = read_stat(stat, h_stat, mrg::kSeqStatWords, st)) return rc;
  if (h_stat[mrg::kSeqStatTooLong]) return fail(MRG_ERR_ARG, "%s: a read is longer than max_len %u, or than its %u words hold", fn, max_len, words_per_read);
  return MRG_OK;
}

int mrg_collapsed_order(mrg_ctx* ctx, const uint32_t* d_quant, uint64_t n, uint32_t n_samples, uint32_t sample, const uint32_t* d_rank,
                        uint32_t* d_order, uint64_t cap, uint64_t* rows, void* d_tmp, uint64_t tmp_bytes, void* stream) {
  const char* fn = "mrg_collapsed_order";
  if (!ctx || !d_quant || !d_rank || !rows || !d_tmp) return fail(MRG_ERR_ARG, "%s: null argument", fn);
  *rows = 0;
  if (cap && !d_order) return fail(MRG_ERR_ARG, "%s: null output buffer", fn);
  if (n == 0 || n >= (1ull << 31)) return fail(MRG_ERR_ARG, "%s: 1 .. 2^31 - 1 reads", fn);
  if (n_samples == 0 || sample >= n_samples) return fail(MRG_ERR_ARG, "%s: sample %u of %u", fn, sample, n_samples);
  const SeqScratch sc(n, true);
  if (int rc = scratch_ok(fn, d_tmp, tmp_bytes, sc.total, "mrg_collapsed_order_temp_bytes")) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  uint64_t *k0 = sc.k0.at(d_tmp), *k1 = sc.k1.at(d_tmp);
  uint32_t *v0 = sc.v0.at(d_tmp), *v1 = sc.v1.at(d_tmp);
  uint32_t *flags = sc.flags.at(d_tmp), *stat = sc.stat.at(d_tmp);
  const uint32_t N = (uint32_t)n;
  // ---- the reads of the sample: flag, exclusive sums, scatter
  HIP_TRY(hipMemsetAsync(stat, 0, mrg::kSeqStatWords * sizeof(uint32_t), st));
  HIP_TRY(mrg::collapsed_flags_launch(d_quant, N, n_samples, sample, flags, stat, st));
  HIP_TRY(mrg::prims::exclusive_sum_u32(flags, flags, n + 1, sc.scan.at(d_tmp), st));
  uint32_t k = 0, h_stat[mrg::kSeqStatWords] = {0, 0, 0, 0};
  HIP_TRY(hipMemcpyAsync(&k, flags + n, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  if (int rc = read_stat(stat, h_stat, mrg::kSeqStatWords, st)) return rc;
  if (k > N) return fail(MRG_ERR_HIP, "%s: %u rows of %u reads", fn, k, N);
  *rows = k;
  if (cap < k) return fail(MRG_ERR_ARG, "%s: %u rows do not fit a buffer of %llu", fn, k, (unsigned long long)cap);
  if (k == 0) return MRG_OK;
  // ---- count << rank_bits | rank ascending, delivered backwards: only the bits the largest count and n - 1 occupy
  const uint32_t rank_bits = bits_for(n - 1), count_bits = bits_for(h_stat[mrg::kSeqStatMaxCount]);
  HIP_TRY(mrg::collapsed_keys_launch(flags, d_quant, N, n_samples, sample, d_rank, rank_bits, k0, v0, st));
  bool second = false;
  HIP_TRY(mrg::prims::radix_sort_pairs_u64(k0, k1, v0, v1, k, rank_bits + count_bits, sc.sort.at(d_tmp), st, &second));
  HIP_TRY(mrg::collapsed_reverse_launch(second ? v1 : v0, k, d_order, st));
  HIP_TRY(hipStreamSynchronize(st));
  return MRG_OK;
}

int64_t mrg_write_collapsed_fasta(const char* path, const uint64_t* reads, uint32_t words_per_read, uint64_t stride, const uint8_t* lens,
                                  const uint64_t* nmask, uint64_t n, const uint32_t* quant, uint32_t n_samples, uint32_t sample,
                                  const uint32_t* order, uint64_t k, const char* const* extra_seqs, const uint64_t* extra_counts,
                                  uint64_t n_extra) {
  const char* fn = "mrg_write_collapsed_fasta";
  if (!path) return fail(MRG_ERR_ARG, "%s: null argument", fn);
  if (k && (!reads || !lens || !quant || !order)) return fail(MRG_ERR_ARG, "%s: null buffers", fn);
  if (n_extra && (!extra_seqs || !extra_counts)) return fail(MRG_ERR_ARG, "%s: null extra rows", fn);
  if ((words_per_read != 1 && words_per_read != 2 && words_per_read != 4 && words_per_read != 8) || stride < n)
    return fail(MRG_ERR_ARG, "%s: bad words_per_read / stride", fn);
  if (n_samples == 0 || sample >= n_samples) return fail(MRG_ERR_ARG, "%s: sample %u of %u", fn, sample, n_samples);
  return guarded(fn, [&] {
    const mrg::CollapsedFaArgs a{path, reads, words_per_read, stride, lens, nmask, n, quant, n_samples, sample, order, k,
                                 extra_seqs, extra_counts, n_extra};
    return (int64_t)mrg::write_collapsed_fasta(a);
  });
}

// ------------------------------------------------------------- predict mode's candidate reads (csrc/predict_reads.hip)
extern "C++" {
namespace {

struct PredictScratch {  // the caller's scratch, carved into 256-byte aligned pieces
  Piece<uint32_t> raw, sel, stat;
  Piece<char> scan;
  size_t total;
  explicit PredictScratch(uint64_t n) {
    Carver c(256, 1);
    raw = c.take<uint32_t>(n + 1);
    sel = c.take<uint32_t>(n + 1);
    scan = c.take<char>(mrg::prims::scan_temp_bytes(n + 1));
    stat = c.take<uint32_t>(mrg::kPredictStatWords);
    total = c.total();
  }
};

}  // namespace
}  // extern "C++"

int mrg_predict_reads_temp_bytes(uint64_t n, uint64_t* bytes) {
  if (!bytes) return fail(MRG_ERR_ARG, "mrg_predict_reads_temp_bytes: null argument");
  if (n >= (1ull << 31)) return fail(MRG_ERR_ARG, "mrg_predict_reads_temp_bytes: %llu reads; the limit is 2^31 - 1", (unsigned long long)n);
  *bytes = PredictScratch(n).total;
  return MRG_OK;
}

int mrg_predict_select(mrg_ctx* ctx, const int8_t* d_pass_id, const uint8_t* d_lens, const uint32_t* d_quant, uint64_t n,
                       uint32_t n_samples, uint32_t min_len, uint32_t max_len, uint64_t count_cutoff, uint64_t* d_total,
                       uint32_t* d_raw_no, uint32_t* d_sel_no, uint64_t* n_raw, uint64_t* n_sel, void* d_tmp, uint64_t tmp_bytes,
                       void* stream) {
  const char* fn = "mrg_predict_select";
  if (!ctx || !n_raw || !n_sel || !d_tmp) return fail(MRG_ERR_ARG, "%s: null argument", fn);
  *n_raw = *n_sel = 0;
  if (n && (!d_pass_id || !d_lens || !d_quant || !d_total || !d_raw_no || !d_sel_no)) return fail(MRG_ERR_ARG, "%s: null buffers", fn);
  if (n >= (1ull << 31)) return fail(MRG_ERR_ARG, "%s: %llu reads; the limit is 2^31 - 1", fn, (unsigned long long)n);
  if (n_samples == 0) return fail(MRG_ERR_ARG, "%s: no sample column", fn);
  if (min_len > max_len) return fail(MRG_ERR_ARG, "%s: the length window %u .. %u is empty", fn, min_len, max_len);
  if (count_cutoff == 0) return fail(MRG_ERR_ARG, "%s: the count cutoff must be at least 1", fn);
  const PredictScratch sc(n);
  if (int rc = scratch_ok(fn, d_tmp, tmp_bytes, sc.total, "mrg_predict_reads_temp_bytes")) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  uint32_t *raw = sc.raw.at(d_tmp), *sel = sc.sel.at(d_tmp);
  mrg::PredictSelectParams p;
  p.pass_id = d_pass_id;
  p.lens = d_lens;
  p.quant = d_quant;
  p.n = (uint32_t)n;
  p.S = n_samples;
  p.min_len = min_len;
  p.max_len = max_len;
  p.cutoff = count_cutoff;
  HIP_TRY(mrg::predict_flags_launch(p, d_total, raw, sel, st));
  HIP_TRY(mrg::prims::exclusive_sum_u32(raw, raw, n + 1, sc.scan.at(d_tmp), st));
  HIP_TRY(mrg::prims::exclusive_sum_u32(sel, sel, n + 1, sc.scan.at(d_tmp), st));
  HIP_TRY(mrg::predict_numbers_launch(raw, sel, p.n, d_raw_no, d_sel_no, st));
  uint32_t k[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(&k[0], raw + n, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(&k[1], sel + n, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (k[0] > n || k[1] > k[0]) return fail(MRG_ERR_HIP, "%s: %u raw and %u filtered rows of %llu reads", fn, k[0], k[1], (unsigned long long)n);
  *n_raw = k[0];
  *n_sel = k[1];
  return MRG_OK;
}

int mrg_predict_sample_reads(mrg_ctx* ctx, const uint32_t* d_quant, uint64_t n, uint32_t n_samples, uint32_t sample,
                             const uint32_t* d_no, uint64_t threshold, uint32_t* d_idx, uint32_t* d_num, uint32_t* d_cnt, uint64_t cap,
                             uint64_t* rows, void* d_tmp, uint64_t tmp_bytes, void* stream) {
  const char* fn = "mrg_predict_sample_reads";
  if (!ctx || !rows || !d_tmp) return fail(MRG_ERR_ARG, "%s: null argument", fn);
  *rows = 0;
  if (n && (!d_quant || !d_no)) return fail(MRG_ERR_ARG, "%s: null buffers", fn);
  if (cap && (!d_idx || !d_num || !d_cnt)) return fail(MRG_ERR_ARG, "%s: null output buffer", fn);
  if (n >= (1ull << 31)) return fail(MRG_ERR_ARG, "%s: %llu reads; the limit is 2^31 - 1", fn, (unsigned long long)n);
  if (n_samples == 0 || sample >= n_samples) return fail(MRG_ERR_ARG, "%s: sample %u of %u", fn, sample, n_samples);
  if (threshold == 0) return fail(MRG_ERR_ARG, "%s: the threshold must be at least 1", fn);
  const PredictScratch sc(n);
  if (int rc = scratch_ok(fn, d_tmp, tmp_bytes, sc.total, "mrg_predict_reads_temp_bytes")) return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  uint32_t* flags = sc.raw.at(d_tmp);
  const uint32_t N = (uint32_t)n;
  // ---- count: flag, exclusive sums
  HIP_TRY(mrg::predict_sample_flags_launch(d_quant, d_no, N, n_samples, sample, threshold, flags, st));
  HIP_TRY(mrg::prims::exclusive_sum_u32(flags, flags, n + 1, sc.scan.at(d_tmp), st));
  uint32_t k = 0;
  HIP_TRY(hipMemcpyAsync(&k, flags + n, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (k > N) return fail(MRG_ERR_HIP, "%s: %u rows of %u reads", fn, k, N);
  *rows = k;
  if (cap < k) return fail(MRG_ERR_ARG, "%s: %u rows do not fit a buffer of %llu", fn, k, (unsigned long long)cap);
  if (k == 0) return MRG_OK;
  // ---- fill: scatter in array order
  HIP_TRY(mrg::predict_sample_fill_launch(flags, d_quant, d_no, N, n_samples, sample, d_idx, d_num, d_cnt, st));
  HIP_TRY(hipStreamSynchronize(st));
  return MRG_OK;
}

int mrg_predict_gather(mrg_ctx* ctx, const uint64_t* d_reads, uint32_t words_per_read, uint64_t stride, const uint8_t* d_lens,
                       const uint64_t* d_nmask, uint64_t n, const uint32_t* d_quant, uint32_t n_samples, uint32_t sample,
                       const uint32_t* d_idx, uint64_t k, uint64_t* d_out_reads, uint8_t* d_out_lens, uint64_t* d_out_nmask,
                       uint32_t* d_out_counts, void* d_tmp, uint64_t tmp_bytes, void* stream) {
  const char* fn = "mrg_predict_gather";
  if (!ctx || !d_tmp) return fail(MRG_ERR_ARG, "%s: null argument", fn);
  if (k && (!d_reads || !d_lens || !d_quant || !d_idx || !d_out_reads || !d_out_lens || !d_out_counts))
    return fail(MRG_ERR_ARG, "%s: null buffers", fn);
  if (words_per_read != 1 && words_per_read != 2 && words_per_read != 4 && words_per_read != 8)
    return fail(MRG_ERR_ARG, "%s: words_per_read must be 1, 2, 4 or 8", fn);
  if (stride < n || n >= (1ull << 31) || k > n) return fail(MRG_ERR_ARG, "%s: bad stride / n / k", fn);
  if (n_samples == 0 || (sample >= n_samples && sample != mrg::kPredictTotalAll)) return fail(MRG_ERR_ARG, "%s: sample %u of %u", fn, sample, n_samples);
  const PredictScratch sc(n);
  if (int rc = scratch_ok(fn, d_tmp, tmp_bytes, sc.total, "mrg_predict_reads_temp_bytes")) return rc;
  if (k == 0) return MRG_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  uint32_t* stat = sc.stat.at(d_tmp);
  HIP_TRY(hipMemsetAsync(stat, 0, mrg::kPredictStatWords * sizeof(uint32_t), st));
  mrg::PredictGatherParams p;
  p.reads = d_reads;
  p.nmask = d_nmask;
  p.lens = d_lens;
  p.quant = d_quant;
  p.idx = d_idx;
  p.stride = stride;
  p.n = (uint32_t)n;
  p.W = words_per_read;
  p.S = n_samples;
  p.sample = sample;
  p.k = (uint32_t)k;
  p.out_reads = d_out_reads;
  p.out_nmask = d_out_nmask;
  p.out_lens = d_out_lens;
  p.out_counts = d_out_counts;
  HIP_TRY(mrg::predict_gather_launch(p, stat, st));
  uint32_t h_stat[mrg::kPredictStatWords] = {0, 0, 0, 0};
  if (int rc = read_stat(stat, h_stat, mrg::kPredictStatWords, st)) return rc;
  if (h_stat[mrg::kPredictStatBadIndex]) return fail(MRG_ERR_ARG, "%s: an index is no read of %llu", fn, (unsigned long long)n);
  if (h_stat[mrg::kPredictStatTooLong]) return fail(MRG_ERR_ARG, "%s: a read is longer than its %u words hold", fn, words_per_read);
  if (h_stat[mrg::kPredictStatOverflow]) return fail(MRG_ERR_ARG, "%s: a read's total count does not fit 32 bits", fn);
  return MRG_OK;
}

int64_t mrg_write_predict_fasta(const char* path, const uint64_t* reads, uint32_t words_per_read, uint64_t stride, const uint8_t* lens,
                                const uint64_t* nmask, uint64_t n, const uint32_t* idx, const uint32_t* num, const void* counts,
                                uint32_t count_bytes, uint64_t k, const char* const* extra_seqs, const uint64_t* extra_nums,
                                const uint64_t* extra_counts, uint64_t n_extra) {
  const char* fn = "mrg_write_predict_fasta";
  if (!path) return fail(MRG_ERR_ARG, "%s: null argument", fn);
  if (k && (!reads || !lens || !idx || !num || !counts)) return fail(MRG_ERR_ARG, "%s: null buffers", fn);
  if (n_extra && (!extra_seqs || !extra_nums || !extra_counts)) return fail(MRG_ERR_ARG, "%s: null extra rows", fn);
  if ((words_per_read != 1 && words_per_read != 2 && words_per_read != 4 && words_per_read != 8) || stride < n)
    return fail(MRG_ERR_ARG, "%s: bad words_per_read / stride", fn);
  if (count_bytes != 4 && count_bytes != 8) return fail(MRG_ERR_ARG, "%s: count_bytes must be 4 or 8", fn);
  return guarded(fn, [&] {
    const mrg::PredictFastaArgs a{path, reads, words_per_read, stride, lens, nmask, n, idx, num, counts, count_bytes, k,
                                  extra_seqs, extra_nums, extra_counts, n_extra};
    return (int64_t)mrg::write_predict_fasta(a);
  });
}

int mrg_predict_read_names(const uint32_t* num, const void* counts, uint32_t count_bytes, uint64_t k, char* blob, uint64_t blob_cap,
                           uint64_t* offsets, uint64_t* blob_bytes) {
  const char* fn = "mrg_predict_read_names";
  if (!offsets || !blob_bytes) return fail(MRG_ERR_ARG, "%s: null argument", fn);
  *blob_bytes = 0;
  if (k && (!num || !counts)) return fail(MRG_ERR_ARG, "%s: null buffers", fn);
  if (count_bytes != 4 && count_bytes != 8) return fail(MRG_ERR_ARG, "%s: count_bytes must be 4 or 8", fn);
  *blob_bytes = mrg::predict_read_names(num, counts, count_bytes, k, blob, blob_cap, offsets);
  if (blob && blob_cap < *blob_bytes) return fail(MRG_ERR_ARG, "%s: %llu bytes of names do not fit a buffer of %llu", fn,
                                                  (unsigned long long)*blob_bytes, (unsigned long long)blob_cap);
  return MRG_OK;
}

// ------------------------------------------------------------- -ai
// The kernels trust the tables: every target id is -1 or a target, every target has at most 32 bases.  MRG_OK or the failure.
static int a2i_check_tables(const char* fn, const int32_t* canon_target, uint64_t n_canon, const int32_t* isomir_target,
                            uint64_t n_isomir, const uint64_t* target_words, const uint8_t* target_lens, uint64_t n_targets) {
  for (int t = 0; t < 2; ++t) {
    const int32_t* tab = t ? isomir_target : canon_target;
    const uint64_t len = t ? n_isomir : n_canon;
    for (uint64_t e = 0; e < len; ++e)
      if (tab[e] < -1 || (tab[e] >= 0 && (uint64_t)tab[e] >= n_targets))
        return fail(MRG_ERR_ARG, "%s: entry %llu of the %s table names target %d of %llu", fn, (unsigned long long)e,
                    t ? "isomiR" : "canonical", tab[e], (unsigned long long)n_targets);
  }
  for (uint64_t t = 0; t < n_targets; ++t) {
    if (target_lens[t] > 32) return fail(MRG_ERR_ARG, "%s: target %llu has %u bases (at most 32)", fn, (unsigned long long)t, target_lens[t]);
    if (target_lens[t] < 32 && (target_words[t] >> (2 * target_lens[t])) != 0)
      return fail(MRG_ERR_ARG, "%s: target %llu holds bits beyond its length", fn, (unsigned long long)t);
  }
  return MRG_OK;
}

int mrg_a2i_align(mrg_ctx* ctx, const uint64_t* d_reads, uint32_t words_per_read, uint64_t stride, const uint8_t* d_lens,
                  const uint64_t* d_nmask, uint64_t n, const int8_t* d_pass_id, const int32_t* d_ref_id, const uint8_t* d_keep,
                  int32_t canon_pass, int32_t isomir_pass, const int32_t* canon_target, uint64_t n_canon,
                  const int32_t* isomir_target, uint64_t n_isomir, const uint64_t* target_words, const uint8_t* target_lens,
                  uint64_t n_targets, uint32_t from_base, uint32_t to_base, uint64_t cap, uint32_t* d_idx, int32_t* d_rec,
                  uint64_t* counts, float* kernel_ms, void* stream) {
  if (!ctx || !counts) return fail(MRG_ERR_ARG, "mrg_a2i_align: null argument");
  if (kernel_ms) *kernel_ms = 0.0f;
  if (n && (!d_reads || !d_lens || !d_pass_id || !d_ref_id)) return fail(MRG_ERR_ARG, "mrg_a2i_align: null buffers");
  if ((n_canon && !canon_target) || (n_isomir && !isomir_target) || (n_targets && (!target_words || !target_lens)))
    return fail(MRG_ERR_ARG, "mrg_a2i_align: null tables");
  if (cap && (!d_idx || !d_rec)) return fail(MRG_ERR_ARG, "mrg_a2i_align: null output buffers");
  if (((uintptr_t)d_rec & 15u) != 0) return fail(MRG_ERR_ARG, "mrg_a2i_align: d_rec must be 16-byte aligned");
  if (words_per_read != 1 && words_per_read != 2 && words_per_read != 4 && words_per_read != 8)
    return fail(MRG_ERR_ARG, "mrg_a2i_align: words_per_read must be 1, 2, 4 or 8");
  if (stride < n || n >= (1ull << 31)) return fail(MRG_ERR_ARG, "mrg_a2i_align: bad stride / n");
  if (canon_pass == isomir_pass || canon_pass < 0 || isomir_pass < 0 || canon_pass > 127 || isomir_pass > 127)
    return fail(MRG_ERR_ARG, "mrg_a2i_align: the two passes must differ and lie in 0..127");
  if (from_base > 3 || to_base > 3) return fail(MRG_ERR_ARG, "mrg_a2i_align: from_base / to_base are codes 0..3");
  if (n_canon >= (1ull << 31) || n_isomir >= (1ull << 31) || n_targets >= (1ull << 31))
    return fail(MRG_ERR_ARG, "mrg_a2i_align: tables too large");
  if (int rc = a2i_check_tables("mrg_a2i_align", canon_target, n_canon, isomir_target, n_isomir, target_words, target_lens, n_targets))
    return rc;
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  counts[0] = 0;
  if (n == 0) return MRG_OK;
  // context scratch: [canon table | isomiR table | target words | target lengths | flags -> offsets (n + 1) | scan scratch]
  auto up = [](uint64_t b) { return (b + 255) & ~255ull; };
  const uint64_t n_flags = n + 1;
  const uint64_t o_canon = 0, o_iso = o_canon + up(n_canon * sizeof(int32_t)), o_tw = o_iso + up(n_isomir * sizeof(int32_t)),
                 o_tl = o_tw + up(n_targets * sizeof(uint64_t)), o_flags = o_tl + up(n_targets),
                 o_tmp = o_flags + up(n_flags * sizeof(uint32_t)), need_bytes = o_tmp + up(mrg::prims::scan_temp_bytes(n_flags));
  if (ctx->scratch_bytes < need_bytes) {
    HIP_TRY(hipStreamSynchronize(st));
    (void)hipFree(ctx->scratch);
    ctx->scratch = nullptr;
    ctx->scratch_bytes = 0;
    HIP_TRY(hipMalloc(&ctx->scratch, need_bytes));
    ctx->scratch_bytes = need_bytes;
  }
  char* base = (char*)ctx->scratch;
  uint32_t* flags = (uint32_t*)(base + o_flags);
  // select and order: the exclusive sums of the flags are the rows (as mrg_isomir_classify; one list, in array order)
  HIP_TRY(mrg::a2i_flags_launch(d_pass_id, d_keep, n, canon_pass, isomir_pass, flags, st));
  HIP_TRY(mrg::prims::exclusive_sum_u32(flags, flags, n_flags, base + o_tmp, st));
  uint32_t total = 0;
  HIP_TRY(hipMemcpyAsync(&total, flags + n, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  counts[0] = total;
  const uint64_t rows = std::min<uint64_t>(total, cap);
  if (rows == 0) return MRG_OK;
  HIP_TRY(mrg::a2i_scatter_launch(d_pass_id, d_keep, n, canon_pass, isomir_pass, flags, cap, d_idx, st));
  if (n_canon) HIP_TRY(hipMemcpyAsync(base + o_canon, canon_target, n_canon * sizeof(int32_t), hipMemcpyHostToDevice, st));
  if (n_isomir) HIP_TRY(hipMemcpyAsync(base + o_iso, isomir_target, n_isomir * sizeof(int32_t), hipMemcpyHostToDevice, st));
  if (n_targets) {
    HIP_TRY(hipMemcpyAsync(base + o_tw, target_words, n_targets * sizeof(uint64_t), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(base + o_tl, target_lens, n_targets, hipMemcpyHostToDevice, st));
  }
  mrg::A2iAlignParams p;
  p.reads = d_reads;
  p.nmask = d_nmask;
  p.lens = d_lens;
  p.pass_id = d_pass_id;
  p.ref_id = d_ref_id;
  p.idx = d_idx;
  p.rows = (uint32_t)rows;
  p.canon_pass = canon_pass;
  p.canon_target = (const int32_t*)(base + o_canon);
  p.n_canon = (uint32_t)n_canon;
  p.isomir_target = (const int32_t*)(base + o_iso);
  p.n_isomir = (uint32_t)n_isomir;
  p.target_words = (const uint64_t*)(base + o_tw);
  p.target_lens = (const uint8_t*)(base + o_tl);
  p.n_targets = (uint32_t)n_targets;
  p.from_base = from_base;
  p.to_base = to_base;
  p.rec = d_rec;
  // kernel_ms: a2i_align_kernel alone, between two events on the stream
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  hipError_t e = hipSuccess;
  if (kernel_ms) {
    e = hipEventCreate(&ev0);
    if (e == hipSuccess) e = hipEventCreate(&ev1);
    if (e == hipSuccess) e = hipEventRecord(ev0, st);
  }
  if (e == hipSuccess) e = mrg::a2i_align_launch(p, st);
  if (e == hipSuccess && kernel_ms) e = hipEventRecord(ev1, st);
  // (the tables were copied from pageable host memory, which the caller may free on return)
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e == hipSuccess && kernel_ms) e = hipEventElapsedTime(kernel_ms, ev0, ev1);
  if (ev0) (void)hipEventDestroy(ev0);
  if (ev1) (void)hipEventDestroy(ev1);
  HIP_TRY(e);
  return MRG_OK;
}

int mrg_a2i_settle(mrg_ctx* ctx, const uint64_t* d_reads, uint32_t words_per_read, uint64_t stride, const uint8_t* d_lens,
                   const uint64_t* d_nmask, uint64_t n, const int32_t* canon_target, uint64_t n_canon, const int32_t* isomir_target,
                   uint64_t n_isomir, const uint64_t* target_words, const uint8_t* target_lens, uint64_t n_targets,
                   uint32_t from_base, uint32_t to_base, uint64_t k, const uint32_t* d_idx, int32_t* d_rec, uint64_t* counts,
                   float* kernel_ms, void* stream) {
  if (!counts) return fail(MRG_ERR_ARG, "mrg_a2i_settle: null argument");
  if (kernel_ms) *kernel_ms = 0.0f;
  if (k && (!d_reads || !d_lens || !d_idx || !d_rec)) return fail(MRG_ERR_ARG, "mrg_a2i_settle: null buffers");
  if ((n_canon && !canon_target) || (n_isomir && !isomir_target) || (n_targets && (!target_words || !target_lens)))
    return fail(MRG_ERR_ARG, "mrg_a2i_settle: null tables");
  if (((uintptr_t)d_rec & 15u) != 0) return fail(MRG_ERR_ARG, "mrg_a2i_settle: d_rec must be 16-byte aligned");
  if (words_per_read != 1 && words_per_read != 2 && words_per_read != 4 && words_per_read != 8)
    return fail(MRG_ERR_ARG, "mrg_a2i_settle: words_per_read must be 1, 2, 4 or 8");
  if (stride < n || n >= (1ull << 31) || k >= (1ull << 31)) return fail(MRG_ERR_ARG, "mrg_a2i_settle: bad stride / n / k");
  if (from_base > 3 || to_base > 3) return fail(MRG_ERR_ARG, "mrg_a2i_settle: from_base / to_base are codes 0..3");
  if (n_canon >= (1ull << 31) || n_isomir >= (1ull << 31) || n_targets >= (1ull << 31))
    return fail(MRG_ERR_ARG, "mrg_a2i_settle: tables too large");
  if (int rc = a2i_check_tables("mrg_a2i_settle", canon_target, n_canon, isomir_target, n_isomir, target_words, target_lens, n_targets))
    return rc;
  // (the context last: what is wrong with the arguments is said on a machine without a device too)
  if (!ctx) return fail(MRG_ERR_ARG, "mrg_a2i_settle: null context (the rows are settled on the device, there is no host route)");
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  counts[0] = counts[1] = 0;
  if (k == 0 || n == 0 || n_targets == 0) return MRG_OK;
  // context scratch: [target words | target lengths | rows settled | flags -> offsets (k + 1) | the rows of status 1 | scan scratch]
  auto up = [](uint64_t b) { return (b + 255) & ~255ull; };
  const uint64_t n_flags = k + 1;
  const uint64_t o_tw = 0, o_tl = o_tw + up(n_targets * sizeof(uint64_t)), o_done = o_tl + up(n_targets),
                 o_flags = o_done + up(sizeof(uint32_t)), o_sel = o_flags + up(n_flags * sizeof(uint32_t)),
                 o_tmp = o_sel + up(k * sizeof(uint32_t)), need_bytes = o_tmp + up(mrg::prims::scan_temp_bytes(n_flags));
  if (ctx->scratch_bytes < need_bytes) {
    HIP_TRY(hipStreamSynchronize(st));
    (void)hipFree(ctx->scratch);
    ctx->scratch = nullptr;
    ctx->scratch_bytes = 0;
    HIP_TRY(hipMalloc(&ctx->scratch, need_bytes));
    ctx->scratch_bytes = need_bytes;
  }
  char* base = (char*)ctx->scratch;
  uint32_t* flags = (uint32_t*)(base + o_flags);
  HIP_TRY(mrg::a2i_tied_select_launch(d_rec, k, flags, st));
  HIP_TRY(mrg::prims::exclusive_sum_u32(flags, flags, n_flags, base + o_tmp, st));
  uint32_t total = 0;
  HIP_TRY(hipMemcpyAsync(&total, flags + k, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  counts[0] = total;
  if (total == 0) return MRG_OK;
  HIP_TRY(mrg::a2i_tied_scatter_launch(d_rec, k, flags, (uint32_t*)(base + o_sel), st));
  HIP_TRY(hipMemcpyAsync(base + o_tw, target_words, n_targets * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(base + o_tl, target_lens, n_targets, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(base + o_done, 0, sizeof(uint32_t), st));
  mrg::A2iSettleParams p;
  p.reads = d_reads;
  p.nmask = d_nmask;
  p.lens = d_lens;
  p.n_reads = n;
  p.idx = d_idx;
  p.rec = d_rec;
  p.sel = (const uint32_t*)(base + o_sel);
  p.n_sel = total;
  p.target_words = (const uint64_t*)(base + o_tw);
  p.target_lens = (const uint8_t*)(base + o_tl);
  p.n_targets = (uint32_t)n_targets;
  p.from_base = from_base;
  p.to_base = to_base;
  p.settled = (uint32_t*)(base + o_done);
  // kernel_ms: a2i_settle_kernel alone, between two events on the stream
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  hipError_t e = hipSuccess;
  if (kernel_ms) {
    e = hipEventCreate(&ev0);
    if (e == hipSuccess) e = hipEventCreate(&ev1);
    if (e == hipSuccess) e = hipEventRecord(ev0, st);
  }
  if (e == hipSuccess) e = mrg::a2i_settle_launch(p, st);
  if (e == hipSuccess && kernel_ms) e = hipEventRecord(ev1, st);
  uint32_t done = 0;
  if (e == hipSuccess) e = hipMemcpyAsync(&done, base + o_done, sizeof(uint32_t), hipMemcpyDeviceToHost, st);
  // (the tables were copied from pageable host memory, which the caller may free on return)
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e == hipSuccess && kernel_ms) e = hipEventElapsedTime(kernel_ms, ev0, ev1);
  if (ev0) (void)hipEventDestroy(ev0);
  if (ev1) (void)hipEventDestroy(ev1);
  HIP_TRY(e);
  counts[1] = done;
  return MRG_OK;
}

int mrg_write_a2i_detail(const char* path, const uint64_t* reads, uint32_t words_per_read, uint64_t stride, const uint8_t* lens,
                         const uint64_t* nmask, uint64_t n, uint64_t n_blocks, const uint64_t* block_off, const int32_t* block_group,
                         const int32_t* block_frame, const char* const* block_text, const char* const* group_names,
                         const char* const* group_targets, uint64_t n_groups, const uint32_t* row_read, const uint32_t* row_count,
                         const uint8_t* row_flags, const int32_t* row_d, uint64_t* lines) {
  if (!path || !block_off) return fail(MRG_ERR_ARG, "mrg_write_a2i_detail: null argument");
  if (n_blocks && (!block_group || !block_frame || !group_names || !group_targets))
    return fail(MRG_ERR_ARG, "mrg_write_a2i_detail: null block tables");
  if (block_off[n_blocks] && (!reads || !lens || !row_read || !row_count || !row_flags || !row_d))
    return fail(MRG_ERR_ARG, "mrg_write_a2i_detail: null buffers");
  if ((words_per_read != 1 && words_per_read != 2 && words_per_read != 4 && words_per_read != 8) || stride < n)
    return fail(MRG_ERR_ARG, "mrg_write_a2i_detail: bad words_per_read / stride");
  for (uint64_t g = 0; g < n_groups; ++g)
    if (!group_names[g] || !group_targets[g]) return fail(MRG_ERR_ARG, "mrg_write_a2i_detail: null group name / target");
  return guarded("mrg_write_a2i_detail", [&] {
    const mrg::A2iDetailArgs a{path, reads, words_per_read, stride, lens, nmask, n, n_blocks, block_off, block_group, block_frame,
                               block_text, group_names, group_targets, n_groups, row_read, row_count, row_flags, row_d};
    mrg::write_a2i_detail(a, lines);
    return MRG_OK;
  });
}

// ------------------------------------------------------------- packing
int mrg_pack_reads(const char* const* seqs, uint64_t n, uint32_t words_per_read, uint64_t* reads,
                   uint8_t* lens, uint64_t* nmask, int* has_n) {
  if ((n && (!seqs || !reads || !lens)) || words_per_read == 0 || words_per_read > MRG_MAX_WORDS)
    return fail(MRG_ERR_ARG, "mrg_pack_reads: bad argument");
  int any_n = 0;
  for (uint64_t r = 0; r < n; ++r) {
    const char* s = seqs[r];
    size_t L = std::strlen(s);
    if (L > (size_t)words_per_read * 32)
      return fail(MRG_ERR_ARG, "mrg_pack_reads: read %llu has %zu nt, more than %u words hold",
                  (unsigned long long)r, L, words_per_read);
    lens[r] = (uint8_t)L;
    for (uint32_t w = 0; w < words_per_read; ++w) {
      reads[(size_t)w * n + r] = 0;
      if (nmask) nmask[(size_t)w * n + r] = 0;
    }
    for (size_t i = 0; i < L; ++i) {
      uint64_t code = 0;
      bool isn = false;
      switch (s[i]) {
        case 'A': case 'a': code = 0; break;
        case 'C': case 'c': code = 1; break;
        case 'G': case 'g': code = 2; break;
        case 'T': case 't': code = 3; break;
        default: isn = true; break;
      }
      reads[(size_t)(i >> 5) * n + r] |= code << ((i & 31) * 2);
      if (isn) {
        any_n = 1;
        if (nmask) nmask[(size_t)(i >> 5) * n + r] |= 1ull << ((i & 31) * 2);
      }
    }
  }
  if (has_n) *has_n = any_n;
  return MRG_OK;
}

// the ragged form of mrg_cascade_run_long: read r = words[word_off[r] .. word_off[r + 1]), ceil(len / 32) words
static int pack_ragged(const char* const* seqs, uint64_t n, uint64_t* words, uint64_t* nmask, uint64_t* word_off, uint32_t* lens,
                       int* has_n) {
  int any_n = 0;
  uint64_t at = 0;
  for (uint64_t r = 0; r < n; ++r) {
    const char* s = seqs[r];
    const size_t L = std::strlen(s);
    if (L > 0x7fffffffull) return fail(MRG_ERR_ARG, "mrg_pack_reads_ragged: read %llu is too long", (unsigned long long)r);
    const uint64_t nw = (L + 31) / 32;
    if (word_off) word_off[r] = at;
    if (lens) lens[r] = (uint32_t)L;
    if (words) {
      for (uint64_t w = 0; w < nw; ++w) {
        words[at + w] = 0;
        if (nmask) nmask[at + w] = 0;
      }
      for (size_t i = 0; i < L; ++i) {
        uint64_t code = 0;
        bool isn = false;
        switch (s[i]) {
          case 'A': case 'a': code = 0; break;
          case 'C': case 'c': code = 1; break;
          case 'G': case 'g': code = 2; break;
          case 'T': case 't': code = 3; break;
          default: isn = true; break;
        }
        words[at + (i >> 5)] |= code << ((i & 31) * 2);
        if (isn) {
          any_n = 1;
          if (nmask) nmask[at + (i >> 5)] |= 1ull << ((i & 31) * 2);
        }
      }
    }
    at += nw;
  }
  if (word_off) word_off[n] = at;
  if (has_n) *has_n = any_n;
  return MRG_OK;
}

int mrg_pack_reads_ragged(const char* const* seqs, uint64_t n, uint64_t* words, uint64_t* nmask, uint64_t* word_off,
                          uint32_t* lens, int* has_n) {
  if (n && !seqs) return fail(MRG_ERR_ARG, "mrg_pack_reads_ragged: null argument");
  if (!word_off) return fail(MRG_ERR_ARG, "mrg_pack_reads_ragged: word_off is required");
  return pack_ragged(seqs, n, words, nmask, word_off, lens, has_n);
}

int mrg_fastq_copy_long(const mrg_fastq* fq, uint64_t* words, uint64_t* nmask, uint64_t* word_off, uint32_t* lens, int* has_n) {
  if (!fq || !word_off) return fail(MRG_ERR_ARG, "mrg_fastq_copy_long: null argument");
  const auto& lr = fq->d.long_reads;
  std::vector<const char*> ptrs(lr.size());
  for (size_t i = 0; i < lr.size(); ++i) ptrs[i] = lr[i].c_str();
  return pack_ragged(ptrs.data(), lr.size(), words, nmask, word_off, lens, has_n);
}

}  // extern "C"

// ---------------------------------------------------------------- -trf density peaks (csrc/trf_peaks.hip)
namespace {

// Checks what the three calls share and uploads the launch metadata -- row offsets, the block list (most work
// first: a rho / border block scans its whole group, a delta block the rank positions before its end), bord_off
// and the rho call's kernel table -- in one device buffer, *meta, that trf_finish frees.
int trf_prepare(const char* fn, mrg_ctx* ctx, const uint32_t* off, uint32_t n_groups, uint32_t max_len,
                const uint64_t* d_codes, const uint64_t* d_nmask, const uint16_t* d_span, bool by_rank,
                const uint32_t* bord_off, const double* ktab, uint32_t n_ktab, mrg::TrfLaunch* L, void** meta,
                const void** extra) {
  if (!ctx || !off || !n_groups) return fail(MRG_ERR_ARG, "%s: null argument", fn);
  if (max_len < 1 || max_len > 255)
    return fail(MRG_ERR_ARG, "%s: templates of 1..255 nt (got %u): a longer tRNA cannot be clustered", fn, max_len);
  if (n_groups > (1u << 24) || off[0] != 0) return fail(MRG_ERR_ARG, "%s: 1..2^24 groups, off[0] = 0", fn);
  for (uint32_t g = 0; g < n_groups; ++g)
    if (off[g + 1] < off[g] || (bord_off && bord_off[g + 1] < bord_off[g]))
      return fail(MRG_ERR_ARG, "%s: offsets decrease at group %u", fn, g);
  if (off[n_groups] && (!d_codes || !d_span)) return fail(MRG_ERR_ARG, "%s: null row buffers", fn);
  const uint32_t T = mrg::kTrfTile;
  std::vector<uint2> blocks;
  for (uint32_t g = 0; g < n_groups; ++g)
    if (!bord_off || bord_off[g + 1] - bord_off[g] >= 3)  // (border pass: only NCLUST > 1)
      for (uint32_t t = 0; t < off[g + 1] - off[g]; t += T) blocks.push_back(make_uint2(g, t));
  auto work = [&](const uint2& b) {
    const uint64_t n = off[b.x + 1] - off[b.x];
    return by_rank ? std::min<uint64_t>(n, (uint64_t)b.y + T) : n;
  };
  std::stable_sort(blocks.begin(), blocks.end(), [&](const uint2& a, const uint2& b) { return work(a) > work(b); });
  const size_t n_off = (n_groups + 1) * sizeof(uint32_t), at_bl = (n_off + 15) & ~(size_t)15;
  const size_t at_x = at_bl + ((blocks.size() * sizeof(uint2) + 15) & ~(size_t)15);
  const size_t n_x = bord_off ? n_off : n_ktab * sizeof(double);
  std::vector<uint8_t> host(at_x + n_x);
  std::memcpy(host.data(), off, n_off);
  if (!blocks.empty()) std::memcpy(host.data() + at_bl, blocks.data(), blocks.size() * sizeof(uint2));
  if (n_x) std::memcpy(host.data() + at_x, bord_off ? (const void*)bord_off : (const void*)ktab, n_x);
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipMalloc(meta, host.size()));
  const hipError_t e = hipMemcpy(*meta, host.data(), host.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess) (void)hipFree(*meta);
  HIP_TRY(e);
  const uint8_t* m = (const uint8_t*)*meta;
  *L = mrg::TrfLaunch{(const uint32_t*)m, (const uint2*)(m + at_bl), (uint32_t)blocks.size(), off[n_groups],
                      (max_len + 31) / 32, d_codes, d_nmask, d_span, nullptr};
  *extra = m + at_x;
  return MRG_OK;
}

int trf_finish(void* meta, hipError_t e, hipStream_t st) {
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  (void)hipFree(meta);
  HIP_TRY(e);
  return MRG_OK;
}

}  // namespace

extern "C" {

int mrg_trf_rho(mrg_ctx* ctx, const uint32_t* off, uint32_t n_groups, uint32_t max_len, const uint64_t* d_codes,
                const uint64_t* d_nmask, const uint16_t* d_span, const double* d_rpm, const double* ktab, uint32_t n_ktab,
                float* d_rho, uint32_t* d_max_dis, void* stream) {
  if (!ktab || !n_ktab || n_ktab > mrg::kTrfKtabMax)
    return fail(MRG_ERR_ARG, "mrg_trf_rho: a kernel table of 1..%u entries is required", mrg::kTrfKtabMax);
  if (!d_max_dis || (off && n_groups && off[n_groups] && (!d_rpm || !d_rho)))
    return fail(MRG_ERR_ARG, "mrg_trf_rho: null output buffers");
  mrg::TrfLaunch L;
  void* meta = nullptr;
  const void* kt = nullptr;
  int rc = trf_prepare("mrg_trf_rho", ctx, off, n_groups, max_len, d_codes, d_nmask, d_span, false, nullptr, ktab,
                       n_ktab, &L, &meta, &kt);
  if (rc != MRG_OK) return rc;
  L.rpm = d_rpm;
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(d_max_dis, 0, n_groups * sizeof(uint32_t), st);
  if (e == hipSuccess) e = mrg::trf_rho_launch(L, (const double*)kt, n_ktab, d_rho, d_max_dis, st);
  return trf_finish(meta, e, st);
}

int mrg_trf_delta(mrg_ctx* ctx, const uint32_t* off, uint32_t n_groups, uint32_t max_len, const uint64_t* d_codes,
                  const uint64_t* d_nmask, const uint16_t* d_span, const uint32_t* d_rank, const uint32_t* d_max_dis,
                  int32_t* d_delta, int32_t* d_nneigh, void* stream) {
  if (!d_max_dis || (off && n_groups && off[n_groups] && (!d_rank || !d_delta || !d_nneigh)))
    return fail(MRG_ERR_ARG, "mrg_trf_delta: null rank / output buffers");
  mrg::TrfLaunch L;
  void* meta = nullptr;
  const void* unused = nullptr;
  int rc = trf_prepare("mrg_trf_delta", ctx, off, n_groups, max_len, d_codes, d_nmask, d_span, true, nullptr, nullptr,
                       0, &L, &meta, &unused);
  if (rc != MRG_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  return trf_finish(meta, mrg::trf_delta_launch(L, d_rank, d_max_dis, d_delta, d_nneigh, st), st);
}

int mrg_trf_border(mrg_ctx* ctx, const uint32_t* off, uint32_t n_groups, uint32_t max_len, const uint64_t* d_codes,
                   const uint64_t* d_nmask, const uint16_t* d_span, const float* d_rho, const int32_t* d_label,
                   const uint32_t* bord_off, float* d_bord, void* stream) {
  if (!bord_off) return fail(MRG_ERR_ARG, "mrg_trf_border: null argument");
  if (off && n_groups && (bord_off[0] != 0 || (off[n_groups] && (!d_rho || !d_label)) || (bord_off[n_groups] && !d_bord)))
    return fail(MRG_ERR_ARG, "mrg_trf_border: bord_off[0] != 0, or null rho / label / output buffers");
  mrg::TrfLaunch L;
  void* meta = nullptr;
  const void* bo = nullptr;
  int rc = trf_prepare("mrg_trf_border", ctx, off, n_groups, max_len, d_codes, d_nmask, d_span, false, bord_off,
                       nullptr, 0, &L, &meta, &bo);
  if (rc != MRG_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = bord_off[n_groups] ? hipMemsetAsync(d_bord, 0, bord_off[n_groups] * sizeof(float), st) : hipSuccess;
  if (e == hipSuccess) e = mrg::trf_border_launch(L, d_rho, d_label, (const uint32_t*)bo, d_bord, st);
  return trf_finish(meta, e, st);
}

// ---------------------------------------------------------------- -trf centres, labels, halos (csrc/trf_labels.hip)
static int trf_check_off(const char* fn, const uint32_t* off, uint32_t n_groups) {
  if (n_groups > (1u << 24) || off[0] != 0) return fail(MRG_ERR_ARG, "%s: 1..2^24 groups, off[0] = 0", fn);
  for (uint32_t g = 0; g < n_groups; ++g)
    if (off[g + 1] < off[g]) return fail(MRG_ERR_ARG, "%s: offsets decrease at group %u", fn, g);
  return MRG_OK;
}

int mrg_trf_assign(mrg_ctx* ctx, const uint32_t* off, uint32_t n_groups, const float* d_rho, const uint32_t* d_rank,
                   const int32_t* d_delta, const int32_t* d_nneigh, int32_t* d_label, uint32_t* nclust, uint64_t cap_centers,
                   uint32_t* cen_off, uint32_t* centers, void* stream) {
  const char* fn = "mrg_trf_assign";
  if (!ctx || !off || !n_groups || !nclust || !cen_off) return fail(MRG_ERR_ARG, "%s: null argument", fn);
  if (int rc = trf_check_off(fn, off, n_groups)) return rc;
  const uint32_t n = off[n_groups], G = n_groups;
  if (n && (!d_rho || !d_rank || !d_delta || !d_nneigh || !d_label)) return fail(MRG_ERR_ARG, "%s: null row buffers", fn);
  if (cap_centers && !centers) return fail(MRG_ERR_ARG, "%s: null centre buffer", fn);
  if (n == 0) {
    std::memset(nclust, 0, G * sizeof(uint32_t));
    std::memset(cen_off, 0, (G + 1ull) * sizeof(uint32_t));
    return MRG_OK;
  }
  uint32_t largest = 1;
  for (uint32_t g = 0; g < G; ++g) largest = std::max(largest, off[g + 1] - off[g]);
  const uint32_t rounds = bits_for(largest - 1) + 1;  // ceil(log2(largest group)) + 1: a chain has fewer steps than rows
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  TrfBuf b;
  const uint64_t o_off = b.reserve((G + 1ull) * 4), o_grp = b.reserve(n * 4ull), o_zero = b.reserve(0), o_gdelta = b.reserve(G * 4ull),
                 o_grho = b.reserve(G * 4ull), o_err = b.reserve(4), o_fb = b.reserve(G * 4ull), o_flags = b.reserve((n + 1ull) * 4),
                 o_ncl = b.reserve((G + 1ull) * 4), o_lab0 = b.reserve(n * 4ull), o_lab1 = b.reserve(n * 4ull),
                 o_nxt0 = b.reserve(n * 4ull), o_nxt1 = b.reserve(n * 4ull), o_cen = b.reserve(n * 4ull),
                 o_tmp = b.reserve(std::max(mrg::prims::scan_temp_bytes(n + 1ull), mrg::prims::scan_temp_bytes(G + 1ull)));
  HIP_TRY(b.alloc());
  HIP_TRY(hipMemcpyAsync(b.p + o_off, off, (G + 1ull) * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(b.p + o_zero, 0, o_fb - o_zero, st));  // gdelta, grho, err
  HIP_TRY(hipMemsetAsync(b.p + o_fb, 0xFF, G * 4ull, st));
  const mrg::TrfAssignIn in{b.at<uint32_t>(o_off), G, n, d_rho, d_rank, d_delta, d_nneigh};
  uint32_t *grp = b.at<uint32_t>(o_grp), *gdelta = b.at<uint32_t>(o_gdelta), *grho = b.at<uint32_t>(o_grho), *err = b.at<uint32_t>(o_err),
           *fb = b.at<uint32_t>(o_fb), *flags = b.at<uint32_t>(o_flags), *ncl = b.at<uint32_t>(o_ncl), *cen = b.at<uint32_t>(o_cen);
  int32_t* lab[2] = {b.at<int32_t>(o_lab0), b.at<int32_t>(o_lab1)};
  uint32_t* nxt[2] = {b.at<uint32_t>(o_nxt0), b.at<uint32_t>(o_nxt1)};
  HIP_TRY(mrg::trf_assign_stats_launch(in, grp, gdelta, grho, err, st));
  HIP_TRY(mrg::trf_assign_flags_launch(in, grp, gdelta, flags, st));
  HIP_TRY(mrg::prims::exclusive_sum_u32(flags, flags, n + 1ull, b.p + o_tmp, st));
  HIP_TRY(mrg::trf_assign_fallback_launch(in, grp, flags, gdelta, grho, fb, st));
  HIP_TRY(mrg::trf_assign_nclust_launch(in, flags, fb, ncl, st));
  HIP_TRY(mrg::prims::exclusive_sum_u32(ncl, ncl, G + 1ull, b.p + o_tmp, st));
  HIP_TRY(mrg::trf_assign_init_launch(in, grp, flags, fb, ncl, lab[0], nxt[0], cen, err, st));
  int cur = 0;
  for (uint32_t r = 0; r < rounds; ++r, cur ^= 1) HIP_TRY(mrg::trf_assign_round_launch(in, grp, lab[cur], nxt[cur], lab[cur ^ 1], nxt[cur ^ 1], st));
  HIP_TRY(mrg::trf_assign_finish_launch(n, lab[cur], d_label, err, st));
  uint32_t h_err = 0;
  std::vector<uint32_t> h_off(G + 1ull);
  HIP_TRY(hipMemcpyAsync(&h_err, err, 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(h_off.data(), ncl, (G + 1ull) * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (h_err) {
    HIP_TRY(hipMemsetAsync(d_label, 0, n * 4ull, st));  // (0 is no label)
    HIP_TRY(hipStreamSynchronize(st));
    return fail(MRG_ERR_ARG, "%s: %s", fn,
                (h_err & mrg::kTrfErrTop)         ? "the first rank entry of a group is none of its rows"
                : (h_err & mrg::kTrfErrNeighbour) ? "a nneigh lies outside its group"
                                                  : "the nneigh of some rows form a cycle");
  }
  const uint64_t total = h_off[G];
  if (total > n) return fail(MRG_ERR_HIP, "%s: more centres than rows", fn);
  if (total && cap_centers >= total) {
    HIP_TRY(hipMemcpyAsync(centers, cen, total * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  std::memcpy(cen_off, h_off.data(), (G + 1ull) * 4);
  for (uint32_t g = 0; g < G; ++g) nclust[g] = h_off[g + 1] - h_off[g];
  return MRG_OK;
}

int mrg_trf_halo(mrg_ctx* ctx, const uint32_t* off, uint32_t n_groups, uint32_t max_len, const uint64_t* d_codes,
                 const uint64_t* d_nmask, const uint16_t* d_span, const float* d_rho, const int32_t* d_label,
                 const uint32_t* d_counts, uint32_t count_stride, const uint32_t* cen_off, const uint32_t* centers,
                 const uint32_t* bord_off, const float* d_bord, uint8_t* d_core, uint32_t* d_order, uint64_t* tallies,
                 void* stream) {
  const char* fn = "mrg_trf_halo";
  if (!ctx || !off || !n_groups || !cen_off || !bord_off) return fail(MRG_ERR_ARG, "%s: null argument", fn);
  if (max_len < 1 || max_len > 255) return fail(MRG_ERR_ARG, "%s: templates of 1..255 nt (got %u)", fn, max_len);
  if (int rc = trf_check_off(fn, off, n_groups)) return rc;
  const uint32_t n = off[n_groups], G = n_groups;
  if (n && (!d_codes || !d_span || !d_rho || !d_label || !d_counts || !d_core || !d_order || !count_stride))
    return fail(MRG_ERR_ARG, "%s: null row buffers", fn);
  if (cen_off[0] != 0 || bord_off[0] != 0) return fail(MRG_ERR_ARG, "%s: cen_off[0] = bord_off[0] = 0", fn);
  uint32_t most = 0;
  for (uint32_t g = 0; g < G; ++g)  // (all of them first: centers[] is as long as cen_off[n_groups] says)
    if (cen_off[g + 1] < cen_off[g] || bord_off[g + 1] < bord_off[g]) return fail(MRG_ERR_ARG, "%s: offsets decrease at group %u", fn, g);
  for (uint32_t g = 0; g < G; ++g) {
    const uint32_t nc = cen_off[g + 1] - cen_off[g], size = off[g + 1] - off[g];
    if (nc > size) return fail(MRG_ERR_ARG, "%s: group %u has more centres than rows", fn, g);
    if (nc && !centers) return fail(MRG_ERR_ARG, "%s: null centres", fn);
    for (uint32_t c = 0; c < nc; ++c)
      if (centers[cen_off[g] + c] >= size) return fail(MRG_ERR_ARG, "%s: a centre of group %u is none of its rows", fn, g);
    if (nc > 1 && bord_off[g + 1] - bord_off[g] != nc + 1)
      return fail(MRG_ERR_ARG, "%s: group %u needs NCLUST + 1 border slots", fn, g);
    most = std::max(most, nc);
  }
  const uint32_t C_all = cen_off[G];
  if ((C_all && !tallies) || (bord_off[G] && !d_bord)) return fail(MRG_ERR_ARG, "%s: null tally / border buffers", fn);
  if (n == 0) return MRG_OK;
  const uint32_t slot_bits = bits_for(most), key_bits = slot_bits + bits_for(G);
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  TrfBuf b;
  const uint64_t o_off = b.reserve((G + 1ull) * 4), o_coff = b.reserve((G + 1ull) * 4), o_boff = b.reserve((G + 1ull) * 4),
                 o_cen = b.reserve(C_all * 4ull), o_zero = b.reserve(0), o_tally = b.reserve(C_all * 32ull), o_err = b.reserve(4),
                 o_k0 = b.reserve(n * 8ull), o_k1 = b.reserve(n * 8ull), o_v0 = b.reserve(n * 4ull), o_v1 = b.reserve(n * 4ull),
                 o_tmp = b.reserve(mrg::prims::radix_temp_bytes(n));
  HIP_TRY(b.alloc());
  HIP_TRY(hipMemcpyAsync(b.p + o_off, off, (G + 1ull) * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(b.p + o_coff, cen_off, (G + 1ull) * 4, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(b.p + o_boff, bord_off, (G + 1ull) * 4, hipMemcpyHostToDevice, st));
  if (C_all) HIP_TRY(hipMemcpyAsync(b.p + o_cen, centers, C_all * 4ull, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(b.p + o_zero, 0, o_k0 - o_zero, st));  // tallies, err
  const mrg::TrfHaloIn in{b.at<uint32_t>(o_off), G, n, n, (max_len + 31) / 32, d_codes, d_nmask, d_span, d_rho, d_label, d_counts,
                          count_stride, b.at<uint32_t>(o_coff), b.at<uint32_t>(o_cen), b.at<uint32_t>(o_boff), d_bord};
  HIP_TRY(mrg::trf_halo_launch(in, slot_bits, d_core, b.at<unsigned long long>(o_tally), b.at<uint64_t>(o_k0), b.at<uint32_t>(o_v0),
                               b.at<uint32_t>(o_err), st));
  bool second = false;
  HIP_TRY(mrg::prims::radix_sort_pairs_u64(b.at<uint64_t>(o_k0), b.at<uint64_t>(o_k1), b.at<uint32_t>(o_v0), b.at<uint32_t>(o_v1), n,
                                           key_bits, b.p + o_tmp, st, &second));
  HIP_TRY(hipMemcpyAsync(d_order, b.p + (second ? o_v1 : o_v0), n * 4ull, hipMemcpyDeviceToDevice, st));
  uint32_t h_err = 0;
  std::vector<uint64_t> h_tally(4ull * C_all);
  HIP_TRY(hipMemcpyAsync(&h_err, b.p + o_err, 4, hipMemcpyDeviceToHost, st));
  if (C_all) HIP_TRY(hipMemcpyAsync(h_tally.data(), b.p + o_tally, C_all * 32ull, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (h_err) return fail(MRG_ERR_ARG, "%s: a label names no cluster of its group", fn);
  if (C_all) std::memcpy(tallies, h_tally.data(), C_all * 32ull);
  return MRG_OK;
}

int mrg_write_trf_cluster_reports(const char* const* paths, uint32_t n_samples, const uint64_t* codes, const uint64_t* nmask,
                                  uint32_t max_len, uint64_t stride, const uint16_t* span, const double* rpm, const uint32_t* rows,
                                  uint64_t n_rows, const uint32_t* off, uint32_t n_groups, const int32_t* group_sample,
                                  const int32_t* group_len, const char* const* group_names, const char* const* group_keys,
                                  const char* const* group_mature, const char* const* group_trailer, const int32_t* labels,
                                  const uint8_t* core, const uint32_t* order, const uint32_t* nclust, const uint32_t* cen_off,
                                  const uint32_t* centers, const uint64_t* tallies, int64_t* status) {
  const char* fn = "mrg_write_trf_cluster_reports";
  if (!paths || !n_samples || !off || !status) return fail(MRG_ERR_ARG, "%s: null argument", fn);
  for (uint32_t s = 0; s < 2 * n_samples; ++s)
    if (!paths[s]) return fail(MRG_ERR_ARG, "%s: null argument", fn);
  if (n_groups && (!group_sample || !group_len || !group_names || !group_keys || !group_mature || !group_trailer || !nclust || !cen_off))
    return fail(MRG_ERR_ARG, "%s: null group tables", fn);
  if (n_rows && (!codes || !span || !rpm || !rows || !labels || !core || !order)) return fail(MRG_ERR_ARG, "%s: null row buffers", fn);
  if (max_len < 1 || max_len > 255 || stride < n_rows || n_rows >= (1ull << 32)) return fail(MRG_ERR_ARG, "%s: bad max_len / stride", fn);
  if (off[0] != 0) return fail(MRG_ERR_ARG, "%s: off[0] = 0", fn);
  for (uint32_t g = 0; g < n_groups; ++g)
    if (off[g + 1] < off[g]) return fail(MRG_ERR_ARG, "%s: offsets decrease at group %u", fn, g);
  if (off[n_groups] != n_rows) return fail(MRG_ERR_ARG, "%s: the offsets do not cover the rows", fn);
  if (n_groups && cen_off[n_groups] && (!centers || !tallies)) return fail(MRG_ERR_ARG, "%s: null centres / tallies", fn);
  status[0] = status[1] = 0;
  return guarded(fn, [&] {
    const mrg::TrfClusterWriteArgs a{paths, n_samples, codes, nmask, max_len, stride, span, rpm, rows, n_rows, off, n_groups,
                                     group_sample, group_len, group_names, group_keys, group_mature, group_trailer, labels, core,
                                     order, nclust, cen_off, centers, tallies, status};
    mrg::write_trf_cluster_reports(a);
    return MRG_OK;
  });
}

int mrg_py3_float_repr(double value, char* out, uint64_t cap) {
  if (!out || cap < 32) return fail(MRG_ERR_ARG, "mrg_py3_float_repr: a buffer of at least 32 bytes is required");
  const std::string s = mrg::py3_float_repr(value);
  if (s.size() + 1 > cap) return fail(MRG_ERR_ARG, "mrg_py3_float_repr: buffer too small");
  std::memcpy(out, s.c_str(), s.size() + 1);
  return MRG_OK;
}

}  // extern "C"
