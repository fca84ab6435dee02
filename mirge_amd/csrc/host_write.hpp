// What the host-side report writers share (no GPU): the output file, the thread rule, the ordered scheduler and the unpacking
// of a packed read.  A writer checks its arguments, opens its files, formats tasks [0, n) with in_batches and closes.  Rounds
// of tasks are formatted by worker threads and flushed in task order on the calling thread, so the bytes a writer produces
// depend on neither the thread count nor its block size.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <exception>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

namespace mrg {

// a stdio file that throws: "cannot open", "short write to", "cannot close"; the destructor closes without a word
struct File {
  FILE* f = nullptr;
  std::string path;
  explicit File(const char* p, const char* mode = "wb") : path(p) {
    f = std::fopen(p, mode);
    if (!f) throw std::runtime_error("cannot open " + path);
  }
  File(const File&) = delete;
  File& operator=(const File&) = delete;
  ~File() {
    if (f) std::fclose(f);
  }
  void write(const char* p, size_t n) {
    if (n && std::fwrite(p, 1, n, f) != n) throw std::runtime_error("short write to " + path);
  }
  void write(const std::string& s) { write(s.data(), s.size()); }
  void close() {
    FILE* x = f;
    f = nullptr;
    if (x && std::fclose(x) != 0) throw std::runtime_error("cannot close " + path);
  }
  std::string read_all() {
    std::string out;
    char buf[1 << 16];
    size_t got;
    while ((got = std::fread(buf, 1, sizeof buf, f)) > 0) out.append(buf, got);
    if (std::ferror(f)) throw std::runtime_error("cannot read " + path);
    return out;
  }
};

// the worker threads of a writer with n_tasks independent tasks: min(16, cores), or the environment's count clamped to
// [1, 16]; never more than the tasks
inline unsigned writer_threads(uint64_t n_tasks) {
  int n = (int)std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  if (const char* e = std::getenv("MIRGE_AMD_TABLE_THREADS")) n = std::max(1, std::min(16, std::atoi(e)));
  return (unsigned)std::min<uint64_t>((uint64_t)n, std::max<uint64_t>(n_tasks, 1));
}

// a count from the environment (the writers' block sizes, lowered by tests): at least 1; dflt where the variable is unset
inline uint64_t env_count(const char* name, uint64_t dflt) {
  const char* e = std::getenv(name);
  return e ? (uint64_t)std::max(1, std::atoi(e)) : dflt;
}

// tasks [0, n) on up to n_threads workers, n_threads at a time; after each batch `flush(first, live)` runs on the caller
template <class Work, class Flush>
void in_batches(uint64_t n, unsigned n_threads, Work work, Flush flush) {
  n_threads = (unsigned)std::min<uint64_t>(n_threads, std::max<uint64_t>(n, 1));
  std::vector<std::exception_ptr> failed(n_threads);
  for (uint64_t t0 = 0; t0 < n; t0 += n_threads) {
    const unsigned live = (unsigned)std::min<uint64_t>(n_threads, n - t0);
    auto run = [&](unsigned t) {
      try {
        failed[t] = nullptr;
        work(t, t0 + t);
      } catch (...) {
        failed[t] = std::current_exception();
      }
    };
    if (live == 1) {
      run(0);
    } else {
      std::vector<std::thread> pool;
      try {
        for (unsigned t = 0; t < live; ++t) pool.emplace_back(run, t);
      } catch (...) {
        for (auto& th : pool) th.join();
        throw;
      }
      for (auto& th : pool) th.join();
    }
    for (unsigned t = 0; t < live; ++t)
      if (failed[t]) std::rethrow_exception(failed[t]);
    flush(t0, live);
  }
}

// the letter of a 2-bit base code
inline char base_char(uint64_t code) { return "ACGT"[code & 3]; }

// bases [first, last) of read u of the columnar 2-bit arrays (word i / 32 of read u at reads[(i / 32) * stride + u], an N where
// nmask, if given, has the low bit of the base's pair set) into out
inline void unpack_read(const uint64_t* reads, const uint64_t* nmask, uint64_t stride, uint64_t u, uint32_t first, uint32_t last,
                        char* out) {
  for (uint32_t i = first; i < last; ++i) {
    const uint64_t w = (uint64_t)(i >> 5) * stride + u;
    const bool is_n = nmask && ((nmask[w] >> ((i & 31) * 2)) & 1ull);
    *out++ = is_n ? 'N' : base_char(reads[w] >> ((i & 31) * 2));
  }
}
// the first L bases
inline void unpack_read(const uint64_t* reads, const uint64_t* nmask, uint64_t stride, uint64_t u, uint32_t L, char* out) {
  unpack_read(reads, nmask, stride, u, 0, L, out);
}
// the first L bases appended to out
inline void unpack_read(const uint64_t* reads, const uint64_t* nmask, uint64_t stride, uint64_t u, uint32_t L, std::string& out) {
  const size_t at = out.size();
  out.resize(at + L);
  unpack_read(reads, nmask, stride, u, 0, L, &out[at]);
}

inline void append_int(std::string& out, long long v) {
  char num[24];
  const int len = std::snprintf(num, sizeof num, "%lld", v);
  out.append(num, (size_t)len);
}

}  // namespace mrg
