// Stand-alone check of mirge_amd/csrc/host_write.hpp (TEST INFRASTRUCTURE; built and run by tests/test_host_write.py):
//   host_write_check <an existing, writable directory>
// prints the first expectation that fails and returns 1; prints "host_write ok" and returns 0 otherwise.
#include "host_write.hpp"

#include <atomic>
#include <cstring>

namespace {

#define EXPECT(cond)                                                  \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
      std::exit(1);                                                   \
    }                                                                 \
  } while (0)

const uint64_t kNoThrow = ~0ull;

// in_batches over n tasks on T threads; task `bad` throws (after it has counted itself)
void check_in_batches(uint64_t n, unsigned T, uint64_t bad) {
  std::vector<std::atomic<int>> ran(n);
  std::vector<std::atomic<unsigned>> slot(n);
  for (uint64_t i = 0; i < n; ++i) {
    ran[i] = 0;
    slot[i] = ~0u;
  }
  std::atomic<uint64_t> counter{0};
  std::atomic<bool> out_of_range{false};
  const std::thread::id caller = std::this_thread::get_id();
  uint64_t next = 0;  // the first task no flush has covered
  bool thrown = false;
  try {
    mrg::in_batches(n, T,
                    [&](unsigned t, uint64_t task) {
                      if (task >= n || t >= T) {
                        out_of_range = true;
                        return;
                      }
                      ++ran[task];
                      slot[task] = t;
                      ++counter;
                      if (task == bad) throw std::runtime_error("task " + std::to_string(task));
                    },
                    [&](uint64_t first, unsigned live) {
                      EXPECT(std::this_thread::get_id() == caller);
                      EXPECT(first == next);
                      EXPECT(live >= 1 && live <= T && first + live <= n);
                      EXPECT(bad == kNoThrow || first + live <= bad);  // neither the batch of the throw nor a later one
                      for (uint64_t i = 0; i < n; ++i) {  // the batch and those before it have run once, nothing behind it has started
                        EXPECT(ran[i] == (i < first + live ? 1 : 0));
                        if (i >= first && i < first + live) EXPECT(slot[i] == (unsigned)(i - first));
                      }
                      next = first + live;
                    });
  } catch (const std::runtime_error& e) {
    thrown = true;
    EXPECT(bad != kNoThrow && e.what() == "task " + std::to_string(bad));
  }
  EXPECT(!out_of_range);
  EXPECT(thrown == (bad != kNoThrow));
  if (bad == kNoThrow) {
    EXPECT(next == n && counter == n);
    for (uint64_t i = 0; i < n; ++i) EXPECT(ran[i] == 1);
  } else {
    // every batch in front of the throwing one was flushed; its own tasks all ran and were joined, none behind it started
    const uint64_t first = bad / T * T;
    EXPECT(next == first);
    const uint64_t expected = std::min<uint64_t>(n, first + T);
    EXPECT(counter == expected);
    for (int i = 0; i < 100; ++i) std::this_thread::yield();
    EXPECT(counter == expected);
  }
}

void check_scheduler() {
  for (unsigned T : {1u, 2u, 16u}) {
    for (uint64_t n : {(uint64_t)0, (uint64_t)1, (uint64_t)T - 1, (uint64_t)T, (uint64_t)T + 1, (uint64_t)3 * T + 2}) check_in_batches(n, T, kNoThrow);
    const uint64_t n = 3 * T + 2;
    check_in_batches(n, T, T / 2);      // first batch
    check_in_batches(n, T, T + T / 2);  // a middle batch
    check_in_batches(n, T, n - 1);      // last batch
  }
  // more threads asked for than tasks
  check_in_batches(3, 16, kNoThrow);
  check_in_batches(3, 16, 1);
}

void check_env() {
  const char* kThreads = "MIRGE_AMD_TABLE_THREADS";
  const char* kCount = "MIRGE_AMD_HOST_WRITE_CHECK_COUNT";
  const unsigned hw = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  struct Case {
    const char* value;  // null: unset
    unsigned threads;   // before the cap by the tasks
    uint64_t count;     // env_count with default 7
  };
  const Case cases[] = {{nullptr, hw, 7}, {"0", 1, 1}, {"-3", 1, 1}, {"5", 5, 5}, {"16", 16, 16}, {"99", 16, 99}, {"abc", 1, 1}};
  for (const Case& c : cases) {
    for (const char* name : {kThreads, kCount}) {
      if (c.value) setenv(name, c.value, 1);
      else unsetenv(name);
    }
    for (uint64_t n_tasks : {(uint64_t)0, (uint64_t)1, (uint64_t)3, (uint64_t)16, (uint64_t)17, (uint64_t)1 << 40}) {
      const unsigned got = mrg::writer_threads(n_tasks);
      EXPECT(got >= 1 && got <= 16 && got <= std::max<uint64_t>(n_tasks, 1));
      EXPECT(got == std::min<uint64_t>(c.threads, std::max<uint64_t>(n_tasks, 1)));
    }
    EXPECT(mrg::env_count(kCount, 7) == c.count);
  }
  unsetenv(kThreads);
  unsetenv(kCount);
}

std::string slurp(const std::string& path) {
  mrg::File in(path.c_str(), "rb");
  return in.read_all();
}

void check_file(const std::string& dir) {
  {
    const std::string path = dir + "/no-such-directory/out.txt";
    bool thrown = false;
    try {
      mrg::File f(path.c_str());
    } catch (const std::runtime_error& e) {
      thrown = true;
      EXPECT(std::string(e.what()) == "cannot open " + path);
    }
    EXPECT(thrown);
  }
  const std::string hello = std::string("hello\0world\n", 12);
  {
    const std::string path = dir + "/closed.bin";
    mrg::File f(path.c_str());
    f.write(hello);
    f.write(std::string());  // nothing
    f.write(nullptr, 0);     // nothing
    f.write("tail", 4);
    f.close();
    EXPECT(slurp(path) == hello + "tail");
  }
  {
    const std::string path = dir + "/dropped.bin";
    {
      mrg::File f(path.c_str());
      f.write(hello);
    }
    EXPECT(slurp(path) == hello);
  }
  {
    const std::string path = dir + "/empty.bin";
    mrg::File f(path.c_str());
    f.write(std::string());
    f.close();
    EXPECT(slurp(path).empty());
  }
  {  // larger than read_all's 64 KiB buffer, and no multiple of it
    const std::string path = dir + "/large.bin";
    std::string big(3 * 65536 + 4321, '\0');
    for (size_t i = 0; i < big.size(); ++i) big[i] = (char)(i * 131 + (i >> 9));
    mrg::File f(path.c_str());
    f.write(big);
    f.close();
    EXPECT(slurp(path) == big);
  }
}

void check_unpack() {
  const uint64_t stride = 3, u = 1, W = 8;
  std::vector<uint64_t> reads(W * stride), nmask(W * stride, 0);
  uint64_t x = 0x9e3779b97f4a7c15ull;
  for (uint64_t& w : reads) {  // xorshift64
    x ^= x << 13;
    x ^= x >> 7;
    x ^= x << 17;
    w = x;
  }
  for (uint32_t L : {0u, 1u, 31u, 32u, 33u, 64u, 255u}) {
    for (uint64_t w = 0; w < W; ++w)
      for (uint64_t r = 0; r < stride; ++r) nmask[w * stride + r] = r == u ? 0 : 0x5555555555555555ull;  // the neighbours are all N
    for (uint32_t p : {0u, 31u, 32u, L - 1})
      if (p < L) nmask[(p / 32) * stride + u] |= 1ull << (p % 32 * 2);
    for (const uint64_t* mask : {(const uint64_t*)nullptr, (const uint64_t*)nmask.data()}) {
      std::string expected(L, '?');
      for (uint32_t i = 0; i < L; ++i) {
        const uint64_t at = (i / 32) * stride + u;
        const unsigned shift = i % 32 * 2;
        expected[i] = "ACGT"[(reads[at] >> shift) & 3];
        if (mask && ((mask[at] >> shift) & 1)) expected[i] = 'N';
      }
      if (mask)
        for (uint32_t p : {0u, 31u, 32u, L - 1})
          if (p < L) EXPECT(expected[p] == 'N');
      char buf[257];
      std::memset(buf, '#', sizeof buf);
      mrg::unpack_read(reads.data(), mask, stride, u, L, buf);
      EXPECT(std::string(buf, L) == expected && buf[L] == '#');
      std::string text = "seq:";
      mrg::unpack_read(reads.data(), mask, stride, u, L, text);
      EXPECT(text == "seq:" + expected);
      if (L >= 3) {  // bases [first, last)
        const uint32_t first = L / 3, last = L - 1;
        std::memset(buf, '#', sizeof buf);
        mrg::unpack_read(reads.data(), mask, stride, u, first, last, buf);
        EXPECT(std::string(buf, last - first) == expected.substr(first, last - first) && buf[last - first] == '#');
      }
    }
  }
}

void check_append_int() {
  std::string out = "x";
  mrg::append_int(out, 0);
  mrg::append_int(out, -12);
  mrg::append_int(out, 9223372036854775807ll);
  EXPECT(out == "x0-129223372036854775807");
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: host_write_check <directory>\n");
    return 2;
  }
  check_scheduler();
  check_env();
  check_file(argv[1]);
  check_unpack();
  check_append_int();
  std::puts("host_write ok");
  return 0;
}
