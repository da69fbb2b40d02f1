// siga_amd/host/host_util.hpp -- internal to the host library: its environment switches, the thread helpers and the phase timer.
#ifndef SIGA_AMD_HOST_HOST_UTIL_HPP_
#define SIGA_AMD_HOST_HOST_UTIL_HPP_

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <thread>
#include <vector>

namespace sigah {

// Every SIGA_* switch of the host library, read where an operation starts (build, rmdup, run, a sigah_* entry, an OutFile) and
// handed down: never a process-wide value, the switches may change between two calls of one process.
struct HostSettings {
  bool host_threads_set = false;  // SIGA_HOST_THREADS=<n>: host threads whatever -t says (the writer: at least 1) ...
  int host_threads = 0;           // ... its value
  bool no_hugepages = false;      // SIGA_NO_HUGEPAGES: A/B aid, no 2 MB pages for the loader's large blocks
  bool timing_loader = false;     // SIGA_TIMING_LOADER: the loader's steps on stderr
  bool loader_copy = false;       // SIGA_LOADER_COPY: A/B aid: every chunk the copying way
  int gzip_level = 0;             // SIGA_GZIP_LEVEL=<1..9>: every block through zlib at that level (0: the writer's own coder)
  bool sync_write = false;        // SIGA_SYNC_WRITE=1: the file is written by the caller, not by the writer's thread
  bool timing = false;            // SIGA_TIMING=1: phase times on stderr
  bool vt_ahead = false;          // SIGA_VT_AHEAD=1: VT lines ahead of the GPU (an option, see VtAhead) ...
  bool no_vt_ahead = false;       // ... SIGA_NO_VT_AHEAD: not even then
  uint64_t vt_ahead_bytes = (uint64_t)3 << 29;  // SIGA_VT_AHEAD_BYTES: text held ahead of the writer at most
  std::vector<int> device_map;    // SIGA_DEVICE_MAP=0,0,...: logical GPU k of the run is physical device map[k] (rehearsing --gpus N on fewer GPUs)
  size_t batch_reads = 0;         // SIGA_BATCH_READS: device batch size instead of the one derived from free memory (0: not set)
  size_t ed_hold_bytes = (size_t)4 << 30;  // SIGA_ED_HOLD_BYTES (tests: 0 = every batch's records wait for the end)
  bool ed_inline = false;         // SIGA_ED_INLINE=1: a batch's ED text before the next batch's VT lines, on the caller's thread
  bool subbatches_set = false;    // SIGAX_SUBBATCHES is set: the library's sub-batches are left as asked for

  HostSettings() {
    if (const char* e = getenv("SIGA_HOST_THREADS")) {
      host_threads_set = true;
      host_threads = atoi(e);
    }
    no_hugepages = getenv("SIGA_NO_HUGEPAGES") != nullptr;
    timing_loader = getenv("SIGA_TIMING_LOADER") != nullptr;
    loader_copy = getenv("SIGA_LOADER_COPY") != nullptr;
    if (const char* e = getenv("SIGA_GZIP_LEVEL")) gzip_level = atoi(e) < 1 || atoi(e) > 9 ? 0 : atoi(e);
    sync_write = getenv("SIGA_SYNC_WRITE") != nullptr;
    timing = getenv("SIGA_TIMING") != nullptr;
    if (const char* e = getenv("SIGA_VT_AHEAD")) vt_ahead = atoi(e) > 0;
    no_vt_ahead = getenv("SIGA_NO_VT_AHEAD") != nullptr;
    if (const char* e = getenv("SIGA_VT_AHEAD_BYTES")) vt_ahead_bytes = std::max<uint64_t>(strtoull(e, nullptr, 10), 1);
    if (const char* e = getenv("SIGA_DEVICE_MAP")) {
      for (const char* p = e; *p;) {
        device_map.push_back(atoi(p));
        while (*p && *p != ',') ++p;
        if (*p == ',') ++p;
      }
    }
    if (const char* e = getenv("SIGA_BATCH_READS")) batch_reads = std::max<size_t>(strtoull(e, nullptr, 10), 1);
    if (const char* e = getenv("SIGA_ED_HOLD_BYTES")) ed_hold_bytes = (size_t)strtoull(e, nullptr, 10);
    ed_inline = getenv("SIGA_ED_INLINE") != nullptr;
    subbatches_set = getenv("SIGAX_SUBBATCHES") != nullptr;
  }
  // Off unless asked for (SIGA_VT_AHEAD=1): on the 16-core boxes the phases of `siga overlap` already keep every core busy, and
  // text made early is text the name ranks and the index load wait for (20 M reads 1.53 s without, 1.84-1.95 s with).
  bool vt_ahead_wanted() const { return vt_ahead && !no_vt_ahead; }
};

// ------------------------------------------------------------------------------------------------------
// host parallelism: the GPU replaces the reference's OpenMP loop over reads; what is left on the host (parsing, name
// ranks, text formatting, deflate) is spread over plain threads
// ------------------------------------------------------------------------------------------------------
inline unsigned host_threads(size_t requested, const HostSettings& hs) {
  if (hs.host_threads > 0) return (unsigned)hs.host_threads;
  unsigned hw = std::max(1u, std::thread::hardware_concurrency());
  unsigned autoN = std::min(hw, 32u);
  return (unsigned)std::max<size_t>(requested > 1 ? requested : 0, autoN);
}

template <class F>
void parallel_for(size_t n, unsigned nt, F f) {
  if (n == 0) return;
  nt = (unsigned)std::min<size_t>(std::max(1u, nt), n);
  if (nt == 1) {
    for (size_t i = 0; i < n; ++i) f(i);
    return;
  }
  std::atomic<size_t> next(0);
  auto work = [&] {
    for (;;) {
      size_t i = next.fetch_add(1);
      if (i >= n) break;
      f(i);
    }
  };
  std::vector<std::thread> th;
  for (unsigned t = 1; t < nt; ++t) th.emplace_back(work);
  work();
  for (auto& x : th) x.join();
}

inline bool is_space(char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\v' || c == '\f' || c == '\r'; }

inline void append_u64(std::string& s, uint64_t v) {
  char tmp[24];
  int n = 0;
  do {
    tmp[n++] = (char)('0' + v % 10);
    v /= 10;
  } while (v);
  while (n) s.push_back(tmp[--n]);
}

struct PhaseTimer {  // SIGA_TIMING=1: phase times on stderr
  bool on;
  std::chrono::steady_clock::time_point t;
  explicit PhaseTimer(bool timing) : on(timing), t(std::chrono::steady_clock::now()) {}
  double split() {  // seconds since the last split() or lap()
    const auto n = std::chrono::steady_clock::now();
    const double s = std::chrono::duration<double>(n - t).count();
    t = n;
    return s;
  }
  void lap(const char* what) {
    const double s = split();
    if (on) fprintf(stderr, "[siga] %-28s %8.3f s\n", what, s);
  }
};

}  // namespace sigah

#endif
