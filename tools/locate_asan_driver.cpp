// tools/locate_asan_driver.cpp -- the batching and formatting of sigah::Locator (siga_amd/host/locate.cpp) under
// AddressSanitizer + UBSan without a GPU and without a Python in between: a stand-alone program that compiles locate.cpp and
// reads.cpp itself and puts a STUB in place of the library's calls -- sigax_locate_batch answered by string search over a
// small read set, with the library's layout of the arrays and its order of the hits.  Query files of FASTA and FASTQ, empty
// queries' neighbours, queries with N, more hits than --max-hits, batches of 1, 3 and "all" queries, two files in a row and
// a missing file; every run's text is compared with the text put together here.  One run of several batches holds its first
// call back until a second one has entered the stub: exactly two batches are in flight, which a Locator that waits for
// each batch before it hands over the next would never show.
//
//   bash tools/locate_asan.sh        (builds this with -fsanitize=address,undefined and runs it)
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <mutex>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "../siga_amd/host/siga_host.hpp"

static std::vector<std::string> g_reads;
static std::atomic<int> g_calls{0}, g_live{0}, g_max_live{0};
static std::atomic<bool> g_hold_first{false};  // the run's first call waits for company (and gives up after 5 s: a failed check)
static std::mutex g_mu;
static std::condition_variable g_entered;

static std::string revcomp(const std::string& w) {
  std::string r(w.rbegin(), w.rend());
  for (char& c : r) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : c == 'T' ? 'A' : 'N';
  return r;
}
static bool acgt(const std::string& w) { return !w.empty() && w.find_first_not_of("ACGT") == std::string::npos; }
static void search(const std::string& w, uint32_t q, uint32_t flag, std::vector<sigax_hit>* out) {
  for (size_t r = 0; r < g_reads.size(); ++r)
    for (size_t p = g_reads[r].find(w); p != std::string::npos; p = g_reads[r].find(w, p + 1))
      out->push_back(sigax_hit{q, (uint32_t)r, (uint32_t)p, flag});
}

// ---- the stub: what locate.cpp calls of libsigax.so ----
extern "C" {
const char* sigax_last_error(void) { return "stub error"; }
void sigax_free(void* p) { free(p); }
int sigax_locate_batch(sigax_index* ix, const char* seqs, const uint64_t* offs, uint64_t n, uint32_t flags, uint32_t max_hits, uint32_t max_len,
                       uint64_t** totals, uint32_t** qflags, uint64_t** hit_offs, sigax_hit** hits) {
  if (ix != (sigax_index*)0x10) return SIGAX_E_ARG;
  const int call = ++g_calls;
  const int live = ++g_live;
  int seen = g_max_live.load();
  while (live > seen && !g_max_live.compare_exchange_weak(seen, live)) {
  }
  {
    std::unique_lock<std::mutex> lock(g_mu);
    g_entered.notify_all();
    if (g_hold_first && call == 1) g_entered.wait_for(lock, std::chrono::seconds(5), [] { return g_live.load() >= 2; });
  }
  std::vector<sigax_hit> all;
  *totals = (uint64_t*)malloc(n * 8 + 8);
  *qflags = (uint32_t*)malloc(n * 4 + 4);
  *hit_offs = (uint64_t*)malloc((n + 1) * 8);
  for (uint64_t q = 0; q < n; ++q) {
    const std::string w(seqs + offs[q], offs[q + 1] - offs[q]);
    std::vector<sigax_hit> h;
    if (acgt(w)) {
      search(w, (uint32_t)q, 0, &h);
      if (flags & SIGAX_RC) search(revcomp(w), (uint32_t)q, SIGAX_HIT_REV, &h);
    }
    (*totals)[q] = h.size();
    (*qflags)[q] = (acgt(w) ? 0u : SIGAX_LOCATE_SKIPPED) | (h.size() > max_hits ? SIGAX_LOCATE_OVER : 0u);
    (*hit_offs)[q] = all.size();
    if (!(*qflags)[q])
      for (sigax_hit x : h) {
        if (x.offset > max_len) x = sigax_hit{x.query, 0xFFFFFFFFu, 0xFFFFFFFFu, x.flags | SIGAX_HIT_CUT};
        all.push_back(x);
      }
  }
  (*hit_offs)[n] = all.size();
  *hits = (sigax_hit*)malloc(all.size() * sizeof(sigax_hit) + 16);
  if (!all.empty()) memcpy(*hits, all.data(), all.size() * sizeof(sigax_hit));
  --g_live;
  return SIGAX_OK;
}
}

static std::string slurp(const std::string& p) {
  std::ifstream f(p, std::ios::binary);
  std::stringstream ss;
  ss << f.rdbuf();
  return ss.str();
}

// the text Locator::run is to write for these queries
static std::string want_text(const std::vector<std::pair<std::string, std::string>>& q, bool rc, uint32_t max_hits, uint32_t max_len) {
  std::string t;
  for (const auto& [name, w] : q) {
    std::vector<sigax_hit> h;
    if (acgt(w)) {
      search(w, 0, 0, &h);
      if (rc) search(revcomp(w), 0, SIGAX_HIT_REV, &h);
    }
    const bool listed = acgt(w) && h.size() <= max_hits;
    t += "QT\t" + name + "\t" + std::to_string(w.size()) + "\t" + std::to_string(h.size()) + "\t" + std::to_string(listed ? h.size() : 0) + "\n";
    if (listed)
      for (const sigax_hit& x : h)
        t += "HT\t" + name + "\t" + (x.offset > max_len ? "*\t*" : std::to_string(x.read) + "\t" + std::to_string(x.offset)) + "\t" +
             ((x.flags & SIGAX_HIT_REV) ? "-" : "+") + "\n";
  }
  return t;
}

int main(int argc, char** argv) {
  const std::string dir = argc > 1 ? argv[1] : "/tmp";
  std::mt19937_64 rng(11);
  auto dna = [&](size_t n) {
    std::string s(n, 'A');
    for (char& c : s) c = "ACGT"[rng() & 3];
    return s;
  };
  const std::string genome = dna(3000);
  for (int i = 0; i < 300; ++i) g_reads.push_back(genome.substr(rng() % (genome.size() - 50), 50));
  g_reads.push_back(std::string(50, 'A'));
  std::vector<std::pair<std::string, std::string>> qa, qb;
  for (int i = 0; i < 40; ++i) {
    const std::string& r = g_reads[rng() % g_reads.size()];
    std::string w = i % 7 == 0 ? revcomp(r) : r.substr(rng() % 20, 5 + rng() % 30);
    if (i % 11 == 3) w[w.size() / 2] = 'N';
    qa.push_back({i % 4 ? "q" + std::to_string(i) : "a_longer_query_name_" + std::to_string(i), w});
  }
  qa.push_back({"one_base", "A"});   // more hits than any --max-hits used here but the last
  qa.push_back({"absent", dna(45)});
  for (int i = 0; i < 17; ++i) qb.push_back({"b" + std::to_string(i), g_reads[rng() % g_reads.size()].substr(i, 30)});
  const std::string fa = dir + "/locate_drv_a.fa", fq = dir + "/locate_drv_b.fastq", out = dir + "/locate_drv.out";
  {
    std::ofstream f(fa);
    for (const auto& [n, w] : qa) f << ">" << n << " some comment\n" << w << "\n";
    std::ofstream g(fq);
    for (const auto& [n, w] : qb) g << "@" << n << "\n" << w << "\n+\n" << std::string(w.size(), 'I') << "\n";
  }
  std::vector<std::pair<std::string, std::string>> both = qa;
  both.insert(both.end(), qb.begin(), qb.end());
  sigax_index* fake = (sigax_index*)0x10;
  int bad = 0;
  auto check = [&](bool ok, const char* what) {
    if (!ok) {
      fprintf(stderr, "FAILED: %s\n", what);
      ++bad;
    }
  };
  for (bool rc : {true, false})
    for (uint32_t max_hits : {5u, 1000u, 0xFFFFFFFFu})
      for (uint32_t max_len : {10u, 0xFFFFFFFFu})
        for (size_t batch : {(size_t)1, (size_t)3, (size_t)0}) {
          for (size_t threads : {(size_t)1, (size_t)4}) {
            sigah::Locator loc(max_hits, max_len, rc);
            size_t processed = 0;
            g_calls = 0;
            check(loc.run(fake, {fa, fq}, out, threads, batch, &processed), "run over two files");
            check(processed == both.size(), "processed count");
            check(slurp(out) == want_text(both, rc, max_hits, max_len), "text of two files");
            check(g_calls == (batch == 0 ? 2 : (int)((qa.size() + batch - 1) / batch + (qb.size() + batch - 1) / batch)), "number of batches");
          }
        }
  check(g_max_live.load() <= 2, "never more than two batches in flight");
  {
    // several batches, the first held until the second is in the stub: both are in flight, and the text is still in order
    sigah::Locator loc(1000u, 0xFFFFFFFFu, true);
    g_calls = 0;
    g_max_live = 0;
    g_hold_first = true;
    check(loc.run(fake, {fa, fq}, out, 2, 3), "run with the first batch held back");
    g_hold_first = false;
    check(g_calls > 4, "several batches");
    check(g_max_live.load() == 2, "exactly two batches in flight");
    check(slurp(out) == want_text(both, true, 1000u, 0xFFFFFFFFu), "text with two batches in flight");
  }
  {
    sigah::Locator loc;
    check(!loc.run(fake, {fq, dir + "/no_such_file.fa", fa}, out), "a missing input ends the run");
    check(slurp(out) == want_text(qb, true, 1000, 0xFFFFFFFFu), "... with what came before it written");
    check(!loc.error().empty(), "... and says so");
    check(!loc.run((sigax_index*)nullptr, {fa}, out) && loc.error() == "FMIndex not loaded", "no index");
    check(!loc.run((sigax_index*)0x20, {fa}, out) && loc.error().find("stub error") != std::string::npos, "the library's error is handed over");
  }
  printf("locate_asan_driver: %s\n", bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}
