// siga_amd/host/strand_index.cpp -- `siga index` on the host: the suffix sorters, BWT(sa, reads) and the .bwt/.sai writers.
#include <cstdio>
#include <cstring>

#include "host_util.hpp"
#include "sais.hpp"
#include "siga_host.hpp"

namespace sigah {

// ------------------------------------------------------------------------------------------------------
// index construction
// ------------------------------------------------------------------------------------------------------
static inline int torank(char c) {  // src/alphabet.h:19-39
  switch (c) {
    case 'A': return 1;
    case 'C': return 2;
    case 'G': return 3;
    case 'T': return 4;
    default: return 0;
  }
}

// Multi-threaded suffix sort for many-core hosts: bucket every suffix by its first KP symbols (counting sort over
// base-6 keys), then comparison-sort the buckets in parallel.  The terminator is unique, so memcmp from offset KP
// decides every pair.  Same total order as SA-IS by construction (plain suffix array, end of text smallest).  Returns
// false (caller falls back to SA-IS) when a bucket is so large that long repeats would make it crawl.
//
// OWN_SENTINELS: the order of `siga index -a sais` (SAISBuilder, src/suffix_array_builder.cpp:31-172: suffixes compared as
// strings up to the end of their read, ties by read index) -- every read's own '$', ordered by read index, instead of one
// shared '$' with comparisons running on into the next read.  In the concatenated text that is: compare up to and including
// the first '$', then by position.  Keys stop at the first '$' (what follows it counts as nothing) and are computed per
// position instead of rolled.  Reads must be ACGT-only (the caller checks: the reference compares raw characters in one
// phase and ranks in the other, which agree only on A, C, G, T).
template <typename I, bool OWN_SENTINELS = false>
static bool parallel_suffix_sort(const uint8_t* T, uint64_t n /* incl. terminator */, I* SA, unsigned threads) {
  const int KP = 9;
  uint64_t nb = 1;
  for (int i = 0; i < KP; ++i) nb *= 6;
  auto key_at = [&](uint64_t p) {
    uint64_t k = 0;
    bool ended = false;
    for (int i = 0; i < KP; ++i) {
      const uint64_t c = (p + i < n && !ended) ? T[p + i] : 0;
      k = k * 6 + c;
      if (OWN_SENTINELS && c <= 1) ended = true;
    }
    return k;
  };
  // counting passes: a modest number of threads (each holds a histogram of nb counters), rolling base-6 keys
  const unsigned ct = std::min<unsigned>(threads, 16);
  uint64_t top = 1;
  for (int i = 0; i < KP - 1; ++i) top *= 6;
  std::vector<uint64_t> start(nb + 1, 0);
  std::vector<std::vector<uint32_t>> hist(ct);
  const uint64_t chunk = (n + ct - 1) / ct;
  auto sweep = [&](unsigned t, bool scatter) {
    uint64_t b = t * chunk, e = std::min(n, b + chunk);
    if (b >= e) return;
    uint64_t k = key_at(b);
    for (uint64_t p = b; p < e; ++p) {
      if (scatter) SA[start[k] + hist[t][k]++] = (I)p;
      else ++hist[t][k];
      if (OWN_SENTINELS) k = p + 1 < n ? key_at(p + 1) : 0;
      else k = (k % top) * 6 + (p + KP < n ? T[p + KP] : 0);
    }
  };
  {
    std::vector<std::thread> th;
    for (unsigned t = 0; t < ct; ++t)
      th.emplace_back([&, t] {
        hist[t].assign(nb, 0);
        sweep(t, false);
      });
    for (auto& x : th) x.join();
  }
  uint64_t acc = 0, biggest = 0;
  for (uint64_t k = 0; k < nb; ++k) {
    start[k] = acc;
    uint64_t c = 0;
    for (unsigned t = 0; t < ct; ++t) {
      uint32_t h = hist[t][k];
      hist[t][k] = (uint32_t)c;  // this thread's offset inside the bucket (< 2^32 checked below)
      c += h;
    }
    if (c > 0xFFFFFFF0ull) return false;
    biggest = std::max(biggest, c);
    acc += c;
  }
  start[nb] = acc;
  if (biggest > (64ull << 20)) return false;
  {
    std::vector<std::thread> th;
    for (unsigned t = 0; t < ct; ++t) th.emplace_back([&, t] { sweep(t, true); });
    for (auto& x : th) x.join();
  }
  // sort the buckets, largest first, pulled from a shared counter
  std::vector<uint64_t> order;
  order.reserve(1 << 20);
  for (uint64_t k = 0; k < nb; ++k)
    if (start[k + 1] - start[k] > 1) order.push_back(k);
  std::sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) { return start[a + 1] - start[a] > start[b + 1] - start[b]; });
  std::atomic<uint64_t> next(0);
  auto less = [&](I a, I b) {
    uint64_t pa = (uint64_t)a + KP, pb = (uint64_t)b + KP;
    if (OWN_SENTINELS) {
      // same key: either both reads ended inside the first KP symbols (equal strings: the earlier read first), or neither
      // did and the strings go on: compare up to and including the next '$' of the one that ends first
      bool ended = false;
      for (int i = 0; i < KP && !ended; ++i) ended = (uint64_t)a + i >= n || T[(uint64_t)a + i] <= 1;
      if (ended) return a < b;
      const uint8_t* ea = (const uint8_t*)memchr(T + pa, 1, n - pa);
      const uint8_t* eb = (const uint8_t*)memchr(T + pb, 1, n - pb);
      const uint64_t la = (ea ? (uint64_t)(ea - (T + pa)) : n - pa - 1) + 1, lb = (eb ? (uint64_t)(eb - (T + pb)) : n - pb - 1) + 1;
      const int c = memcmp(T + pa, T + pb, std::min(la, lb));
      if (c != 0) return c < 0;
      return a < b;  // both end here ('$' against a base differs above): the earlier read first
    }
    if (pa >= n || pb >= n) return a > b;  // the shorter suffix (later start) is smaller
    uint64_t la = n - pa, lb = n - pb;
    int c = memcmp(T + pa, T + pb, std::min(la, lb));
    if (c != 0) return c < 0;
    return la < lb;
  };
  {
    std::vector<std::thread> th;
    for (unsigned t = 0; t < threads; ++t)
      th.emplace_back([&] {
        while (true) {
          uint64_t i = next.fetch_add(1);
          if (i >= order.size()) break;
          uint64_t k = order[i];
          std::sort(SA + start[k], SA + start[k + 1], less);
        }
      });
    for (auto& x : th) x.join();
  }
  return true;
}

template <typename I>
static bool build_strand(const char* seqs, const uint64_t* offs, uint64_t nReads, bool reverse, StrandIndex* out,
                         unsigned threads, bool own_sentinels = false) {
  uint64_t total = 0;
  for (uint64_t i = 0; i < nReads; ++i) total += (offs[i + 1] - offs[i]) + 1;
  // text over {terminator 0, $ 1, A 2, C 3, G 4, T 5}; one '$' after every read, unique terminator at the end
  std::vector<uint8_t> T(total + 1);
  std::vector<uint64_t> starts(nReads);
  uint64_t p = 0;
  for (uint64_t i = 0; i < nReads; ++i) {
    starts[i] = p;
    uint64_t b = offs[i], e = offs[i + 1];
    if (!reverse) {
      for (uint64_t k = b; k < e; ++k) T[p++] = (uint8_t)(torank(seqs[k]) + 1);
    } else {  // src/indexer.cpp:60-64: reads reversed, not complemented
      for (uint64_t k = e; k > b; --k) T[p++] = (uint8_t)(torank(seqs[k - 1]) + 1);
    }
    T[p++] = 1;
  }
  T[p] = 0;
  std::vector<I> SA(total + 1);
  if (own_sentinels) {
    // `-a sais`: the bucket sort with the reads' own sentinels; the terminator's row comes out first (key 0) like the others'
    if (!parallel_suffix_sort<I, true>(T.data(), total + 1, SA.data(), std::max(threads, 1u))) return false;
  } else if (threads < 2 || total < (1u << 20) || !parallel_suffix_sort<I>(T.data(), total + 1, SA.data(), threads))
    sais<uint8_t, I>(T.data(), SA.data(), (I)(total + 1), (I)6);
  out->runs.clear();
  out->sai.clear();
  out->sai.reserve(nReads);
  out->nStrings = nReads;
  out->nSymbols = total;
  // BWT(sa, reads): src/bwt.cpp:7-32 (run == c && !full -> ++run; else flush)
  uint8_t run = 0;
  auto push = [&](uint32_t rank) {
    if (run) {
      if ((uint32_t)(run >> 5) == rank && (run & 31) != 31) {
        ++run;
        return;
      }
      out->runs.push_back(run);
    }
    run = (uint8_t)((rank << 5) | 1u);
  };
  for (uint64_t k = 1; k <= total; ++k) {  // SA[0] is the terminator
    uint64_t pos = (uint64_t)SA[k];
    uint32_t prevCode = pos == 0 ? 1u : T[pos - 1];
    push(prevCode - 1);
    if (prevCode == 1) {  // maybe the start of a read: SA row with j == 0 (src/suffix_array_builder.cpp:520-531).
      // Decided by position, not by the preceding symbol: a non-ACGT base ranks like the sentinel (alphabet.h:19-39).
      auto it = std::lower_bound(starts.begin(), starts.end(), pos);
      if (it != starts.end() && *it == pos) out->sai.push_back((uint32_t)(it - starts.begin()));
    }
  }
  if (run) out->runs.push_back(run);
  return true;
}

bool BuildStrandIndex(const char* seqs, const uint64_t* offs, uint64_t nReads, bool reverse, StrandIndex* out,
                      std::string* error, unsigned threads, bool own_sentinels) {
  uint64_t total = 0;
  for (uint64_t i = 0; i < nReads; ++i) {
    if (offs[i + 1] < offs[i]) {
      if (error) *error = "bad read offsets";
      return false;
    }
    total += (offs[i + 1] - offs[i]) + 1;
  }
  if (nReads >= 0xFFFFFFFFull) {  // SuffixArray::Elem is uint32 (src/suffix_array.h:33-34)
    if (error) *error = "too many reads for the .sai format";
    return false;
  }
  if (own_sentinels) {
    for (uint64_t k = offs[0]; k < offs[nReads]; ++k)
      if (torank(seqs[k]) == 0) {
        if (error) *error = "algorithm sais: reads with bases other than A, C, G, T are not supported";
        return false;
      }
  }
  try {
    bool ok;
    if (total + 1 < 0x7FFFFFF0ull) ok = build_strand<int32_t>(seqs, offs, nReads, reverse, out, threads, own_sentinels);
    else ok = build_strand<int64_t>(seqs, offs, nReads, reverse, out, threads, own_sentinels);
    if (!ok && error) *error = "algorithm sais: input too repetitive for the bucket sort";
    return ok;
  } catch (const std::bad_alloc&) {
    if (error) *error = "out of memory building the suffix array";
    return false;
  }
}

// The same on the GPU (libsigax: sigax_build_strand).  *rc receives the library's code: SIGAX_E_CAPACITY means the input
// is too repetitive for the device sort and the caller should use BuildStrandIndex.
bool BuildStrandIndexGPU(const char* seqs, const uint64_t* offs, uint64_t nReads, bool reverse, int device, StrandIndex* out,
                         std::string* error, int* rc_out) {
  uint8_t* runs = nullptr;
  uint32_t* sai = nullptr;
  uint64_t nruns = 0, nsym = 0;
  int rc = sigax_build_strand(seqs, offs, nReads, reverse ? 1 : 0, device, &runs, &nruns, &sai, &nsym);
  if (rc_out) *rc_out = rc;
  if (rc != SIGAX_OK) {
    if (error) *error = sigax_last_error();
    return false;
  }
  out->runs.assign(runs, runs + nruns);
  out->sai.assign(sai, sai + nReads);
  out->nStrings = nReads;
  out->nSymbols = nsym;
  sigax_free(runs);
  sigax_free(sai);
  return true;
}

bool StrandIndex::writeBWT(const std::string& path) const {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) return false;
  uint16_t magic = 0xCACA;
  uint64_t nruns = runs.size();
  int32_t flag = 0;
  bool ok = fwrite(&magic, 2, 1, f) == 1 && fwrite(&nStrings, 8, 1, f) == 1 && fwrite(&nSymbols, 8, 1, f) == 1 &&
            fwrite(&nruns, 8, 1, f) == 1 && fwrite(&flag, 4, 1, f) == 1 &&
            (nruns == 0 || fwrite(runs.data(), 1, nruns, f) == nruns);
  return fclose(f) == 0 && ok;
}

bool StrandIndex::writeSAI(const std::string& path) const {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) return false;
  char hdr[64];
  const int hn = snprintf(hdr, sizeof(hdr), "%u\n%llu\n%llu\n", 0xCACAu, (unsigned long long)sai.size(), (unsigned long long)sai.size());
  bool ok = fwrite(hdr, 1, (size_t)hn, f) == (size_t)hn;
  // "<readIdx> 0\n" per row (src/suffix_array.cpp:17-44), formatted in slices of 2^20 rows on a few threads (20 M rows of
  // BASELINE configs[2] took one thread a second, digit by digit into a std::string) and written in order
  const size_t slice = (size_t)1 << 20, nslices = (sai.size() + slice - 1) / slice;
  const unsigned nt = (unsigned)std::min<size_t>(std::max<size_t>(nslices, 1), std::min(8u, std::max(1u, std::thread::hardware_concurrency())));
  for (size_t base = 0; ok && base < nslices; base += nt) {
    const size_t cnt = std::min<size_t>(nt, nslices - base);
    std::vector<std::string> text(cnt);
    parallel_for(cnt, nt, [&](size_t k) {
      const size_t b0 = (base + k) * slice, e0 = std::min(sai.size(), b0 + slice);
      std::string& o = text[k];
      o.resize((e0 - b0) * 13);  // ten digits at most, " 0\n"
      char* w = &o[0];
      for (size_t i = b0; i < e0; ++i) {
        uint32_t id = sai[i];
        char d[12];
        int n = 0;
        do {
          d[n++] = (char)('0' + id % 10);
          id /= 10;
        } while (id);
        while (n) *w++ = d[--n];
        *w++ = ' ';
        *w++ = '0';
        *w++ = '\n';
      }
      o.resize((size_t)(w - &o[0]));
    });
    for (size_t k = 0; ok && k < cnt; ++k) ok = fwrite(text[k].data(), 1, text[k].size(), f) == text[k].size();
  }
  return fclose(f) == 0 && ok;
}

}  // namespace sigah
