// siga_amd/host/locate.cpp -- Locator (`siga locate`): where every query of the inputs occurs in the indexed reads.
#include <cstdio>
#include <future>

#include "host_util.hpp"
#include "reads.hpp"
#include "siga_host.hpp"

namespace sigah {

namespace {

// what one sigax_locate_batch call gave back; the arrays are the library's (sigax_free)
struct Located {
  int rc = SIGAX_OK;
  std::string error;  // the library's text is thread-local: the calling thread hands it over
  uint64_t* totals = nullptr;
  uint32_t* qflags = nullptr;
  uint64_t* hit_offs = nullptr;
  sigax_hit* hits = nullptr;
  Located() = default;
  Located(const Located&) = delete;
  Located& operator=(const Located&) = delete;
  Located(Located&& o) noexcept : rc(o.rc), error(std::move(o.error)), totals(o.totals), qflags(o.qflags), hit_offs(o.hit_offs), hits(o.hits) {
    o.totals = nullptr;
    o.qflags = nullptr;
    o.hit_offs = nullptr;
    o.hits = nullptr;
  }
  ~Located() {
    sigax_free(totals);
    sigax_free(qflags);
    sigax_free(hit_offs);
    sigax_free(hits);
  }
};

// "QT\t<name>\t<query length>\t<total>\t<listed>" and the query's "HT\t<name>\t<read index>\t<offset>\t<+|->" lines, in the
// library's order; a hit whose walk was cut at --max-length has no place: "HT\t<name>\t*\t*\t<+|->"
void format_query(std::string& t, std::string_view name, uint64_t len, const Located& r, size_t k) {
  const uint64_t a = r.hit_offs[k], b = r.hit_offs[k + 1];
  t += "QT\t";
  t.append(name.data(), name.size());
  t += '\t';
  append_u64(t, len);
  t += '\t';
  append_u64(t, r.totals[k]);
  t += '\t';
  append_u64(t, b - a);
  t += '\n';
  for (uint64_t h = a; h < b; ++h) {
    const sigax_hit& hit = r.hits[h];
    t += "HT\t";
    t.append(name.data(), name.size());
    if (hit.flags & SIGAX_HIT_CUT) {
      t += "\t*\t*\t";
    } else {
      t += '\t';
      append_u64(t, hit.read);
      t += '\t';
      append_u64(t, hit.offset);
      t += '\t';
    }
    t += (hit.flags & SIGAX_HIT_REV) ? '-' : '+';
    t += '\n';
  }
}

}  // namespace

// Two batches in flight: batch i is handed to a thread of its own (sigax_locate_batch is synchronous and runs on a stream of
// its own), then batch i - 1 is waited for, its lines formatted by the host threads, piece by piece, and written in query order.
bool Locator::run(sigax_index* index, const std::vector<std::string>& inputs, const std::string& output, size_t threads, size_t batchQueries,
                  size_t* processed) const {
  _error.clear();
  if (processed) *processed = 0;
  if (!index) {
    _error = "FMIndex not loaded";
    return false;
  }
  FILE* out = output.empty() ? stdout : fopen(output.c_str(), "wb");
  if (!out) {
    _error = "Failed to create " + output;
    return false;
  }
  const HostSettings hs;
  const unsigned nt = host_threads(threads, hs);
  const size_t cap_queries = batchQueries ? batchQueries : ((size_t)1 << 18);
  const uint64_t cap_bases = (uint64_t)64 << 20;  // (a query longer than this is a batch of its own)
  bool ok = true;
  auto fail = [&](const std::string& what) {
    if (ok) _error = what;
    ok = false;
  };
  std::vector<std::string> pieces;
  for (size_t f = 0; f < inputs.size() && ok; ++f) {
    ReadStore rs;
    if (!LoadReads(inputs[f], &rs, nt, hs)) {
      fail("Failed to create DNASeqReader " + inputs[f]);
      break;
    }
    const size_t n = rs.size();
    if (n == 0) continue;
    for (size_t i = 0; i < n; ++i)
      if (rs.offs[i + 1] - rs.offs[i] > 0xFFFFFFFFull) fail("query too long in " + inputs[f]);
    if (!ok) break;
    std::vector<size_t> cut(1, 0);
    for (size_t b = 0; b < n;) {
      size_t e = b + 1;
      while (e < n && e - b < cap_queries && rs.offs[e + 1] - rs.offs[b] <= cap_bases) ++e;
      cut.push_back(e);
      b = e;
    }
    const size_t nb = cut.size() - 1;
    const uint32_t flags = _rc ? SIGAX_RC : 0u, max_hits = _maxHits, max_len = _maxLength;
    auto submit = [&, index](size_t i) {
      const char* seqs = rs.seqs.data();
      const uint64_t* offs = rs.offs.data() + cut[i];
      const uint64_t cnt = cut[i + 1] - cut[i];
      return std::async(std::launch::async, [=] {
        Located r;
        r.rc = sigax_locate_batch(index, seqs, offs, cnt, flags, max_hits, max_len, &r.totals, &r.qflags, &r.hit_offs, &r.hits);
        if (r.rc != SIGAX_OK) r.error = sigax_last_error();
        return r;
      });
    };
    auto drain = [&](size_t i, std::future<Located>& fut) {
      const Located r = fut.get();
      if (r.rc != SIGAX_OK) {
        fail("locate failed: " + r.error);
        return;
      }
      if (!ok) return;
      const size_t b = cut[i], cnt = cut[i + 1] - b, np = std::min<size_t>(std::max<size_t>(1, cnt / 4096), 4 * (size_t)nt);
      pieces.resize(np);
      parallel_for(np, nt, [&](size_t p) {
        std::string& t = pieces[p];
        t.clear();
        for (size_t k = cnt * p / np; k < cnt * (p + 1) / np; ++k) format_query(t, rs.name(b + k), rs.offs[b + k + 1] - rs.offs[b + k], r, k);
      });
      for (const std::string& t : pieces)
        if (!t.empty() && fwrite(t.data(), 1, t.size(), out) != t.size()) fail("Failed to write " + (output.empty() ? std::string("stdout") : output));
      if (processed) *processed += cnt;
    };
    std::future<Located> flight[2];  // every future is waited for before `rs` goes: its thread reads the store
    for (size_t i = 0; i < nb; ++i) {
      flight[i & 1] = submit(i);
      if (i > 0) drain(i - 1, flight[(i - 1) & 1]);
      if (!ok) {
        (void)flight[i & 1].get();
        break;
      }
    }
    if (ok) drain(nb - 1, flight[(nb - 1) & 1]);
  }
  if (fflush(out) != 0) fail("Failed to write output");
  if (out != stdout) fclose(out);
  return ok;
}

}  // namespace sigah
