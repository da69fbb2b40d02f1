// siga_amd/csrc/sigax_pairs.cpp -- `siga unitig --pairs` on the device: the entry points of sigax_pairs.hip.
#include <cmath>
#include <cstring>

#include "sigax_internal.h"

static_assert(sizeof(sigax_pair_link) == 24, "sigax_pair_link must be 24 bytes");
static_assert(sizeof(sigax_pairs_opts) == 24, "sigax_pairs_opts must be 24 bytes");

namespace {

// where the pieces of the caller's scratch lie (every piece 16-byte aligned)
struct PairWork {
  u64 where, cnt, scan_total, keys[2], vals[2], head, scan, partial, sort_tmp, sort_bytes, bytes;
  u64 zero_bytes;  // where, cnt and scan_total lie together at the front: one memset
};
PairWork pair_work(u64 n, u64 sort_bytes) {
  PairWork w;
  const u64 cap = n / 2;
  u64 at = 0;
  auto take = [&](u64 bytes) {
    const u64 here = at;
    at += (bytes + 15) & ~15ull;
    return here;
  };
  w.where = take(n * 8);
  w.cnt = take(PAIR_WORDS * 8);
  w.scan_total = take(8);
  w.zero_bytes = at;
  for (int k = 0; k < 2; ++k) w.keys[k] = take(cap * 8);
  for (int k = 0; k < 2; ++k) w.vals[k] = take(cap * 8);
  w.head = take(cap * 4);
  w.scan = take((cap + 1) * 8);
  w.partial = take(scan_partials_needed(cap) * 8);
  w.sort_tmp = take(sort_bytes);
  w.sort_bytes = sort_bytes;
  w.bytes = at;
  return w;
}

int pair_limits(u64 n_reads) {
  if (n_reads >= (1ull << 31)) return sigax_fail(SIGAX_E_ARG, "2^31 reads or more: a link key names a unitig end in 32 bits");
  return SIGAX_OK;
}

int pairs_opts_ok(const sigax_pairs_opts* o) {
  if (!o) return sigax_fail(SIGAX_E_ARG, "NULL where the pairs options are required");
  if (o->reserved != 0) return sigax_fail(SIGAX_E_ARG, "sigax_pairs_opts.reserved must be 0");
  if (o->flags & ~SIGAX_PAIRS_OUTWARD) return sigax_fail(SIGAX_E_ARG, "sigax_pairs_opts.flags 0x%x: SIGAX_PAIRS_OUTWARD or 0", o->flags);
  if (o->hist_bins == 0 || o->hist_bins > SIGAX_PAIRS_MAX_BINS)
    return sigax_fail(SIGAX_E_ARG, "hist_bins %u: 1 to %u", o->hist_bins, SIGAX_PAIRS_MAX_BINS);
  if (o->hist_shift > 31) return sigax_fail(SIGAX_E_ARG, "hist_shift %u: at most 31", o->hist_shift);
  return SIGAX_OK;
}

int pair_work_for(int device, u64 n_reads, PairWork* w) {
  u64 sort_bytes = 0;
  if (n_reads / 2) {
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(pairs_sort_bytes(n_reads / 2, &sort_bytes));
  }
  *w = pair_work(n_reads, sort_bytes);
  return SIGAX_OK;
}

}  // namespace

extern "C" int sigax_unitigs_pairs_workspace(int device, uint64_t n_reads, uint64_t* bytes) {
  if (!bytes) return sigax_fail(SIGAX_E_ARG, "bad argument");
  const int rc = pair_limits(n_reads);
  if (rc != SIGAX_OK) return rc;
  PairWork w;
  const int rw = pair_work_for(device, n_reads, &w);
  if (rw != SIGAX_OK) return rw;
  *bytes = w.bytes;
  return SIGAX_OK;
}

extern "C" int sigax_unitigs_pairs_device(int device, const void* d_mate, const void* d_lengths, uint64_t n_reads, const void* d_n_unitigs,
                                          const void* d_seq_offs, const void* d_lay_offs, const void* d_uflags,
                                          const sigax_placement* d_layout, const sigax_pairs_opts* opts, void* d_hist,
                                          sigax_pair_link* d_links, void* d_status24, void* d_work, uint64_t work_bytes, void* stream) {
  const int rl = pair_limits(n_reads);
  if (rl != SIGAX_OK) return rl;
  const int ro = pairs_opts_ok(opts);
  if (ro != SIGAX_OK) return ro;
  if (!d_hist || !d_status24) return sigax_fail(SIGAX_E_ARG, "NULL where a buffer is required");
  if (n_reads && (!d_mate || !d_lengths || !d_n_unitigs || !d_seq_offs || !d_lay_offs || !d_uflags || !d_layout || !d_work ||
                  (n_reads / 2 && !d_links)))
    return sigax_fail(SIGAX_E_ARG, "NULL where a buffer is required");
  if (((uintptr_t)d_hist | (uintptr_t)d_status24) & 7) return sigax_fail(SIGAX_E_ARG, "d_hist and d_status24 must be 8-byte aligned");
  if (n_reads && (((uintptr_t)d_layout | (uintptr_t)d_work) & 15)) return sigax_fail(SIGAX_E_ARG, "d_layout and d_work must be 16-byte aligned");
  if (n_reads && (((uintptr_t)d_n_unitigs | (uintptr_t)d_seq_offs | (uintptr_t)d_lay_offs | (uintptr_t)d_links) & 7))
    return sigax_fail(SIGAX_E_ARG, "d_n_unitigs, d_seq_offs, d_lay_offs and d_links must be 8-byte aligned");
  if (n_reads && (((uintptr_t)d_mate | (uintptr_t)d_lengths | (uintptr_t)d_uflags) & 3))
    return sigax_fail(SIGAX_E_ARG, "d_mate, d_lengths and d_uflags must be 4-byte aligned");
  HIP_TRY(hipSetDevice(device));
  const hipStream_t st = (hipStream_t)stream;
  if (n_reads == 0) {
    HIP_TRY(hipMemsetAsync(d_status24, 0, 24 * 8, st));
    HIP_TRY(hipMemsetAsync(d_hist, 0, (size_t)opts->hist_bins * 8, st));
    return SIGAX_OK;
  }
  PairWork w;
  const int rw = pair_work_for(device, n_reads, &w);
  if (rw != SIGAX_OK) return rw;
  if (work_bytes < w.bytes)
    return sigax_fail(SIGAX_E_ARG, "workspace of %llu bytes, %llu needed (sigax_unitigs_pairs_workspace)", (u64)work_bytes, w.bytes);
  char* base = (char*)d_work;
  PairArgs a;
  a.mate = (const uint32_t*)d_mate;
  a.lengths = (const uint32_t*)d_lengths;
  a.n_reads = n_reads;
  a.n_unitigs = (const u64*)d_n_unitigs;
  a.seq_offs = (const u64*)d_seq_offs;
  a.lay_offs = (const u64*)d_lay_offs;
  a.uflags = (const uint32_t*)d_uflags;
  a.layout = d_layout;
  a.flags = opts->flags;
  a.hist_bins = opts->hist_bins;
  a.hist_shift = opts->hist_shift;
  a.max_span = opts->max_span;
  a.hist = (u64*)d_hist;
  a.links = d_links;
  a.status = (u64*)d_status24;
  a.where = (u64*)(base + w.where);
  a.cnt = (u64*)(base + w.cnt);
  a.cap = n_reads / 2;
  for (int k = 0; k < 2; ++k) {
    a.keys[k] = (u64*)(base + w.keys[k]);
    a.vals[k] = (u64*)(base + w.vals[k]);
  }
  a.head = (uint32_t*)(base + w.head);
  a.scan = (u64*)(base + w.scan);
  a.partial = (u64*)(base + w.partial);
  a.scan_total = (u64*)(base + w.scan_total);
  a.sort_tmp = base + w.sort_tmp;
  a.sort_tmp_bytes = w.sort_bytes;
  HIP_TRY(hipMemsetAsync(base, 0, (size_t)w.zero_bytes, st));
  HIP_TRY(hipMemsetAsync(d_hist, 0, (size_t)opts->hist_bins * 8, st));
  if (a.cap) HIP_TRY(hipMemsetAsync(a.keys[0], 0xFF, (size_t)a.cap * 8, st));
  HIP_TRY(launch_pairs(a, st));
  return SIGAX_OK;
}

extern "C" int sigax_unitigs_pairs_host(int device, const uint32_t* mate, const uint32_t* lengths, uint64_t n_reads, uint64_t n_unitigs,
                                        const uint64_t* seq_offs, const uint64_t* lay_offs, const uint32_t* uflags,
                                        const sigax_placement* layout, const sigax_pairs_opts* opts, uint64_t** hist, sigax_pair_link** links,
                                        uint64_t status24[24]) {
  if (!hist || !links || !status24) return sigax_fail(SIGAX_E_ARG, "NULL where a buffer is required");
  *hist = nullptr;
  *links = nullptr;
  for (int k = 0; k < 24; ++k) status24[k] = 0;
  const int rl = pair_limits(n_reads);
  if (rl != SIGAX_OK) return rl;
  const int ro = pairs_opts_ok(opts);
  if (ro != SIGAX_OK) return ro;
  if (n_reads && (!mate || !lengths || !seq_offs || !lay_offs || (n_unitigs && !uflags)))
    return sigax_fail(SIGAX_E_ARG, "NULL where a buffer is required");
  if (n_unitigs > n_reads) return sigax_fail(SIGAX_E_ARG, "%llu unitigs of %llu reads", (u64)n_unitigs, (u64)n_reads);
  const u64 n = n_reads, placed = n ? lay_offs[n_unitigs] : 0;
  if (placed > n) return sigax_fail(SIGAX_E_ARG, "%llu placements of %llu reads", placed, n);
  if (placed && !layout) return sigax_fail(SIGAX_E_ARG, "NULL where a buffer is required");
  const u32 bins = opts->hist_bins;
  HostGuard hg;
  uint64_t* h_hist = hg.alloc<uint64_t>((size_t)bins * 8);
  if (!hg.ok) return sigax_fail(SIGAX_E_CAPACITY, "out of host memory");
  memset(h_hist, 0, (size_t)bins * 8);
  sigax_pair_link* h_links = nullptr;
  u64 status[24];
  memset(status, 0, sizeof status);
  if (n) {
    HIP_TRY(hipSetDevice(device));
    PairWork w;
    const int rw = pair_work_for(device, n, &w);
    if (rw != SIGAX_OK) return rw;
    DevGuard g;
    void *d_mate, *d_len, *d_so, *d_lo, *d_uf, *d_lay, *d_hist, *d_links, *d_status, *d_work;
    HIP_TRY(g.alloc(&d_mate, (size_t)n * 4));
    HIP_TRY(g.alloc(&d_len, (size_t)n * 4));
    HIP_TRY(g.alloc(&d_so, ((size_t)n + 1) * 8));
    HIP_TRY(g.alloc(&d_lo, ((size_t)n + 1) * 8));
    HIP_TRY(g.alloc(&d_uf, (size_t)n * 4));
    HIP_TRY(g.alloc(&d_lay, (size_t)n * sizeof(sigax_placement)));
    HIP_TRY(g.alloc(&d_hist, (size_t)bins * 8));
    HIP_TRY(g.alloc(&d_links, (size_t)(n / 2) * sizeof(sigax_pair_link)));
    HIP_TRY(g.alloc(&d_status, 32 * 8));
    HIP_TRY(g.alloc(&d_work, (size_t)w.bytes));
    HIP_TRY(hipMemcpy(d_mate, mate, (size_t)n * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_len, lengths, (size_t)n * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_so, seq_offs, ((size_t)n_unitigs + 1) * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_lo, lay_offs, ((size_t)n_unitigs + 1) * 8, hipMemcpyHostToDevice));
    if (n_unitigs) HIP_TRY(hipMemcpy(d_uf, uflags, (size_t)n_unitigs * 4, hipMemcpyHostToDevice));
    if (placed) HIP_TRY(hipMemcpy(d_lay, layout, (size_t)placed * sizeof(sigax_placement), hipMemcpyHostToDevice));
    const u64 nu = n_unitigs;  // the count the device reads: behind the 24 status words
    HIP_TRY(hipMemcpy((u64*)d_status + 24, &nu, 8, hipMemcpyHostToDevice));
    const int rc = sigax_unitigs_pairs_device(device, d_mate, d_len, n, (u64*)d_status + 24, d_so, d_lo, d_uf, (const sigax_placement*)d_lay, opts,
                                              d_hist, (sigax_pair_link*)d_links, d_status, d_work, w.bytes, nullptr);
    if (rc != SIGAX_OK) return rc;
    HIP_TRY(hipMemcpy(status, d_status, 24 * 8, hipMemcpyDeviceToHost));  // (waits for the null stream's kernels)
    if (status[22] > n / 2) return sigax_fail(SIGAX_E_DEVICE, "link records beyond their buffer");
    HIP_TRY(hipMemcpy(h_hist, d_hist, (size_t)bins * 8, hipMemcpyDeviceToHost));
    h_links = hg.alloc<sigax_pair_link>((size_t)status[22] * sizeof(sigax_pair_link));
    if (!hg.ok) return sigax_fail(SIGAX_E_CAPACITY, "out of host memory");
    if (status[22]) HIP_TRY(hipMemcpy(h_links, d_links, (size_t)status[22] * sizeof(sigax_pair_link), hipMemcpyDeviceToHost));
  } else {
    h_links = hg.alloc<sigax_pair_link>(0);
    if (!hg.ok) return sigax_fail(SIGAX_E_CAPACITY, "out of host memory");
  }
  for (int k = 0; k < 24; ++k) status24[k] = status[k];
  *hist = h_hist;
  *links = h_links;
  hg.release();
  return SIGAX_OK;
}

extern "C" int sigax_pairs_estimate(const uint64_t status24[24], uint64_t* insert_size, uint64_t* delta, double* span_mean, double* span_sd) {
  if (!status24) return sigax_fail(SIGAX_E_ARG, "bad argument");
  auto moments = [&](int at, double* mean, double* sd) {
    *mean = *sd = 0.0;
    const u64 n = status24[at];
    if (n == 0) return;
    const double m = (double)status24[at + 1] / (double)n;
    const double sq = ((double)status24[at + 3] * 18446744073709551616.0 + (double)status24[at + 2]) / (double)n;
    const double var = sq - m * m;
    *mean = m;
    *sd = var > 0.0 ? std::sqrt(var) : 0.0;
  };
  double m = 0, s = 0;
  moments(10, &m, &s);
  if (insert_size) *insert_size = (uint64_t)m;
  if (delta) *delta = (uint64_t)s;
  moments(14, &m, &s);
  if (span_mean) *span_mean = m;
  if (span_sd) *span_sd = s;
  return SIGAX_OK;
}
