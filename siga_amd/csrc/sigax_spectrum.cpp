// siga_amd/csrc/sigax_spectrum.cpp -- `siga preqc` on the device: the entry points of sigax_spectrum.hip.
#include <cstring>

#include "sigax_internal.h"

#define SPECTRUM_WORK_BYTES 64ull  // the kernel's string counter (one u64), padded to a line of its own

static int walk_check(sigax_index* ix, int which, const void* d_rows, u64 n, const void* d_status) {
  if (!ix || (which != 0 && which != 1) || !d_status || (n && !d_rows)) return sigax_fail(SIGAX_E_ARG, "bad argument");
  if (which == 1 && ix->fwd_only) return sigax_fail(SIGAX_E_STATE, "the index was opened without its reverse strand");
  return SIGAX_OK;
}

static int walk_enqueue(sigax_index* ix, int which, const u64* d_rows, u64 n, u32 max_len, u32* d_lens, u64* d_stretch, const u64* d_offs,
                        unsigned char* d_seqs, u64* d_status, hipStream_t st) {
  HIP_TRY(hipMemsetAsync(d_status, 0, d_seqs ? 24 : 16, st));
  WalkArgs wa;
  wa.s = ix->st[which];
  wa.rows = d_rows;
  wa.n = n;
  wa.max_len = max_len;
  wa.lens = d_lens;
  wa.stretch = d_stretch;
  wa.offs = d_offs;
  wa.out = d_seqs;
  wa.status = d_status;
  launch_walk(wa, ix->wide, st);
  HIP_TRY(hipGetLastError());
  return SIGAX_OK;
}

extern "C" int sigax_string_lengths_device(sigax_index* ix, int which, const void* d_rows, uint64_t n, uint32_t max_len, void* d_lens,
                                           void* d_stretch, void* d_status2, void* stream) {
  const int rc = walk_check(ix, which, d_rows, n, d_status2);
  if (rc != SIGAX_OK) return rc;
  if (n && !d_lens) return sigax_fail(SIGAX_E_ARG, "bad argument");
  HIP_TRY(hipSetDevice(ix->device));
  return walk_enqueue(ix, which, (const u64*)d_rows, n, max_len, (u32*)d_lens, (u64*)d_stretch, nullptr, nullptr, (u64*)d_status2,
                      (hipStream_t)stream);
}

extern "C" int sigax_get_strings_device(sigax_index* ix, int which, const void* d_rows, uint64_t n, uint32_t max_len, const void* d_offs,
                                        void* d_seqs, void* d_status3, void* stream) {
  const int rc = walk_check(ix, which, d_rows, n, d_status3);
  if (rc != SIGAX_OK) return rc;
  if (n && (!d_offs || !d_seqs)) return sigax_fail(SIGAX_E_ARG, "bad argument");
  HIP_TRY(hipSetDevice(ix->device));
  if (n == 0) {
    HIP_TRY(hipMemsetAsync(d_status3, 0, 24, (hipStream_t)stream));
    return SIGAX_OK;
  }
  return walk_enqueue(ix, which, (const u64*)d_rows, n, max_len, nullptr, nullptr, (const u64*)d_offs, (unsigned char*)d_seqs,
                      (u64*)d_status3, (hipStream_t)stream);
}

// rows (host) -> lengths, offsets and text in device memory, all owned by `g`; *total = the bytes of text
static int rows_to_device_strings(sigax_index* ix, int which, const u64* rows, u64 n, u32 max_len, DevGuard& g, u64** d_rows_out,
                                  u64** d_stretch, u64** d_offs, unsigned char** d_seqs, u64* total) {
  u64 *d_rows = nullptr, *d_partial = nullptr, *d_total = nullptr, *d_status = nullptr;
  u32* d_lens = nullptr;
  HIP_TRY(g.alloc((void**)&d_rows, (size_t)n * 8));
  HIP_TRY(g.alloc((void**)&d_lens, (size_t)n * 4));
  if (d_stretch) HIP_TRY(g.alloc((void**)d_stretch, (size_t)n * 8));
  HIP_TRY(g.alloc((void**)d_offs, ((size_t)n + 1) * 8));
  HIP_TRY(g.alloc((void**)&d_partial, (size_t)scan_partials_needed(n) * 8));
  HIP_TRY(g.alloc((void**)&d_total, 8));
  HIP_TRY(g.alloc((void**)&d_status, 24));
  const hipStream_t st = (hipStream_t)0;
  HIP_TRY(hipMemcpy(d_rows, rows, (size_t)n * 8, hipMemcpyHostToDevice));
  int rc = walk_enqueue(ix, which, d_rows, n, max_len, d_lens, d_stretch ? *d_stretch : nullptr, nullptr, nullptr, d_status, st);
  if (rc != SIGAX_OK) return rc;
  launch_scan(d_lens, n, d_partial, *d_offs, d_total, st);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(total, d_total, 8, hipMemcpyDeviceToHost));
  HIP_TRY(g.alloc((void**)d_seqs, (size_t)*total + 16));
  rc = walk_enqueue(ix, which, d_rows, n, max_len, nullptr, nullptr, *d_offs, *d_seqs, d_status, st);
  if (rc != SIGAX_OK) return rc;
  u64 status[3];
  HIP_TRY(hipMemcpy(status, d_status, 24, hipMemcpyDeviceToHost));
  if (status[2]) return sigax_fail(SIGAX_E_DEVICE, "%llu strings changed their length between the two passes", status[2]);
  if (d_rows_out) *d_rows_out = d_rows;
  return SIGAX_OK;
}

extern "C" int sigax_get_strings(sigax_index* ix, int which, const uint64_t* rows, uint64_t n, uint32_t max_len, char** seqs,
                                 uint64_t** offs, uint64_t* stretch) {
  if (!ix || (which != 0 && which != 1) || !seqs || !offs || (n && !rows)) return sigax_fail(SIGAX_E_ARG, "bad argument");
  if (which == 1 && ix->fwd_only) return sigax_fail(SIGAX_E_STATE, "the index was opened without its reverse strand");
  HIP_TRY(hipSetDevice(ix->device));
  *seqs = nullptr;
  *offs = nullptr;
  u64 total = 0;
  u64 *d_stretch = nullptr, *d_offs = nullptr;
  unsigned char* d_seqs = nullptr;
  DevGuard g;
  if (n) {
    const int rc = rows_to_device_strings(ix, which, (const u64*)rows, n, max_len, g, nullptr, stretch ? &d_stretch : nullptr, &d_offs,
                                          &d_seqs, &total);
    if (rc != SIGAX_OK) return rc;
  }
  HostGuard hg;
  char* h_seqs = hg.alloc<char>((size_t)total + 1);
  uint64_t* h_offs = hg.alloc<uint64_t>(((size_t)n + 1) * 8);
  if (!hg.ok) return sigax_fail(SIGAX_E_CAPACITY, "out of host memory");
  h_offs[0] = 0;
  h_seqs[total] = '\0';
  hipError_t e = hipSuccess;
  if (n) {
    e = hipMemcpy(h_offs, d_offs, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess && total) e = hipMemcpy(h_seqs, d_seqs, (size_t)total, hipMemcpyDeviceToHost);
    if (e == hipSuccess && stretch) e = hipMemcpy(stretch, d_stretch, (size_t)n * 8, hipMemcpyDeviceToHost);
  }
  if (e != hipSuccess) return sigax_fail(SIGAX_E_DEVICE, "copying the strings: %s", hipGetErrorString(e));
  hg.release();
  *seqs = h_seqs;
  *offs = h_offs;
  return SIGAX_OK;
}

// ---- k-mer spectrum ----
extern "C" int sigax_kmer_spectrum_workspace(uint64_t n_reads, uint64_t* bytes) {
  if (!bytes) return sigax_fail(SIGAX_E_ARG, "bad argument");
  (void)n_reads;  // a wave takes whole strings off one counter: nothing per string
  *bytes = SPECTRUM_WORK_BYTES;
  return SIGAX_OK;
}

static int spectrum_enqueue(sigax_index* ix, const unsigned char* d_seqs, const u64* d_offs, u64 n_reads, u32 k, u64 n_bins, u64* d_hist,
                            u64* d_stat, u64* d_work, hipStream_t st) {
  HIP_TRY(hipMemsetAsync(d_stat, 0, 32, st));
  HIP_TRY(hipMemsetAsync(d_work, 0, 8, st));
  SpectrumArgs sa;
  sa.fwd = ix->st[0];
  sa.seqs = d_seqs;
  sa.offs = d_offs;
  sa.n_reads = n_reads;
  sa.n_bins = n_bins;
  sa.k = k;
  const int rp = ptab_for_stream(ix, st, &sa.ptab, &sa.pk);
  if (rp != SIGAX_OK) return rp;
  sa.hist = d_hist;
  sa.dstat = d_stat;
  sa.counter = d_work;
  launch_spectrum(sa, ix->wide, ix->n_cu, st);
  HIP_TRY(hipGetLastError());
  return SIGAX_OK;
}

extern "C" int sigax_kmer_spectrum_device(sigax_index* ix, const void* d_seqs, const void* d_offs, uint64_t n_reads, uint32_t k,
                                          uint64_t n_bins, void* d_hist, void* d_stat4, void* d_work, uint64_t work_bytes, void* stream) {
  if (!ix || k == 0 || n_bins == 0) return sigax_fail(SIGAX_E_ARG, "bad argument");
  if (n_reads && (!d_seqs || !d_offs || !d_hist || !d_stat4 || !d_work || work_bytes < SPECTRUM_WORK_BYTES))
    return sigax_fail(SIGAX_E_ARG, "bad argument");
  HIP_TRY(hipSetDevice(ix->device));
  if (n_reads == 0) return SIGAX_OK;
  return spectrum_enqueue(ix, (const unsigned char*)d_seqs, (const u64*)d_offs, n_reads, k, n_bins, (u64*)d_hist, (u64*)d_stat4, (u64*)d_work,
                          (hipStream_t)stream);
}

// the spectrum of strings in device memory, added to the host's bins
static int spectrum_to_host(sigax_index* ix, DevGuard& g, const unsigned char* d_seqs, const u64* d_offs, u64 n_reads, u32 k, u64 n_bins,
                            uint64_t* hist, uint64_t stat4[4]) {
  u64 *d_hist = nullptr, *d_stat = nullptr, *d_work = nullptr;
  HIP_TRY(g.alloc((void**)&d_hist, (size_t)n_bins * 8));
  HIP_TRY(g.alloc((void**)&d_stat, 32));
  HIP_TRY(g.alloc((void**)&d_work, SPECTRUM_WORK_BYTES));
  HIP_TRY(hipMemset(d_hist, 0, (size_t)n_bins * 8));
  const int rc = spectrum_enqueue(ix, d_seqs, d_offs, n_reads, k, n_bins, d_hist, d_stat, d_work, (hipStream_t)0);
  if (rc != SIGAX_OK) return rc;
  HIP_TRY(hipStreamSynchronize((hipStream_t)0));
  std::vector<u64> h((size_t)n_bins);
  HIP_TRY(hipMemcpy(h.data(), d_hist, (size_t)n_bins * 8, hipMemcpyDeviceToHost));
  for (u64 b = 0; b < n_bins; ++b) hist[b] += h[b];
  if (stat4) HIP_TRY(hipMemcpy(stat4, d_stat, 32, hipMemcpyDeviceToHost));
  return SIGAX_OK;
}

extern "C" int sigax_kmer_spectrum_batch(sigax_index* ix, const char* seqs, const uint64_t* offs, uint64_t n_reads, uint32_t k,
                                         uint64_t n_bins, uint64_t* hist, uint64_t stat4[4]) {
  if (!ix || k == 0 || n_bins == 0 || (n_reads && (!seqs || !offs || !hist))) return sigax_fail(SIGAX_E_ARG, "bad argument");
  HIP_TRY(hipSetDevice(ix->device));
  if (stat4) memset(stat4, 0, 32);
  if (n_reads == 0) return SIGAX_OK;
  unsigned char* d_seqs = nullptr;
  u64* d_offs = nullptr;
  DevGuard g;
  const int rs = stage_strings(g, seqs, offs, n_reads, ~0ull, "string", (hipStream_t)0, &d_seqs, &d_offs);
  if (rs != SIGAX_OK) return rs;
  return spectrum_to_host(ix, g, d_seqs, d_offs, n_reads, k, n_bins, hist, stat4);
}

extern "C" int sigax_kmer_spectrum_rows(sigax_index* ix, const uint64_t* rows, uint64_t n, uint32_t k, uint32_t max_len, uint64_t n_bins,
                                        uint64_t* hist, uint64_t stat4[4]) {
  if (!ix || k == 0 || n_bins == 0 || (n && (!rows || !hist))) return sigax_fail(SIGAX_E_ARG, "bad argument");
  HIP_TRY(hipSetDevice(ix->device));
  if (stat4) memset(stat4, 0, 32);
  if (n == 0) return SIGAX_OK;
  u64 total = 0;
  u64* d_offs = nullptr;
  unsigned char* d_seqs = nullptr;
  DevGuard g;
  const int rc = rows_to_device_strings(ix, 0, (const u64*)rows, n, max_len, g, nullptr, nullptr, &d_offs, &d_seqs, &total);
  if (rc != SIGAX_OK) return rc;
  return spectrum_to_host(ix, g, d_seqs, d_offs, n, k, n_bins, hist, stat4);
}

extern "C" int sigax_kmer_spectrum_rows_hint(sigax_index* ix, uint32_t max_len, uint64_t n_bins, uint64_t* max_rows) {
  if (!ix || !max_rows) return sigax_fail(SIGAX_E_ARG, "bad argument");
  HIP_TRY(hipSetDevice(ix->device));
  size_t mfree = 0, mtotal = 0;
  HIP_TRY(hipMemGetInfo(&mfree, &mtotal));
  // half of what is free; a row costs its number, its length, its offset and up to max_len bytes of text.  No more than
  // 2^24 rows: by then the launches are long enough to hide everything around them
  const u64 budget = (u64)mfree / 2, fixed = n_bins * 8 + 4096, per_row = 8 + 4 + 8 + 1 + (u64)max_len;
  const u64 rows = budget > fixed ? (budget - fixed) / per_row : 0;
  *max_rows = std::min<u64>(std::max<u64>(rows, 1024), 1ull << 24);
  return SIGAX_OK;
}
