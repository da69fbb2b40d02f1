// siga_amd/csrc/sigax_match.cpp -- `siga match` on the device: the entry points of sigax_match.hip.
#include "sigax_internal.h"

static int match_enqueue(sigax_index* ix, const unsigned char* d_seqs, const u64* d_offs, u64 n_reads, u64 max_length, uint32_t flags,
                         u64* d_counts, u64* d_stat, hipStream_t st) {
  HIP_TRY(hipMemsetAsync(d_stat, 0, 32, st));
  MatchArgs ma;
  ma.fwd = ix->st[0];
  ma.seqs = d_seqs;
  ma.offs = d_offs;
  ma.n_reads = n_reads;
  ma.max_length = max_length;
  ma.rc = (flags & SIGAX_RC) ? 1u : 0u;
  const int rp = ptab_for_stream(ix, st, &ma.ptab, &ma.pk);
  if (rp != SIGAX_OK) return rp;
  ma.counts = d_counts;
  ma.dstat = d_stat;
  launch_match(ma, ix->wide, ix->n_cu, st);
  HIP_TRY(hipGetLastError());
  return SIGAX_OK;
}

extern "C" int sigax_match_device(sigax_index* ix, const void* d_seqs, const void* d_offs, uint64_t n_reads, uint64_t max_length,
                                  uint32_t flags, void* d_counts, void* d_stat4, void* stream) {
  if (!ix || (flags & ~SIGAX_RC) || (n_reads && (!d_seqs || !d_offs || !d_counts || !d_stat4))) return sigax_fail(SIGAX_E_ARG, "bad argument");
  HIP_TRY(hipSetDevice(ix->device));
  if (n_reads == 0) return SIGAX_OK;
  return match_enqueue(ix, (const unsigned char*)d_seqs, (const u64*)d_offs, n_reads, max_length, flags, (u64*)d_counts, (u64*)d_stat4,
                       (hipStream_t)stream);
}

extern "C" int sigax_match_batch(sigax_index* ix, const char* seqs, const uint64_t* offs, uint64_t n_reads, uint64_t max_length,
                                 uint32_t flags, uint64_t* counts) {
  if (!ix || (flags & ~SIGAX_RC) || (n_reads && (!seqs || !offs || !counts))) return sigax_fail(SIGAX_E_ARG, "bad argument");
  HIP_TRY(hipSetDevice(ix->device));
  if (n_reads == 0) return SIGAX_OK;
  unsigned char* d_seqs = nullptr;
  u64 *d_offs = nullptr, *d_counts = nullptr, *d_stat = nullptr;
  DevGuard g;
  const int rs = stage_strings(g, seqs, offs, n_reads, 0xFFFFFFFFull, "read", (hipStream_t)0, &d_seqs, &d_offs);
  if (rs != SIGAX_OK) return rs;
  HIP_TRY(g.alloc((void**)&d_counts, (size_t)n_reads * 16));
  HIP_TRY(g.alloc((void**)&d_stat, 32));
  const int rc = match_enqueue(ix, d_seqs, d_offs, n_reads, max_length, flags, d_counts, d_stat, (hipStream_t)0);
  if (rc != SIGAX_OK) return rc;
  HIP_TRY(hipStreamSynchronize((hipStream_t)0));
  HIP_TRY(hipMemcpy(counts, d_counts, (size_t)n_reads * 16, hipMemcpyDeviceToHost));
  return SIGAX_OK;
}

// ---- batches in flight (sigax.h: sigax_matcher) ----
struct sigax_matcher {
  sigax_index* ix;
  u64 max_reads, max_bases;
  struct Slot {
    hipStream_t st = nullptr;
    unsigned char* d_seqs = nullptr;
    u64 *d_offs = nullptr, *d_counts = nullptr, *d_stat = nullptr;
    u64 *h_offs = nullptr, *h_counts = nullptr;  // pinned; h_counts ends with the 4 statistics
    u64 n = 0;
  };
  std::vector<Slot> slots;
};

extern "C" void sigax_matcher_destroy(sigax_matcher* m) {
  if (!m) return;
  (void)hipSetDevice(m->ix->device);
  for (auto& s : m->slots) {
    if (s.st) {
      (void)hipStreamSynchronize(s.st);
      (void)hipStreamDestroy(s.st);
    }
    if (s.d_seqs) hipFree(s.d_seqs);
    if (s.d_offs) hipFree(s.d_offs);
    if (s.d_counts) hipFree(s.d_counts);
    if (s.d_stat) hipFree(s.d_stat);
    if (s.h_offs) (void)hipHostFree(s.h_offs);
    if (s.h_counts) (void)hipHostFree(s.h_counts);
  }
  delete m;
}

extern "C" int sigax_matcher_create(sigax_index* ix, uint32_t slots, uint64_t max_reads, uint64_t max_bases, sigax_matcher** out) {
  if (!ix || !out || slots == 0 || slots > 8) return sigax_fail(SIGAX_E_ARG, "bad argument");
  HIP_TRY(hipSetDevice(ix->device));
  if (max_reads == 0 || max_bases == 0) {
    // from the free memory: half of it over the slots, a read costing its bases (150 assumed) + 8 + 16 bytes; no more than 2^24
    // reads per batch, by which size the copies and the kernel overlap as well as they ever will
    size_t mfree = 0, mtotal = 0;
    HIP_TRY(hipMemGetInfo(&mfree, &mtotal));
    const u64 per_slot = (u64)mfree / 2 / slots;
    if (max_reads == 0) max_reads = std::min<u64>(std::max<u64>(per_slot / (150 + 24), 1024), 1ull << 24);
    if (max_bases == 0) max_bases = std::max<u64>(max_reads * 150, 1ull << 20);
  }
  sigax_matcher* m = new sigax_matcher;
  m->ix = ix;
  m->max_reads = max_reads;
  m->max_bases = max_bases;
  m->slots.resize(slots);
  for (auto& s : m->slots) {
    const bool ok = hipStreamCreateWithFlags(&s.st, hipStreamNonBlocking) == hipSuccess && hipMalloc((void**)&s.d_seqs, max_bases + 16) == hipSuccess &&
                    hipMalloc((void**)&s.d_offs, (max_reads + 1) * 8) == hipSuccess && hipMalloc((void**)&s.d_counts, max_reads * 16 + 16) == hipSuccess &&
                    hipMalloc((void**)&s.d_stat, 32) == hipSuccess && hipHostMalloc((void**)&s.h_offs, (max_reads + 1) * 8) == hipSuccess &&
                    hipHostMalloc((void**)&s.h_counts, max_reads * 16 + 32) == hipSuccess;
    if (!ok) {
      const int rc = sigax_fail(SIGAX_E_DEVICE, "matcher buffers: %s", hipGetErrorString(hipGetLastError()));
      sigax_matcher_destroy(m);
      return rc;
    }
  }
  *out = m;
  return SIGAX_OK;
}

extern "C" int sigax_matcher_capacity(const sigax_matcher* m, uint64_t* max_reads, uint64_t* max_bases) {
  if (!m) return sigax_fail(SIGAX_E_ARG, "bad argument");
  if (max_reads) *max_reads = m->max_reads;
  if (max_bases) *max_bases = m->max_bases;
  return SIGAX_OK;
}

extern "C" int sigax_matcher_submit(sigax_matcher* m, uint32_t slot, const char* seqs, const uint64_t* offs, uint64_t n_reads,
                                    uint64_t max_length, uint32_t flags) {
  if (!m || slot >= m->slots.size() || (flags & ~SIGAX_RC) || (n_reads && (!seqs || !offs))) return sigax_fail(SIGAX_E_ARG, "bad argument");
  HIP_TRY(hipSetDevice(m->ix->device));
  sigax_matcher::Slot& s = m->slots[slot];
  HIP_TRY(hipStreamSynchronize(s.st));  // the slot's previous batch (its pinned buffers are about to be written)
  s.n = n_reads;
  if (n_reads == 0) return SIGAX_OK;
  const u64 b0 = offs[0], nb = offs[n_reads] - b0;
  if (n_reads > m->max_reads || nb > m->max_bases) return sigax_fail(SIGAX_E_CAPACITY, "batch of %llu reads, %llu bases does not fit the slot", (u64)n_reads, nb);
  for (u64 i = 0; i <= n_reads; ++i) s.h_offs[i] = offs[i] - b0;
  HIP_TRY(hipMemcpyAsync(s.d_seqs, seqs + b0, nb, hipMemcpyHostToDevice, s.st));
  HIP_TRY(hipMemcpyAsync(s.d_offs, s.h_offs, (n_reads + 1) * 8, hipMemcpyHostToDevice, s.st));
  const int rc = match_enqueue(m->ix, s.d_seqs, s.d_offs, n_reads, max_length, flags, s.d_counts, s.d_stat, s.st);
  if (rc != SIGAX_OK) return rc;
  HIP_TRY(hipMemcpyAsync(s.h_counts, s.d_counts, n_reads * 16, hipMemcpyDeviceToHost, s.st));
  HIP_TRY(hipMemcpyAsync(s.h_counts + 2 * n_reads, s.d_stat, 32, hipMemcpyDeviceToHost, s.st));
  return SIGAX_OK;
}

extern "C" int sigax_matcher_wait(sigax_matcher* m, uint32_t slot, const uint64_t** counts, uint64_t stat4[4]) {
  if (!m || slot >= m->slots.size()) return sigax_fail(SIGAX_E_ARG, "bad argument");
  HIP_TRY(hipSetDevice(m->ix->device));
  sigax_matcher::Slot& s = m->slots[slot];
  HIP_TRY(hipStreamSynchronize(s.st));
  if (counts) *counts = (const uint64_t*)s.h_counts;
  if (stat4)
    for (int i = 0; i < 4; ++i) stat4[i] = s.n ? s.h_counts[2 * s.n + i] : 0;
  return SIGAX_OK;
}
