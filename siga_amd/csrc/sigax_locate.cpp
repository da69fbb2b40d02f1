// siga_amd/csrc/sigax_locate.cpp -- `siga locate` on the device: the entry points of sigax_locate.hip.
#include <cstring>

#include "sigax_internal.h"

namespace {

// where the pieces of the caller's scratch lie
struct LocateWork {
  u64 chains, cnt, partial, counters, bytes;
};
LocateWork locate_work(u64 n) {
  LocateWork w;
  u64 at = 0;
  w.chains = at;  // {lower row, width} of a query's two chains
  at += n * 32;
  w.partial = at;
  at += scan_partials_needed(n) * 8;
  w.counters = at;  // the search's chain counter (and 8 bytes that keep what follows aligned)
  at += 16;
  w.cnt = at;
  at += n * 4;
  w.bytes = (at + 15) & ~15ull;
  return w;
}

int locate_usable(const sigax_index* ix) {
  if (!ix->d_sai[0] || ix->n_sai != ix->n_strings)
    return sigax_fail(SIGAX_E_STATE, "the index was opened without its forward .sai table: locating needs it to name the reads");
  if (ix->st[0].C[1] != ix->n_strings)
    return sigax_fail(SIGAX_E_STATE, "reads with non-ACGT bases: stretches are not reads, hits cannot be located");
  return SIGAX_OK;
}

LocateArgs locate_args(sigax_index* ix, const unsigned char* d_seqs, const u64* d_offs, u64 n, uint32_t flags, uint32_t max_hits,
                       uint32_t max_len, u64* d_totals, uint32_t* d_qflags, u64* d_hit_offs, u64* d_status, void* d_work) {
  const LocateWork w = locate_work(n);
  char* base = (char*)d_work;
  LocateArgs la;
  la.fwd = ix->st[0];
  la.seqs = d_seqs;
  la.offs = d_offs;
  la.n_queries = n;
  la.rc = (flags & SIGAX_RC) ? 1u : 0u;
  la.pk = 0;  // (locate_search_enqueue looks for the table)
  la.ptab = nullptr;
  la.max_hits = max_hits;
  la.max_len = max_len;
  la.chains = (ulonglong2*)(base + w.chains);
  la.totals = d_totals;
  la.qflags = d_qflags;
  la.cnt = (uint32_t*)(base + w.cnt);
  la.hit_offs = d_hit_offs;
  la.hits = nullptr;
  la.rows = nullptr;
  la.hits_cap = 0;
  la.sai = ix->d_sai[0];
  la.n_sai = ix->n_sai;
  la.status = d_status;
  la.counters = (u64*)(base + w.counters);
  return la;
}

// search, flags and totals, prefix sum: after this d_totals, d_qflags, d_hit_offs and status[0] are complete
int locate_search_enqueue(sigax_index* ix, LocateArgs& la, u64* d_hit_offs, void* d_work, hipStream_t st) {
  const LocateWork w = locate_work(la.n_queries);
  char* base = (char*)d_work;
  HIP_TRY(hipMemsetAsync(la.status, 0, 32, st));
  HIP_TRY(hipMemsetAsync(la.chains, 0, (size_t)la.n_queries * 32, st));
  HIP_TRY(hipMemsetAsync(la.counters, 0, 16, st));
  const int rp = ptab_for_stream(ix, st, &la.ptab, &la.pk);
  if (rp != SIGAX_OK) return rp;
  launch_locate_search(la, ix->wide, ix->n_cu, st);
  launch_locate_finish(la, st);
  launch_scan(la.cnt, la.n_queries, (u64*)(base + w.partial), d_hit_offs, la.status, st);  // status[0] = hit_offs[n]
  HIP_TRY(hipGetLastError());
  return SIGAX_OK;
}

int locate_walk_enqueue(sigax_index* ix, LocateArgs& la, sigax_hit* d_hits, u64* d_rows, u64 hits_cap, hipStream_t st) {
  la.hits = d_hits;
  la.rows = d_rows;
  la.hits_cap = hits_cap;
  launch_locate_walk(la, ix->wide, st);
  HIP_TRY(hipGetLastError());
  return SIGAX_OK;
}

}  // namespace

extern "C" int sigax_locate_workspace(uint64_t n_queries, uint64_t* bytes) {
  if (!bytes) return sigax_fail(SIGAX_E_ARG, "bad argument");
  *bytes = locate_work(n_queries).bytes;
  return SIGAX_OK;
}

extern "C" int sigax_locate_device(sigax_index* ix, const void* d_seqs, const void* d_offs, uint64_t n_queries, uint32_t flags,
                                   uint32_t max_hits, uint32_t max_len, void* d_totals, void* d_qflags, void* d_hit_offs, void* d_hits,
                                   void* d_rows, uint64_t hits_cap, void* d_status4, void* d_work, uint64_t work_bytes, void* stream) {
  if (!ix || (flags & ~SIGAX_RC)) return sigax_fail(SIGAX_E_ARG, "bad argument");
  if (n_queries && (!d_seqs || !d_offs || !d_totals || !d_qflags || !d_hit_offs || !d_status4 || !d_work || (hits_cap && !d_hits)))
    return sigax_fail(SIGAX_E_ARG, "NULL where a buffer is required");
  if (n_queries && ((((uintptr_t)d_hits | (uintptr_t)d_work) & 15) || ((uintptr_t)d_rows & 7)))
    return sigax_fail(SIGAX_E_ARG, "d_hits and d_work must be 16-byte aligned");
  if (n_queries > 0xFFFFFFFFull) return sigax_fail(SIGAX_E_ARG, "more than 2^32 - 1 queries: a hit names its query in 32 bits");
  if (locate_walk_slots(n_queries, max_hits, hits_cap) > LOCATE_MAX_SLOTS)
    return sigax_fail(SIGAX_E_ARG, "hits_cap, or n_queries * max_hits below it, is above the %llu hits one call walks", LOCATE_MAX_SLOTS);
  if (n_queries && work_bytes < locate_work(n_queries).bytes)
    return sigax_fail(SIGAX_E_ARG, "workspace of %llu bytes, %llu needed (sigax_locate_workspace)", (u64)work_bytes, locate_work(n_queries).bytes);
  const int rc = locate_usable(ix);
  if (rc != SIGAX_OK) return rc;
  HIP_TRY(hipSetDevice(ix->device));
  if (n_queries == 0) return SIGAX_OK;
  const hipStream_t st = (hipStream_t)stream;
  LocateArgs la = locate_args(ix, (const unsigned char*)d_seqs, (const u64*)d_offs, n_queries, flags, max_hits, max_len, (u64*)d_totals,
                              (uint32_t*)d_qflags, (u64*)d_hit_offs, (u64*)d_status4, d_work);
  const int rs = locate_search_enqueue(ix, la, (u64*)d_hit_offs, d_work, st);
  if (rs != SIGAX_OK) return rs;
  return locate_walk_enqueue(ix, la, (sigax_hit*)d_hits, (u64*)d_rows, hits_cap, st);
}

extern "C" int sigax_locate_batch(sigax_index* ix, const char* seqs, const uint64_t* offs, uint64_t n_queries, uint32_t flags,
                                  uint32_t max_hits, uint32_t max_len, uint64_t** totals, uint32_t** qflags, uint64_t** hit_offs,
                                  sigax_hit** hits) {
  if (!ix || (flags & ~SIGAX_RC) || !totals || !qflags || !hit_offs || !hits || (n_queries && (!seqs || !offs)))
    return sigax_fail(SIGAX_E_ARG, "bad argument");
  *totals = nullptr;
  *qflags = nullptr;
  *hit_offs = nullptr;
  *hits = nullptr;
  if (n_queries > 0xFFFFFFFFull) return sigax_fail(SIGAX_E_ARG, "more than 2^32 - 1 queries: a hit names its query in 32 bits");
  const int ru = locate_usable(ix);
  if (ru != SIGAX_OK) return ru;
  HIP_TRY(hipSetDevice(ix->device));
  const u64 n = n_queries;
  u64 n_hits = 0;
  DevGuard g;
  unsigned char* d_seqs = nullptr;
  u64 *d_offs = nullptr, *d_totals = nullptr, *d_hit_offs = nullptr, *d_status = nullptr;
  uint32_t* d_qflags = nullptr;
  sigax_hit* d_hits = nullptr;
  void* d_work = nullptr;
  // a stream of its own: calls from several host threads (two batches in flight) do not queue behind each other
  hipStream_t st = nullptr;
  struct StreamGuard {
    hipStream_t* s;
    ~StreamGuard() {
      if (*s) (void)hipStreamDestroy(*s);
    }
  } sg{&st};
  if (n) {
    HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    int rc = stage_strings(g, seqs, offs, n, 0xFFFFFFFFull, "query", st, &d_seqs, &d_offs);
    if (rc != SIGAX_OK) return rc;
    HIP_TRY(g.alloc((void**)&d_totals, (size_t)n * 8));
    HIP_TRY(g.alloc((void**)&d_qflags, (size_t)n * 4));
    HIP_TRY(g.alloc((void**)&d_hit_offs, ((size_t)n + 1) * 8));
    HIP_TRY(g.alloc((void**)&d_status, 32));
    HIP_TRY(g.alloc(&d_work, (size_t)locate_work(n).bytes));
    LocateArgs la = locate_args(ix, d_seqs, d_offs, n, flags, max_hits, max_len, d_totals, d_qflags, d_hit_offs, d_status, d_work);
    rc = locate_search_enqueue(ix, la, d_hit_offs, d_work, st);
    if (rc != SIGAX_OK) return rc;
    HIP_TRY(hipMemcpyAsync(&n_hits, d_status, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (n_hits > LOCATE_MAX_SLOTS) return sigax_fail(SIGAX_E_CAPACITY, "%llu hits listed, above the %llu one call walks", n_hits, LOCATE_MAX_SLOTS);
    if (n_hits) {
      HIP_TRY(g.alloc((void**)&d_hits, (size_t)n_hits * sizeof(sigax_hit)));
      rc = locate_walk_enqueue(ix, la, d_hits, nullptr, n_hits, st);
      if (rc != SIGAX_OK) return rc;
    }
  }
  HostGuard hg;
  uint64_t* h_totals = hg.alloc<uint64_t>((size_t)n * 8);
  uint32_t* h_qflags = hg.alloc<uint32_t>((size_t)n * 4);
  uint64_t* h_offs = hg.alloc<uint64_t>(((size_t)n + 1) * 8);
  sigax_hit* h_hits = hg.alloc<sigax_hit>((size_t)n_hits * sizeof(sigax_hit));
  if (!hg.ok) return sigax_fail(SIGAX_E_CAPACITY, "out of host memory");
  h_offs[0] = 0;
  hipError_t e = hipSuccess;
  if (n) {
    e = hipMemcpyAsync(h_totals, d_totals, (size_t)n * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(h_qflags, d_qflags, (size_t)n * 4, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(h_offs, d_hit_offs, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess && n_hits) e = hipMemcpyAsync(h_hits, d_hits, (size_t)n_hits * sizeof(sigax_hit), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
  }
  if (e != hipSuccess) return sigax_fail(SIGAX_E_DEVICE, "copying the hits: %s", hipGetErrorString(e));
  hg.release();
  *totals = h_totals;
  *qflags = h_qflags;
  *hit_offs = h_offs;
  *hits = h_hits;
  return SIGAX_OK;
}
