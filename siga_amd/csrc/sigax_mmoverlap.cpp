// siga_amd/csrc/sigax_mmoverlap.cpp -- `siga overlap -e` on the device: the entry points of sigax_mmoverlap.hip.
#include <cstring>

#include "sigax_internal.h"
#include "sigax_mmoverlap.h"

namespace {

int mmo_usable(const sigax_index* ix) {
  const int rc = seeded_usable(ix, "overlaps with mismatches need", "no overlap can be verified against");
  if (rc != SIGAX_OK) return rc;
  if (!ix->d_read_len || !ix->d_name_rank || ix->n_meta != ix->n_strings)
    return sigax_fail(SIGAX_E_STATE, "sigax_index_set_reads has not been called: overlaps with mismatches need the reads' name ranks");
  return SIGAX_OK;
}

int check_params(const sigax_mmo_params* p) {
  if (!p) return sigax_fail(SIGAX_E_ARG, "params is NULL");
  if (p->flags > SIGAX_MMO_CONTAINMENTS) return sigax_fail(SIGAX_E_ARG, "flags %u: 0 or SIGAX_MMO_CONTAINMENTS", p->flags);
  return seeded_check_params(p->seed_length, p->seed_stride, p->max_seed_hits, p->min_overlap, p->error_permille, p->max_candidates,
                             p->max_read_len, 0);
}

// the middle of the workspace: n_rec and n_flag, zeroed by the seeding stage (a read that ends early has none), then rec_offs;
// words[1] = the records of the call
struct MmoMiddle {
  u64 n_rec, n_flag, rec_offs, bytes;
};
MmoMiddle mmo_middle(u64 n) { return {0, up16(n * 4), 2 * up16(n * 4), 2 * up16(n * 4) + up16((n + 1) * 8)}; }
int mmo_work(u64 n, u64 n_bases, const sigax_mmo_params& p, u64 hits_cap, SeedWork* out) {
  return seed_work(n, n_bases, p.seed_length, p.seed_stride, hits_cap, mmo_middle(n).bytes, out);
}

// stages: 1 the seeds and their hits, 2 and k_mmo, 3 and the commit (the whole call)
int mmo_enqueue(sigax_index* ix, const unsigned char* d_ref_text, const u64* d_ref_offs, u64 first, u64 n, const sigax_mmo_params& p,
                sigax_mm_edge* d_edges, u64 edges_cap, u64* d_cursor, unsigned char* d_contained, u64* d_status, void* d_work, const SeedWork& w,
                u64 hits_cap, hipStream_t st, int stages = 3) {
  char* base = (char*)d_work;
  u64* words = (u64*)(base + w.words);
  const MmoMiddle m = mmo_middle(n);
  // the seeds of the reference text's reads first .. first + n
  const int rc = seed_enqueue(ix, d_ref_text, d_ref_offs + first, n, p.seed_length, p.seed_stride, p.max_read_len, p.max_seed_hits, d_work, w,
                              m.rec_offs, hits_cap, st);
  if (rc != SIGAX_OK) return rc;
  if (stages < 2) return SIGAX_OK;
  MmoArgs a;
  a.R = {d_ref_text, d_ref_offs, ix->n_strings};
  a.name_rank = ix->d_name_rank;
  a.first_read = first;
  a.n_reads = n;
  a.p = p;
  a.tab_cap = cand_tab_cap(p.max_candidates);
  a.L = seed_hits<uint4>(d_work, w, hits_cap);
  a.n_rec = (uint32_t*)(base + w.middle + m.n_rec);
  a.n_flag = (uint32_t*)(base + w.middle + m.n_flag);
  a.rec_offs = (u64*)(base + w.middle + m.rec_offs);
  a.rec_total = words + 1;
  a.edges = d_edges;
  a.edges_cap = edges_cap;
  a.cursor = d_cursor;
  a.contained = d_contained;
  a.counters = words + 8;
  a.status = d_status;
  const int e = launch_mmo(a, st);
  if (e != (int)hipSuccess)
    return sigax_fail(SIGAX_E_DEVICE, "the overlap kernel's %u bytes of LDS: %s", mmo_lds_bytes(a.tab_cap), hipGetErrorString((hipError_t)e));
  if (stages < 3) {
    HIP_TRY(hipGetLastError());
    return SIGAX_OK;
  }
  launch_scan(a.n_rec, n, (u64*)(base + w.partial), a.rec_offs, a.rec_total, st);
  launch_mmo_commit(a, st);
  HIP_TRY(hipGetLastError());
  return SIGAX_OK;
}

int mmoverlap_device(sigax_index* ix, const void* d_ref_text, const void* d_ref_offs, uint64_t first_read, uint64_t n_reads, uint64_t n_bases,
                     const sigax_mmo_params* params, sigax_mm_edge* d_edges, uint64_t edges_cap, void* d_cursor, void* d_contained, void* d_status8,
                     void* d_work, uint64_t work_bytes, uint64_t hits_cap, void* stream, int stages) {
  if (!ix) return sigax_fail(SIGAX_E_ARG, "bad argument");
  const int rp = check_params(params);
  if (rp != SIGAX_OK) return rp;
  const int ru = mmo_usable(ix);
  if (ru != SIGAX_OK) return ru;
  if (first_read > ix->n_strings || n_reads > ix->n_strings - first_read)
    return sigax_fail(SIGAX_E_ARG, "reads %llu .. %llu + %llu: the index holds %llu", (u64)first_read, (u64)first_read, (u64)n_reads, ix->n_strings);
  if (n_reads >= 0x80000000ull) return sigax_fail(SIGAX_E_ARG, "n_reads %llu: below 2^31", (u64)n_reads);
  if (!d_status8 || ((uintptr_t)d_status8 & 7)) return sigax_fail(SIGAX_E_ARG, "d_status8 is NULL or misaligned");
  HIP_TRY(hipSetDevice(ix->device));
  const hipStream_t st = (hipStream_t)stream;
  if (n_reads == 0) {
    HIP_TRY(hipMemsetAsync(d_status8, 0, 64, st));
    return SIGAX_OK;
  }
  if (!d_ref_text || !d_ref_offs || !d_cursor || !d_contained || !d_work || (!d_edges && edges_cap))
    return sigax_fail(SIGAX_E_ARG, "NULL where a buffer is required");
  if (((uintptr_t)d_work & 15) || ((uintptr_t)d_ref_offs & 7) || ((uintptr_t)d_cursor & 7) || ((uintptr_t)d_edges & 7))
    return sigax_fail(SIGAX_E_ARG, "d_work must be 16-byte aligned, d_ref_offs, d_cursor and d_edges 8-byte aligned");
  SeedWork w;
  sigax_mmo_params p = *params;
  p.max_read_len = seeded_max_len(p.max_read_len);
  const int rw = mmo_work(n_reads, n_bases, p, hits_cap, &w);
  if (rw != SIGAX_OK) return rw;
  if (work_bytes < w.bytes) return sigax_fail(SIGAX_E_ARG, "workspace of %llu bytes, %llu needed (sigax_mmoverlap_workspace)", (u64)work_bytes, w.bytes);
  return mmo_enqueue(ix, (const unsigned char*)d_ref_text, (const u64*)d_ref_offs, first_read, n_reads, p, d_edges, edges_cap, (u64*)d_cursor,
                     (unsigned char*)d_contained, (u64*)d_status8, d_work, w, hits_cap, st, stages);
}

// ---- finish ----
struct FinishWork {
  u64 keys0, keys1, vals0, vals1, sorted, head, scan, partial, sort_tmp, sort_tmp_bytes, bytes;
};
int finish_work(u64 n, FinishWork* out) {
  if (n > 0xFFFFFFFFull) return sigax_fail(SIGAX_E_ARG, "n_raw %llu: at most 2^32 - 1 records in one finish", n);
  FinishWork w;
  u64 at = 0;
  w.keys0 = at;
  at += up16(n * 8);
  w.keys1 = at;
  at += up16(n * 8);
  w.vals0 = at;
  at += up16(n * 8);
  w.vals1 = at;
  at += up16(n * 8);
  w.sorted = at;
  at += up16(n * sizeof(sigax_mm_edge));
  w.head = at;
  at += up16(n * 4);
  w.scan = at;
  at += up16((n + 1) * 8);
  w.partial = at;
  at += up16(scan_partials_needed(n) * 8);
  w.sort_tmp = at;
  u64 tb = 0;
  const hipError_t e = mmo_sort_bytes(n, &tb);
  if (e != hipSuccess) return sigax_fail(SIGAX_E_DEVICE, "the sort's workspace: %s", hipGetErrorString(e));
  w.sort_tmp_bytes = tb;
  at += up16(tb);
  w.bytes = at + 16;
  *out = w;
  return SIGAX_OK;
}

int finish_enqueue(sigax_mm_edge* d_edges, u64 n, u64* d_n_unique, void* d_work, const FinishWork& w, hipStream_t st) {
  char* base = (char*)d_work;
  MmoFinishArgs a;
  a.edges = d_edges;
  a.n = n;
  a.keys[0] = (u64*)(base + w.keys0);
  a.keys[1] = (u64*)(base + w.keys1);
  a.vals[0] = (u64*)(base + w.vals0);
  a.vals[1] = (u64*)(base + w.vals1);
  a.sorted = (sigax_mm_edge*)(base + w.sorted);
  a.head = (uint32_t*)(base + w.head);
  a.scan = (u64*)(base + w.scan);
  a.partial = (u64*)(base + w.partial);
  a.n_unique = d_n_unique;
  a.sort_tmp = base + w.sort_tmp;
  a.sort_tmp_bytes = w.sort_tmp_bytes;
  const hipError_t e = launch_mmo_finish(a, st);
  if (e != hipSuccess) return sigax_fail(SIGAX_E_DEVICE, "ordering the records: %s", hipGetErrorString(e));
  return SIGAX_OK;
}

}  // namespace

extern "C" int sigax_mmoverlap_workspace(uint64_t n_reads, uint64_t n_bases, const sigax_mmo_params* params, uint64_t hits_cap, uint64_t* bytes) {
  if (!bytes) return sigax_fail(SIGAX_E_ARG, "bad argument");
  const int rc = check_params(params);
  if (rc != SIGAX_OK) return rc;
  SeedWork w;
  const int rw = mmo_work(n_reads, n_bases, *params, hits_cap, &w);
  if (rw != SIGAX_OK) return rw;
  *bytes = w.bytes;
  return SIGAX_OK;
}

extern "C" int sigax_mmoverlap_device(sigax_index* ix, const void* d_ref_text, const void* d_ref_offs, uint64_t first_read, uint64_t n_reads,
                                      uint64_t n_bases, const sigax_mmo_params* params, sigax_mm_edge* d_edges, uint64_t edges_cap, void* d_cursor,
                                      void* d_contained, void* d_status8, void* d_work, uint64_t work_bytes, uint64_t hits_cap, void* stream) {
  return mmoverlap_device(ix, d_ref_text, d_ref_offs, first_read, n_reads, n_bases, params, d_edges, edges_cap, d_cursor, d_contained, d_status8,
                          d_work, work_bytes, hits_cap, stream, 3);
}

extern "C" int sigax_mmoverlap_stages_device(sigax_index* ix, const void* d_ref_text, const void* d_ref_offs, uint64_t first_read, uint64_t n_reads,
                                             uint64_t n_bases, const sigax_mmo_params* params, sigax_mm_edge* d_edges, uint64_t edges_cap,
                                             void* d_cursor, void* d_contained, void* d_status8, void* d_work, uint64_t work_bytes, uint64_t hits_cap,
                                             void* stream, int stages) {
  if (stages < 1 || stages > 2) return sigax_fail(SIGAX_E_ARG, "stages %d: 1 or 2", stages);
  return mmoverlap_device(ix, d_ref_text, d_ref_offs, first_read, n_reads, n_bases, params, d_edges, edges_cap, d_cursor, d_contained, d_status8,
                          d_work, work_bytes, hits_cap, stream, stages);
}

extern "C" int sigax_mmoverlap_finish_workspace(uint64_t n_raw, uint64_t* bytes) {
  if (!bytes) return sigax_fail(SIGAX_E_ARG, "bad argument");
  FinishWork w;
  const int rc = finish_work(n_raw, &w);
  if (rc != SIGAX_OK) return rc;
  *bytes = w.bytes;
  return SIGAX_OK;
}

extern "C" int sigax_mmoverlap_finish_device(sigax_mm_edge* d_edges, uint64_t n_raw, void* d_n_unique, void* d_work, uint64_t work_bytes,
                                             void* stream) {
  if (!d_n_unique || ((uintptr_t)d_n_unique & 7)) return sigax_fail(SIGAX_E_ARG, "d_n_unique is NULL or misaligned");
  if (n_raw && (!d_edges || !d_work)) return sigax_fail(SIGAX_E_ARG, "NULL where a buffer is required");
  if (((uintptr_t)d_work & 15) || ((uintptr_t)d_edges & 7)) return sigax_fail(SIGAX_E_ARG, "d_work must be 16-byte aligned, d_edges 8-byte aligned");
  FinishWork w;
  const int rc = finish_work(n_raw, &w);
  if (rc != SIGAX_OK) return rc;
  if (n_raw && work_bytes < w.bytes)
    return sigax_fail(SIGAX_E_ARG, "workspace of %llu bytes, %llu needed (sigax_mmoverlap_finish_workspace)", (u64)work_bytes, w.bytes);
  return finish_enqueue(d_edges, n_raw, (u64*)d_n_unique, d_work, w, (hipStream_t)stream);
}

// Test hooks, read per call: the reads a piece holds at most, the hits its first try has room for, the records the first buffer
// has room for.
extern "C" int sigax_mmoverlap_batch(sigax_index* ix, const sigax_pile_ref* ref, const sigax_mmo_params* params, sigax_mm_edge** edges,
                                     uint64_t* n_edges, uint8_t* contained, uint64_t status8[8]) {
  if (!ix || !ref || !edges || !n_edges) return sigax_fail(SIGAX_E_ARG, "bad argument");
  *edges = nullptr;
  *n_edges = 0;
  const int rp = check_params(params);
  if (rp != SIGAX_OK) return rp;
  const int ru = mmo_usable(ix);
  if (ru != SIGAX_OK) return ru;
  const void *rt = nullptr, *ro = nullptr;
  uint64_t tb = 0;
  const int rb = sigax_pile_ref_buffers(ref, &rt, &ro, &tb);
  if (rb != SIGAX_OK) return rb;
  if (tb != ix->n_symbols - ix->n_strings) return sigax_fail(SIGAX_E_ARG, "the reference text is not this index's");
  if (status8) memset(status8, 0, 64);
  const u64 n = ix->n_strings;
  if (n == 0) return SIGAX_OK;
  if (!contained) return sigax_fail(SIGAX_E_ARG, "NULL where a buffer is required");
  if (n >= 0x80000000ull) return sigax_fail(SIGAX_E_ARG, "%llu reads: below 2^31", n);
  HIP_TRY(hipSetDevice(ix->device));
  const unsigned char* d_text = (const unsigned char*)rt;
  const u64* d_offs = (const u64*)ro;
  std::vector<u64> offs((size_t)n + 1);
  HIP_TRY(hipMemcpy(offs.data(), d_offs, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost));
  sigax_mmo_params p = *params;
  p.max_read_len = seeded_max_len(p.max_read_len, offs.data(), n);
  const u64 piece_max = std::max<u64>(1, env_u64("SIGAX_TEST_MMO_PIECE", 1ull << 18));
  const u64 first_hits = env_u64("SIGAX_TEST_MMO_HITS_CAP", ~0ull);
  hipStream_t st = (hipStream_t)0;
  DevGuard keep;
  unsigned char* d_contained = nullptr;
  u64 *d_cursor = nullptr, *d_status = nullptr;
  HIP_TRY(keep.alloc((void**)&d_contained, (size_t)n));
  HIP_TRY(keep.alloc((void**)&d_cursor, 16));
  HIP_TRY(keep.alloc((void**)&d_status, 64));
  HIP_TRY(hipMemsetAsync(d_contained, 0, (size_t)n, st));
  HIP_TRY(hipMemsetAsync(d_cursor, 0, 16, st));
  // the records: one buffer that grows by what a call reports and what the reads still to come may need
  sigax_mm_edge* d_edges = nullptr;
  u64 edges_cap = env_u64("SIGAX_TEST_MMO_EDGES_CAP", std::max<u64>(4096, n * 16));
  HIP_TRY(hipMalloc((void**)&d_edges, (size_t)std::max<u64>(edges_cap, 1) * sizeof(sigax_mm_edge)));
  struct EdgeBuf {
    sigax_mm_edge** p;
    ~EdgeBuf() {
      if (*p) (void)hipFree(*p);
    }
  } edge_guard{&d_edges};
  u64 cursor = 0, total[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  u64 b = 0, piece = std::min(piece_max, n);
  while (b < n) {
    const u64 e = std::min(n, b + piece), cnt = e - b, nb = offs[e] - offs[b];
    size_t mfree = 0, mtotal = 0;
    HIP_TRY(hipMemGetInfo(&mfree, &mtotal));
    const u64 budget = (u64)mfree / 2;
    u64 hits_cap = seeded_first_hits_cap(first_hits, nb, budget);
    bool done = false, split = false;
    for (int attempt = 0; attempt < 3 && !done && !split; ++attempt) {
      SeedWork w;
      const int rw = mmo_work(cnt, nb, p, hits_cap, &w);
      if (rw != SIGAX_OK) return rw;
      if (w.bytes > budget && cnt > 1) {
        split = true;
        break;
      }
      DevGuard g;
      void* d_work = nullptr;
      HIP_TRY(g.alloc(&d_work, (size_t)w.bytes));
      const int rc = mmo_enqueue(ix, d_text, d_offs, b, cnt, p, d_edges, edges_cap, d_cursor, d_contained, d_status, d_work, w, hits_cap, st);
      if (rc != SIGAX_OK) return rc;
      u64 status[8];
      HIP_TRY(hipMemcpyAsync(status, d_status, 64, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      if (status[0] > hits_cap) {
        const int ro = seeded_hits_overflow(status[0], budget, cnt, &hits_cap, &split);
        if (ro != SIGAX_OK) return ro;
        continue;
      }
      if (status[7] > edges_cap - cursor) {  // nothing was written: room for these and, at this rate, for the reads to come
        const u64 need = cursor + status[7];
        const u64 grown = need + (u64)((double)need / (double)e * (double)(n - e) * 1.1);
        sigax_mm_edge* bigger = nullptr;
        hipError_t he = hipMalloc((void**)&bigger, (size_t)grown * sizeof(sigax_mm_edge));
        u64 got = grown;
        if (he != hipSuccess && grown > need) {
          (void)hipGetLastError();
          he = hipMalloc((void**)&bigger, (size_t)need * sizeof(sigax_mm_edge));
          got = need;
        }
        if (he != hipSuccess) return sigax_fail(SIGAX_E_CAPACITY, "%llu overlap records do not fit the device: %s", need, hipGetErrorString(he));
        if (cursor) HIP_TRY(hipMemcpy(bigger, d_edges, (size_t)cursor * sizeof(sigax_mm_edge), hipMemcpyDeviceToDevice));
        (void)hipFree(d_edges);
        d_edges = bigger;
        edges_cap = got;
        continue;
      }
      cursor += status[7];
      for (int k = 0; k < 8; ++k) total[k] += status[k];
      done = true;
    }
    if (done) {
      b = e;
    } else {
      if (cnt == 1) return sigax_fail(SIGAX_E_CAPACITY, "one read of %llu bases does not fit the device", nb);
      piece = (cnt + 1) / 2;
    }
  }
  // every piece's records at once: a pair whose reads lie in two pieces was written by both
  u64 n_unique = 0;
  if (cursor) {
    FinishWork fw;
    const int rf = finish_work(cursor, &fw);
    if (rf != SIGAX_OK) return rf;
    DevGuard g;
    void* d_work = nullptr;
    const hipError_t he = g.alloc(&d_work, (size_t)fw.bytes);
    if (he != hipSuccess)
      return sigax_fail(SIGAX_E_CAPACITY, "ordering %llu overlap records needs %llu bytes of device memory: %s", cursor, fw.bytes, hipGetErrorString(he));
    const int rc = finish_enqueue(d_edges, cursor, d_cursor + 1, d_work, fw, st);
    if (rc != SIGAX_OK) return rc;
    HIP_TRY(hipMemcpyAsync(&n_unique, d_cursor + 1, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (n_unique > cursor) return sigax_fail(SIGAX_E_DEVICE, "%llu records after ordering %llu", n_unique, cursor);
  }
  HostGuard hg;
  sigax_mm_edge* out = hg.alloc<sigax_mm_edge>((size_t)n_unique * sizeof(sigax_mm_edge));
  if (!hg.ok) return sigax_fail(SIGAX_E_CAPACITY, "out of host memory for %llu overlap records", n_unique);
  if (n_unique) HIP_TRY(hipMemcpy(out, d_edges, (size_t)n_unique * sizeof(sigax_mm_edge), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(contained, d_contained, (size_t)n, hipMemcpyDeviceToHost));
  if (status8) memcpy(status8, total, 64);
  hg.release();
  *edges = out;
  *n_edges = n_unique;
  return SIGAX_OK;
}
