// siga_amd/csrc/sigax_pileup.cpp -- `siga correct -a overlap` on the device: the entry points of sigax_pileup.hip.
#include <cstring>

#include "sigax_internal.h"
#include "sigax_pileup.h"

namespace {

int pile_usable(const sigax_index* ix) { return seeded_usable(ix, "the pile-up needs", "no pile can be built from"); }

// ---- one round ----
int check_params(const sigax_pile_params* p) {
  if (!p) return sigax_fail(SIGAX_E_ARG, "params is NULL");
  if (p->conflict < 1) return sigax_fail(SIGAX_E_ARG, "conflict 0: from 1");
  if (p->min_depth < 1) return sigax_fail(SIGAX_E_ARG, "min_depth 0: from 1");
  return seeded_check_params(p->seed_length, p->seed_stride, p->max_seed_hits, p->min_overlap, p->error_permille, p->max_candidates,
                             p->max_read_len, p->reserved);
}

int pile_work(u64 n, u64 n_bases, const sigax_pile_params& p, u64 hits_cap, SeedWork* out) {
  return seed_work(n, n_bases, p.seed_length, p.seed_stride, hits_cap, 0, out);  // nothing of its own between the seeds' parts
}

// pile_only: the seeds and hits are in d_work already (sigax_pileup_pile_device)
int pile_enqueue(sigax_index* ix, const unsigned char* d_seqs, const u64* d_offs, u64 n, u64 n_bases, const sigax_pile_params& p,
                 const unsigned char* d_ref_text, const u64* d_ref_offs, unsigned char* d_out, unsigned char* d_valid,
                 unsigned char* d_changed, u64* d_status, void* d_work, const SeedWork& w, u64 hits_cap, hipStream_t st,
                 bool pile_only = false) {
  u64* words = (u64*)((char*)d_work + w.words);
  PileArgs a;
  a.seqs = d_seqs;
  a.offs = d_offs;
  a.n_reads = n;
  a.p = p;
  a.len_cap = (p.max_read_len + 63u) & ~63u;
  a.tab_cap = cand_tab_cap(p.max_candidates);
  a.L = seed_hits<const uint4>(d_work, w, hits_cap);
  a.R = {d_ref_text, d_ref_offs, ix->n_strings};
  a.out_seqs = d_out;
  a.valid = d_valid;
  a.changed = d_changed;
  a.counters = words + 8;
  a.status = d_status;
  if (pile_only) {
    HIP_TRY(hipMemsetAsync(words + 8, 0, 64, st));
    const int e = launch_pile(a, st);
    if (e != (int)hipSuccess) return sigax_fail(SIGAX_E_DEVICE, "the pile-up kernel: %s", hipGetErrorString((hipError_t)e));
    launch_pile_status(a, st);
    HIP_TRY(hipGetLastError());
    return SIGAX_OK;
  }
  const int rc = seed_enqueue(ix, d_seqs, d_offs, n, p.seed_length, p.seed_stride, p.max_read_len, p.max_seed_hits, d_work, w, 0, hits_cap, st);
  if (rc != SIGAX_OK) return rc;
  const int e = launch_pile(a, st);
  if (e != (int)hipSuccess)
    return sigax_fail(SIGAX_E_DEVICE, "the pile-up kernel's %u bytes of LDS: %s", pile_lds_bytes(a.len_cap, a.tab_cap), hipGetErrorString((hipError_t)e));
  launch_pile_status(a, st);
  HIP_TRY(hipGetLastError());
  return SIGAX_OK;
}

}  // namespace

extern "C" int sigax_pileup_workspace(uint64_t n_reads, uint64_t n_bases, const sigax_pile_params* params, uint64_t hits_cap, uint64_t* bytes) {
  if (!bytes) return sigax_fail(SIGAX_E_ARG, "bad argument");
  const int rc = check_params(params);
  if (rc != SIGAX_OK) return rc;
  SeedWork w;
  const int rw = pile_work(n_reads, n_bases, *params, hits_cap, &w);
  if (rw != SIGAX_OK) return rw;
  *bytes = w.bytes;
  return SIGAX_OK;
}

static int pileup_device(sigax_index* ix, const void* d_seqs, const void* d_offs, uint64_t n_reads, uint64_t n_bases,
                         const sigax_pile_params* params, const void* d_ref_text, const void* d_ref_offs, void* d_out_seqs, void* d_valid,
                         void* d_changed, void* d_status8, void* d_work, uint64_t work_bytes, uint64_t hits_cap, void* stream,
                         bool pile_only) {
  if (!ix) return sigax_fail(SIGAX_E_ARG, "bad argument");
  const int rp = check_params(params);
  if (rp != SIGAX_OK) return rp;
  const int ru = pile_usable(ix);
  if (ru != SIGAX_OK) return ru;
  if (n_reads >= 0x80000000ull) return sigax_fail(SIGAX_E_ARG, "n_reads %llu: below 2^31", (u64)n_reads);
  if (!d_status8 || ((uintptr_t)d_status8 & 7)) return sigax_fail(SIGAX_E_ARG, "d_status8 is NULL or misaligned");
  HIP_TRY(hipSetDevice(ix->device));
  const hipStream_t st = (hipStream_t)stream;
  if (n_reads == 0) {
    HIP_TRY(hipMemsetAsync(d_status8, 0, 64, st));
    return SIGAX_OK;
  }
  if (!d_seqs || !d_offs || !d_ref_text || !d_ref_offs || !d_out_seqs || !d_valid || !d_changed || !d_work)
    return sigax_fail(SIGAX_E_ARG, "NULL where a buffer is required");
  if (((uintptr_t)d_work & 15) || ((uintptr_t)d_offs & 7) || ((uintptr_t)d_ref_offs & 7))
    return sigax_fail(SIGAX_E_ARG, "d_work must be 16-byte aligned, d_offs and d_ref_offs 8-byte aligned");
  SeedWork w;
  sigax_pile_params p = *params;
  p.max_read_len = seeded_max_len(p.max_read_len);
  const int rw = pile_work(n_reads, n_bases, p, hits_cap, &w);
  if (rw != SIGAX_OK) return rw;
  if (work_bytes < w.bytes) return sigax_fail(SIGAX_E_ARG, "workspace of %llu bytes, %llu needed (sigax_pileup_workspace)", (u64)work_bytes, w.bytes);
  return pile_enqueue(ix, (const unsigned char*)d_seqs, (const u64*)d_offs, n_reads, n_bases, p, (const unsigned char*)d_ref_text,
                      (const u64*)d_ref_offs, (unsigned char*)d_out_seqs, (unsigned char*)d_valid, (unsigned char*)d_changed, (u64*)d_status8,
                      d_work, w, hits_cap, st, pile_only);
}

extern "C" int sigax_pileup_device(sigax_index* ix, const void* d_seqs, const void* d_offs, uint64_t n_reads, uint64_t n_bases,
                                   const sigax_pile_params* params, const void* d_ref_text, const void* d_ref_offs, void* d_out_seqs,
                                   void* d_valid, void* d_changed, void* d_status8, void* d_work, uint64_t work_bytes, uint64_t hits_cap,
                                   void* stream) {
  return pileup_device(ix, d_seqs, d_offs, n_reads, n_bases, params, d_ref_text, d_ref_offs, d_out_seqs, d_valid, d_changed, d_status8, d_work,
                       work_bytes, hits_cap, stream, false);
}

extern "C" int sigax_pileup_pile_device(sigax_index* ix, const void* d_seqs, const void* d_offs, uint64_t n_reads, uint64_t n_bases,
                                        const sigax_pile_params* params, const void* d_ref_text, const void* d_ref_offs, void* d_out_seqs,
                                        void* d_valid, void* d_changed, void* d_status8, void* d_work, uint64_t work_bytes,
                                        uint64_t hits_cap, void* stream) {
  return pileup_device(ix, d_seqs, d_offs, n_reads, n_bases, params, d_ref_text, d_ref_offs, d_out_seqs, d_valid, d_changed, d_status8, d_work,
                       work_bytes, hits_cap, stream, true);
}

namespace {

// One round over m reads in host memory (offsets from 0), in pieces that fit the device: out, valid, changed and the status
// words added to status8.  Test hooks, read per call: the reads a piece holds at most, the hits its first try has room for.
int round_on_device(sigax_index* ix, const sigax_pile_ref* ref, const char* seqs, const u64* offs, u64 m, const sigax_pile_params& p,
                    char* out, uint8_t* valid, uint8_t* changed, u64 status8[8]) {
  const u64 piece_max = std::max<u64>(1, env_u64("SIGAX_TEST_PILE_PIECE", 1ull << 18));
  const u64 first_cap = env_u64("SIGAX_TEST_PILE_HITS_CAP", ~0ull);
  hipStream_t st = (hipStream_t)0;
  u64 b = 0;
  u64 piece = std::min(piece_max, m);
  while (b < m) {
    const u64 e = std::min(m, b + piece), cnt = e - b, nb = offs[e] - offs[b];
    size_t mfree = 0, mtotal = 0;
    HIP_TRY(hipMemGetInfo(&mfree, &mtotal));
    const u64 budget = (u64)mfree / 2;
    u64 hits_cap = seeded_first_hits_cap(first_cap, nb, budget);
    bool done = false, split = false;
    for (int attempt = 0; attempt < 2 && !done && !split; ++attempt) {
      SeedWork w;
      const int rw = pile_work(cnt, nb, p, hits_cap, &w);
      if (rw != SIGAX_OK) return rw;
      if (w.bytes + 2 * nb + 10 * cnt > budget && cnt > 1) {
        split = true;
        break;
      }
      DevGuard g;
      unsigned char *d_seqs = nullptr, *d_out = nullptr, *d_valid = nullptr, *d_changed = nullptr;
      u64 *d_offs = nullptr, *d_status = nullptr;
      void* d_work = nullptr;
      const int rs = stage_strings(g, seqs, (const uint64_t*)(offs + b), cnt, ~0ull, "read", st, &d_seqs, &d_offs);
      if (rs != SIGAX_OK) return rs;
      HIP_TRY(g.alloc((void**)&d_out, (size_t)nb + 16));
      HIP_TRY(g.alloc((void**)&d_valid, (size_t)cnt));
      HIP_TRY(g.alloc((void**)&d_changed, (size_t)cnt));
      HIP_TRY(g.alloc((void**)&d_status, 64));
      HIP_TRY(g.alloc(&d_work, (size_t)w.bytes));
      const int rc = pile_enqueue(ix, d_seqs, d_offs, cnt, nb, p, ref->d_text, ref->d_offs, d_out, d_valid, d_changed, d_status, d_work, w,
                                  hits_cap, st);
      if (rc != SIGAX_OK) return rc;
      u64 status[8];
      HIP_TRY(hipMemcpyAsync(status, d_status, 64, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      if (status[0] > hits_cap) {
        const int ro = seeded_hits_overflow(status[0], budget, cnt, &hits_cap, &split);
        if (ro != SIGAX_OK) return ro;
        continue;
      }
      HIP_TRY(hipMemcpyAsync(out + offs[b], d_out, (size_t)nb, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipMemcpyAsync(valid + b, d_valid, (size_t)cnt, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipMemcpyAsync(changed + b, d_changed, (size_t)cnt, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      for (int k = 0; k < 8; ++k) status8[k] += status[k];
      done = true;
    }
    if (done) {
      b = e;
    } else {
      if (cnt == 1) return sigax_fail(SIGAX_E_CAPACITY, "one read of %llu bases does not fit the device", nb);
      piece = (cnt + 1) / 2;
    }
  }
  return SIGAX_OK;
}

}  // namespace

extern "C" int sigax_pileup_batch(sigax_index* ix, const sigax_pile_ref* ref, const char* seqs, const uint64_t* offs, uint64_t n_reads,
                                  const sigax_pile_params* params, uint32_t rounds, char* out_seqs, uint8_t* valid, uint8_t* changed,
                                  uint64_t status8[8], uint32_t* rounds_run) {
  if (!ix || !ref) return sigax_fail(SIGAX_E_ARG, "bad argument");
  const int rp = check_params(params);
  if (rp != SIGAX_OK) return rp;
  if (rounds < 1) return sigax_fail(SIGAX_E_ARG, "rounds 0: from 1");
  const int ru = pile_usable(ix);
  if (ru != SIGAX_OK) return ru;
  if (ref->device != ix->device || ref->n_strings != ix->n_strings || ref->text_bytes != ix->n_symbols - ix->n_strings)
    return sigax_fail(SIGAX_E_ARG, "the reference text is not this index's");
  if (status8) memset(status8, 0, 64);
  if (rounds_run) *rounds_run = 0;
  if (n_reads == 0) return SIGAX_OK;
  if (!seqs || !offs || !out_seqs || !valid || !changed) return sigax_fail(SIGAX_E_ARG, "NULL where a buffer is required");
  if (n_reads >= 0x80000000ull) return sigax_fail(SIGAX_E_ARG, "n_reads %llu: below 2^31", (u64)n_reads);
  for (u64 i = 0; i < n_reads; ++i)
    if (offs[i + 1] < offs[i]) return sigax_fail(SIGAX_E_ARG, "read %llu: bad offsets", i);
  HIP_TRY(hipSetDevice(ix->device));
  sigax_pile_params p = *params;
  p.max_read_len = seeded_max_len(p.max_read_len, (const u64*)offs, n_reads);  // the LDS of a wave follows the batch's longest read
  const u64 b0 = offs[0];
  memcpy(out_seqs + b0, seqs + b0, (size_t)(offs[n_reads] - b0));
  memset(valid, 0, (size_t)n_reads);
  memset(changed, 0, (size_t)n_reads);
  u64 total[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  std::vector<u64> active((size_t)n_reads), next;
  for (u64 i = 0; i < n_reads; ++i) active[(size_t)i] = i;
  std::vector<char> in, res;
  std::vector<u64> po;
  std::vector<uint8_t> v, ch;
  uint32_t run = 0;
  while (run < rounds && !active.empty()) {
    const u64 m = active.size();
    po.assign((size_t)m + 1, 0);
    for (u64 k = 0; k < m; ++k) po[(size_t)k + 1] = po[(size_t)k] + (offs[active[(size_t)k] + 1] - offs[active[(size_t)k]]);
    in.resize((size_t)po[(size_t)m] + 1);
    res.resize((size_t)po[(size_t)m] + 1);
    for (u64 k = 0; k < m; ++k) memcpy(in.data() + po[(size_t)k], out_seqs + offs[active[(size_t)k]], (size_t)(po[(size_t)k + 1] - po[(size_t)k]));
    v.assign((size_t)m, 0);
    ch.assign((size_t)m, 0);
    const int rc = round_on_device(ix, ref, in.data(), po.data(), m, p, res.data(), v.data(), ch.data(), total);
    if (rc != SIGAX_OK) return rc;
    ++run;
    next.clear();
    for (u64 k = 0; k < m; ++k) {
      const u64 i = active[(size_t)k];
      memcpy(out_seqs + offs[i], res.data() + po[(size_t)k], (size_t)(po[(size_t)k + 1] - po[(size_t)k]));
      valid[i] = v[(size_t)k];
      if (ch[(size_t)k]) {
        changed[i] = 1;
        next.push_back(i);
      }
    }
    active.swap(next);
  }
  if (status8) memcpy(status8, total, 64);
  if (rounds_run) *rounds_run = run;
  return SIGAX_OK;
}
