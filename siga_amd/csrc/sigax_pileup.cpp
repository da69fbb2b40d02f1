// siga_amd/csrc/sigax_pileup.cpp -- `siga correct -a overlap` on the device: the entry points of sigax_pileup.hip.
#include <cstring>

#include "sigax_internal.h"
#include "sigax_pileup.h"

namespace {

#define PILE_REF_MAX_LEN 0x3FFFFFFFu  // reference reads are shorter than 2^30 bases (the diagonal's 31 bits, sigax_pileup.hip)

u64 up16(u64 v) { return (v + 15) & ~15ull; }

int pile_usable(const sigax_index* ix) {
  if (!ix->d_sai[0] || ix->n_sai != ix->n_strings)
    return sigax_fail(SIGAX_E_STATE, "the index was opened without its forward .sai table: the pile-up needs it to name the reads");
  if (ix->st[0].C[1] != ix->n_strings)
    return sigax_fail(SIGAX_E_STATE, "reads with non-ACGT bases in the index: stretches are not reads, no pile can be built from them");
  return SIGAX_OK;
}

// ---- reference text ----
struct RefWork {
  u64 rows, stretch, rows_by_id, lens, lens_by_id, partial, words, bytes;
};
RefWork ref_work(u64 n) {
  RefWork w;
  u64 at = 0;
  w.rows = at;
  at += up16(n * 8);
  w.stretch = at;
  at += up16(n * 8);
  w.rows_by_id = at;
  at += up16(n * 8);
  w.lens = at;
  at += up16(n * 4);
  w.lens_by_id = at;
  at += up16(n * 4);
  w.partial = at;
  at += up16(scan_partials_needed(n) * 8);
  w.words = at;  // 8 u64: [0..2] the walk's status, [3] total bases, [4] rows without a read, [5] reads
  at += 64;
  w.bytes = at;
  return w;
}

int ref_text_enqueue(sigax_index* ix, unsigned char* d_text, u64* d_offs, u64* d_status, void* d_work, hipStream_t st) {
  const u64 n = ix->n_strings;
  const RefWork w = ref_work(n);
  char* base = (char*)d_work;
  u64* rows = (u64*)(base + w.rows);
  u64* stretch = (u64*)(base + w.stretch);
  u64* rows_by_id = (u64*)(base + w.rows_by_id);
  u32* lens = (u32*)(base + w.lens);
  u32* lens_by_id = (u32*)(base + w.lens_by_id);
  u64* words = (u64*)(base + w.words);
  HIP_TRY(hipMemsetAsync(words, 0, 64, st));
  HIP_TRY(hipMemsetAsync(rows_by_id, 0xFF, (size_t)n * 8, st));  // a read no row names: a row out of range, length 0
  HIP_TRY(hipMemsetAsync(lens_by_id, 0, (size_t)n * 4, st));
  HIP_TRY(hipMemcpyAsync(words + 5, &ix->n_strings, 8, hipMemcpyHostToDevice, st));
  launch_ref_iota(rows, n, st);
  HIP_TRY(hipGetLastError());
  int rc = sigax_string_lengths_device(ix, 0, rows, n, PILE_REF_MAX_LEN, lens, stretch, words, st);
  if (rc != SIGAX_OK) return rc;
  RefOrderArgs ra;
  ra.lens = lens;
  ra.stretch = stretch;
  ra.sai = ix->d_sai[0];
  ra.n = n;
  ra.rows_by_id = rows_by_id;
  ra.lens_by_id = lens_by_id;
  ra.bad = words + 4;
  launch_ref_order(ra, st);
  launch_scan(lens_by_id, n, (u64*)(base + w.partial), d_offs, words + 3, st);
  HIP_TRY(hipGetLastError());
  rc = sigax_get_strings_device(ix, 0, rows_by_id, n, PILE_REF_MAX_LEN, d_offs, d_text, words, st);
  if (rc != SIGAX_OK) return rc;
  // {reads, bases, rows that gave no read, slots of the wrong size}
  HIP_TRY(hipMemcpyAsync(d_status + 0, words + 5, 8, hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_status + 1, words + 3, 8, hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_status + 2, words + 4, 8, hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_status + 3, words + 2, 8, hipMemcpyDeviceToDevice, st));
  return SIGAX_OK;
}

// ---- one round ----
int check_params(const sigax_pile_params* p) {
  if (!p) return sigax_fail(SIGAX_E_ARG, "params is NULL");
  if (p->seed_length < 12 || p->seed_length > 64) return sigax_fail(SIGAX_E_ARG, "seed_length %u: 12..64", p->seed_length);
  if (p->seed_stride < 1 || p->seed_stride > p->seed_length) return sigax_fail(SIGAX_E_ARG, "seed_stride %u: 1..seed_length", p->seed_stride);
  if (p->max_seed_hits < 1 || p->max_seed_hits > 4096) return sigax_fail(SIGAX_E_ARG, "max_seed_hits %u: 1..4096", p->max_seed_hits);
  if (p->min_overlap < 1) return sigax_fail(SIGAX_E_ARG, "min_overlap 0: from 1");
  if (p->error_permille > 250) return sigax_fail(SIGAX_E_ARG, "error_permille %u: 0..250", p->error_permille);
  if (p->conflict < 1) return sigax_fail(SIGAX_E_ARG, "conflict 0: from 1");
  if (p->min_depth < 1) return sigax_fail(SIGAX_E_ARG, "min_depth 0: from 1");
  if (p->max_candidates < 1 || p->max_candidates > 4096) return sigax_fail(SIGAX_E_ARG, "max_candidates %u: 1..4096", p->max_candidates);
  if (p->max_read_len > SIGAX_PILE_MAX_LEN) return sigax_fail(SIGAX_E_ARG, "max_read_len %u: 0..%u", p->max_read_len, SIGAX_PILE_MAX_LEN);
  if (p->reserved != 0) return sigax_fail(SIGAX_E_ARG, "reserved must be 0");
  return SIGAX_OK;
}

struct PileWork {
  u64 seed_cap;
  u64 seed_cnt, seed_start, partial, words, seed_bytes, seed_offs, totals, qflags, hit_offs, loc_work, loc_work_bytes, hits, bytes;
};
int pile_work(u64 n, u64 n_bases, const sigax_pile_params& p, u64 hits_cap, PileWork* out) {
  PileWork w;
  // a read of n bases has at most n / T + 1 seeds: (n - S) / T + 2 <= n / T + 1 with S >= T
  w.seed_cap = n_bases / p.seed_stride + n;
  if (w.seed_cap == 0) w.seed_cap = 1;
  if (w.seed_cap > 0xFFFFFFFFull) return sigax_fail(SIGAX_E_ARG, "%llu seed slots: a hit names its seed in 32 bits", w.seed_cap);
  if (hits_cap > LOCATE_MAX_SLOTS) return sigax_fail(SIGAX_E_ARG, "hits_cap above the %llu hits one call walks", LOCATE_MAX_SLOTS);
  u64 at = 0;
  w.seed_cnt = at;
  at += up16(n * 4);
  w.seed_start = at;
  at += up16((n + 1) * 8);
  w.partial = at;
  at += up16(scan_partials_needed(n) * 8);
  w.words = at;  // [0] seeds, [1..] reserved, [4..7] locate's status, [8..15] the round's counters
  at += 128;
  w.seed_bytes = at;
  at += up16(w.seed_cap * p.seed_length + 16);
  w.seed_offs = at;
  at += up16((w.seed_cap + 1) * 8);
  w.totals = at;
  at += up16(w.seed_cap * 8);
  w.qflags = at;
  at += up16(w.seed_cap * 4);
  w.hit_offs = at;
  at += up16((w.seed_cap + 1) * 8);
  w.loc_work = at;
  uint64_t lw = 0;
  const int rc = sigax_locate_workspace(w.seed_cap, &lw);
  if (rc != SIGAX_OK) return rc;
  w.loc_work_bytes = lw;
  at += up16(lw);
  w.hits = at;
  at += hits_cap * 16;
  w.bytes = at + 16;
  *out = w;
  return SIGAX_OK;
}

sigax_pile_params with_len(const sigax_pile_params& p) {
  sigax_pile_params q = p;
  if (q.max_read_len == 0) q.max_read_len = SIGAX_PILE_MAX_LEN;
  return q;
}

// pile_only: the seeds and hits are in d_work already (sigax_pileup_pile_device)
int pile_enqueue(sigax_index* ix, const unsigned char* d_seqs, const u64* d_offs, u64 n, u64 n_bases, const sigax_pile_params& p,
                 const unsigned char* d_ref_text, const u64* d_ref_offs, unsigned char* d_out, unsigned char* d_valid,
                 unsigned char* d_changed, u64* d_status, void* d_work, const PileWork& w, u64 hits_cap, hipStream_t st,
                 bool pile_only = false) {
  char* base = (char*)d_work;
  u64* words = (u64*)(base + w.words);
  PileArgs a;
  a.seqs = d_seqs;
  a.offs = d_offs;
  a.n_reads = n;
  a.p = p;
  a.len_cap = (p.max_read_len + 63u) & ~63u;
  a.tab_cap = pile_tab_cap(p.max_candidates);
  a.seed_cnt = (uint32_t*)(base + w.seed_cnt);
  a.seed_start = (u64*)(base + w.seed_start);
  a.seed_total = words;
  a.seed_cap = w.seed_cap;
  a.seed_bytes = (unsigned char*)(base + w.seed_bytes);
  a.seed_offs = (u64*)(base + w.seed_offs);
  a.qflags = (const uint32_t*)(base + w.qflags);
  a.hit_offs = (const u64*)(base + w.hit_offs);
  a.hits = (const sigax_hit*)(base + w.hits);
  a.hits_cap = hits_cap;
  a.loc_status = words + 4;
  a.ref_text = d_ref_text;
  a.ref_offs = d_ref_offs;
  a.n_ref = ix->n_strings;
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
  HIP_TRY(hipMemsetAsync(words, 0, 128, st));
  launch_pile_seed_count(a, st);
  launch_scan(a.seed_cnt, n, (u64*)(base + w.partial), a.seed_start, a.seed_total, st);
  launch_pile_seed_fill(a, st);
  HIP_TRY(hipGetLastError());
  // the seeds through the locate kernels: both strands, at most H hits a seed, walks as long as a reference read may be
  const int rc = sigax_locate_device(ix, a.seed_bytes, a.seed_offs, w.seed_cap, SIGAX_RC, p.max_seed_hits, PILE_REF_MAX_LEN, base + w.totals,
                                     base + w.qflags, base + w.hit_offs, base + w.hits, nullptr, hits_cap, words + 4, base + w.loc_work,
                                     w.loc_work_bytes, st);
  if (rc != SIGAX_OK) return rc;
  const int e = launch_pile(a, st);
  if (e != (int)hipSuccess)
    return sigax_fail(SIGAX_E_DEVICE, "the pile-up kernel's %u bytes of LDS: %s", pile_lds_bytes(a.len_cap, a.tab_cap), hipGetErrorString((hipError_t)e));
  launch_pile_status(a, st);
  HIP_TRY(hipGetLastError());
  return SIGAX_OK;
}

}  // namespace

struct sigax_pile_ref {
  int device;
  u64 n_strings, text_bytes;
  unsigned char* d_text;
  u64* d_offs;
};

extern "C" int sigax_reference_text_workspace(sigax_index* ix, uint64_t* text_bytes, uint64_t* work_bytes) {
  if (!ix || !text_bytes || !work_bytes) return sigax_fail(SIGAX_E_ARG, "bad argument");
  const int rc = pile_usable(ix);
  if (rc != SIGAX_OK) return rc;
  *text_bytes = ix->n_symbols - ix->n_strings;
  *work_bytes = ref_work(ix->n_strings).bytes;
  return SIGAX_OK;
}

extern "C" int sigax_reference_text_device(sigax_index* ix, void* d_text, uint64_t text_bytes, void* d_text_offs, void* d_status4, void* d_work,
                                           uint64_t work_bytes, void* stream) {
  if (!ix) return sigax_fail(SIGAX_E_ARG, "bad argument");
  const int rc = pile_usable(ix);
  if (rc != SIGAX_OK) return rc;
  if (!d_text || !d_text_offs || !d_status4 || !d_work) return sigax_fail(SIGAX_E_ARG, "NULL where a buffer is required");
  if (((uintptr_t)d_work & 15) || ((uintptr_t)d_text_offs & 7) || ((uintptr_t)d_status4 & 7))
    return sigax_fail(SIGAX_E_ARG, "d_work must be 16-byte aligned, d_text_offs and d_status4 8-byte aligned");
  if (text_bytes < ix->n_symbols - ix->n_strings)
    return sigax_fail(SIGAX_E_ARG, "text_bytes %llu, %llu needed (sigax_reference_text_workspace)", (u64)text_bytes, ix->n_symbols - ix->n_strings);
  if (work_bytes < ref_work(ix->n_strings).bytes)
    return sigax_fail(SIGAX_E_ARG, "workspace of %llu bytes, %llu needed (sigax_reference_text_workspace)", (u64)work_bytes, ref_work(ix->n_strings).bytes);
  HIP_TRY(hipSetDevice(ix->device));
  return ref_text_enqueue(ix, (unsigned char*)d_text, (u64*)d_text_offs, (u64*)d_status4, d_work, (hipStream_t)stream);
}

extern "C" int sigax_pileup_workspace(uint64_t n_reads, uint64_t n_bases, const sigax_pile_params* params, uint64_t hits_cap, uint64_t* bytes) {
  if (!bytes) return sigax_fail(SIGAX_E_ARG, "bad argument");
  const int rc = check_params(params);
  if (rc != SIGAX_OK) return rc;
  PileWork w;
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
  PileWork w;
  const sigax_pile_params p = with_len(*params);
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

extern "C" int sigax_pile_ref_create(sigax_index* ix, sigax_pile_ref** out) {
  if (!ix || !out) return sigax_fail(SIGAX_E_ARG, "bad argument");
  *out = nullptr;
  const int ru = pile_usable(ix);
  if (ru != SIGAX_OK) return ru;
  HIP_TRY(hipSetDevice(ix->device));
  const u64 n = ix->n_strings, tb = ix->n_symbols - ix->n_strings;
  DevGuard g, keep;
  unsigned char* d_text = nullptr;
  u64 *d_offs = nullptr, *d_status = nullptr;
  void* d_work = nullptr;
  HIP_TRY(keep.alloc((void**)&d_text, (size_t)tb + 16));
  HIP_TRY(keep.alloc((void**)&d_offs, ((size_t)n + 1) * 8));
  HIP_TRY(g.alloc((void**)&d_status, 32));
  HIP_TRY(g.alloc(&d_work, (size_t)ref_work(n).bytes));
  const int rc = ref_text_enqueue(ix, d_text, d_offs, d_status, d_work, (hipStream_t)0);
  if (rc != SIGAX_OK) return rc;
  u64 status[4];
  HIP_TRY(hipMemcpy(status, d_status, 32, hipMemcpyDeviceToHost));
  if (status[2] || status[3] || status[1] != tb)
    return sigax_fail(SIGAX_E_STATE, "the index does not give its reads back: %llu rows without a read, %llu slots of the wrong size, %llu of %llu bases",
                      status[2], status[3], status[1], tb);
  sigax_pile_ref* r = new sigax_pile_ref;
  r->device = ix->device;
  r->n_strings = n;
  r->text_bytes = tb;
  r->d_text = d_text;
  r->d_offs = d_offs;
  keep.ptrs.clear();
  *out = r;
  return SIGAX_OK;
}

extern "C" void sigax_pile_ref_destroy(sigax_pile_ref* r) {
  if (!r) return;
  (void)hipSetDevice(r->device);
  (void)hipFree(r->d_text);
  (void)hipFree(r->d_offs);
  delete r;
}

extern "C" int sigax_pile_ref_buffers(const sigax_pile_ref* r, const void** d_text, const void** d_text_offs, uint64_t* text_bytes) {
  if (!r) return sigax_fail(SIGAX_E_ARG, "bad argument");
  if (d_text) *d_text = r->d_text;
  if (d_text_offs) *d_text_offs = r->d_offs;
  if (text_bytes) *text_bytes = r->text_bytes;
  return SIGAX_OK;
}

namespace {

// test hooks, read per call: reads a piece holds at most, and the hits the first try of a piece has room for
u64 env_u64(const char* name, u64 dflt) {
  const char* v = getenv(name);
  return v ? strtoull(v, nullptr, 10) : dflt;
}

// One round over m reads in host memory (offsets from 0), in pieces that fit the device: out, valid, changed and the status
// words added to status8.
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
    // the first try: room for 16 hits a base (some 20-fold cover at the default stride), no more than the budget holds
    u64 hits_cap = first_cap != ~0ull ? first_cap : std::min<u64>(std::max<u64>(nb * 16, 4096), budget / 16);
    bool done = false, split = false;
    for (int attempt = 0; attempt < 2 && !done && !split; ++attempt) {
      PileWork w;
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
      if (status[0] > hits_cap) {  // nothing was written: size the hits from what the seeds list, or take fewer reads
        if (status[0] > LOCATE_MAX_SLOTS || status[0] * 16 > budget) {
          if (cnt == 1) return sigax_fail(SIGAX_E_CAPACITY, "one read lists %llu hits: they do not fit the device", status[0]);
          split = true;
        } else {
          hits_cap = status[0];
        }
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
  if (p.max_read_len == 0) {  // the LDS of a wave follows the batch's longest read
    u64 longest = 1;
    for (u64 i = 0; i < n_reads; ++i) longest = std::max<u64>(longest, offs[i + 1] - offs[i]);
    p.max_read_len = (uint32_t)std::min<u64>(longest, SIGAX_PILE_MAX_LEN);
  }
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
