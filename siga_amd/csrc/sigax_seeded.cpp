// siga_amd/csrc/sigax_seeded.cpp -- the host side of the seeding stage (sigax_seeded.h): the reference text's entry points, the
// workspace layout and the enqueue of seeds and hits, and what the callers' checks and batch loops have in common.
#include <cstring>

#include "sigax_internal.h"
#include "sigax_seeded.h"

u64 up16(u64 v) { return (v + 15) & ~15ull; }

u64 env_u64(const char* name, u64 dflt) {
  const char* v = getenv(name);
  return v ? strtoull(v, nullptr, 10) : dflt;
}

int seeded_usable(const sigax_index* ix, const char* needs, const char* cannot) {
  if (!ix->d_sai[0] || ix->n_sai != ix->n_strings)
    return sigax_fail(SIGAX_E_STATE, "the index was opened without its forward .sai table: %s it to name the reads", needs);
  if (ix->st[0].C[1] != ix->n_strings)
    return sigax_fail(SIGAX_E_STATE, "reads with non-ACGT bases in the index: stretches are not reads, %s them", cannot);
  return SIGAX_OK;
}

int seeded_check_params(uint32_t seed_length, uint32_t seed_stride, uint32_t max_seed_hits, uint32_t min_overlap, uint32_t error_permille,
                        uint32_t max_candidates, uint32_t max_read_len, uint32_t reserved) {
  if (seed_length < 12 || seed_length > 64) return sigax_fail(SIGAX_E_ARG, "seed_length %u: 12..64", seed_length);
  if (seed_stride < 1 || seed_stride > seed_length) return sigax_fail(SIGAX_E_ARG, "seed_stride %u: 1..seed_length", seed_stride);
  if (max_seed_hits < 1 || max_seed_hits > 4096) return sigax_fail(SIGAX_E_ARG, "max_seed_hits %u: 1..4096", max_seed_hits);
  if (min_overlap < 1) return sigax_fail(SIGAX_E_ARG, "min_overlap 0: from 1");
  if (error_permille > 250) return sigax_fail(SIGAX_E_ARG, "error_permille %u: 0..250", error_permille);
  if (max_candidates < 1 || max_candidates > 4096) return sigax_fail(SIGAX_E_ARG, "max_candidates %u: 1..4096", max_candidates);
  if (max_read_len > SIGAX_PILE_MAX_LEN) return sigax_fail(SIGAX_E_ARG, "max_read_len %u: 0..%u", max_read_len, SIGAX_PILE_MAX_LEN);
  if (reserved != 0) return sigax_fail(SIGAX_E_ARG, "reserved must be 0");
  return SIGAX_OK;
}

uint32_t seeded_max_len(uint32_t max_read_len) { return max_read_len ? max_read_len : SIGAX_PILE_MAX_LEN; }

uint32_t seeded_max_len(uint32_t max_read_len, const u64* offs, u64 n) {
  if (max_read_len) return max_read_len;
  u64 longest = 1;
  for (u64 i = 0; i < n; ++i) longest = std::max<u64>(longest, offs[i + 1] - offs[i]);
  return (uint32_t)std::min<u64>(longest, SIGAX_PILE_MAX_LEN);
}

// room for 16 hits a base (some 20-fold cover at the default stride), no more than the budget holds
u64 seeded_first_hits_cap(u64 test_cap, u64 nb, u64 budget) {
  return test_cap != ~0ull ? test_cap : std::min<u64>(std::max<u64>(nb * 16, 4096), budget / 16);
}

// nothing was written: size the hits from what the seeds list, or take fewer reads
int seeded_hits_overflow(u64 listed, u64 budget, u64 cnt, u64* hits_cap, bool* split) {
  if (listed > LOCATE_MAX_SLOTS || listed * 16 > budget) {
    if (cnt == 1) return sigax_fail(SIGAX_E_CAPACITY, "one read lists %llu hits: they do not fit the device", listed);
    *split = true;
  } else {
    *hits_cap = listed;
  }
  return SIGAX_OK;
}

int seed_work(u64 n, u64 n_bases, uint32_t S, uint32_t T, u64 hits_cap, u64 middle_bytes, SeedWork* out) {
  SeedWork w;
  // a read of n bases has at most n / T + 1 seeds: (n - S) / T + 2 <= n / T + 1 with S >= T
  w.seed_cap = n_bases / T + n;
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
  w.words = at;
  at += 128;
  w.middle = at;
  at += middle_bytes;
  w.seed_bytes = at;
  at += up16(w.seed_cap * S + 16);
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

int seed_enqueue(sigax_index* ix, const unsigned char* d_seqs, const u64* d_offs, u64 n, uint32_t S, uint32_t T, uint32_t max_read_len, uint32_t H,
                 void* d_work, const SeedWork& w, u64 zero_middle, u64 hits_cap, hipStream_t st) {
  char* base = (char*)d_work;
  u64* words = (u64*)(base + w.words);
  SeedArgs s;
  s.seqs = d_seqs;
  s.offs = d_offs;
  s.n_reads = n;
  s.S = S;
  s.T = T;
  s.max_read_len = max_read_len;
  s.seed_cnt = (uint32_t*)(base + w.seed_cnt);
  s.seed_start = (u64*)(base + w.seed_start);
  s.seed_total = words;
  s.seed_cap = w.seed_cap;
  s.seed_bytes = (unsigned char*)(base + w.seed_bytes);
  s.seed_offs = (u64*)(base + w.seed_offs);
  HIP_TRY(hipMemsetAsync(words, 0, 128, st));
  if (zero_middle) HIP_TRY(hipMemsetAsync(base + w.middle, 0, (size_t)zero_middle, st));
  launch_seed_count(s, st);
  launch_scan(s.seed_cnt, n, (u64*)(base + w.partial), s.seed_start, s.seed_total, st);
  launch_seed_fill(s, st);
  HIP_TRY(hipGetLastError());
  // the seeds through the locate kernels: both strands, at most H hits a seed, walks as long as a reference read may be
  return sigax_locate_device(ix, s.seed_bytes, s.seed_offs, w.seed_cap, SIGAX_RC, H, SEED_REF_MAX_LEN, base + w.totals, base + w.qflags,
                             base + w.hit_offs, base + w.hits, nullptr, hits_cap, words + 4, base + w.loc_work, w.loc_work_bytes, st);
}

// ---- reference text ----
namespace {

int ref_usable(const sigax_index* ix) { return seeded_usable(ix, "the pile-up needs", "no pile can be built from"); }

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
  int rc = sigax_string_lengths_device(ix, 0, rows, n, SEED_REF_MAX_LEN, lens, stretch, words, st);
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
  rc = sigax_get_strings_device(ix, 0, rows_by_id, n, SEED_REF_MAX_LEN, d_offs, d_text, words, st);
  if (rc != SIGAX_OK) return rc;
  // {reads, bases, rows that gave no read, slots of the wrong size}
  HIP_TRY(hipMemcpyAsync(d_status + 0, words + 5, 8, hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_status + 1, words + 3, 8, hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_status + 2, words + 4, 8, hipMemcpyDeviceToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_status + 3, words + 2, 8, hipMemcpyDeviceToDevice, st));
  return SIGAX_OK;
}

}  // namespace

extern "C" int sigax_reference_text_workspace(sigax_index* ix, uint64_t* text_bytes, uint64_t* work_bytes) {
  if (!ix || !text_bytes || !work_bytes) return sigax_fail(SIGAX_E_ARG, "bad argument");
  const int rc = ref_usable(ix);
  if (rc != SIGAX_OK) return rc;
  *text_bytes = ix->n_symbols - ix->n_strings;
  *work_bytes = ref_work(ix->n_strings).bytes;
  return SIGAX_OK;
}

extern "C" int sigax_reference_text_device(sigax_index* ix, void* d_text, uint64_t text_bytes, void* d_text_offs, void* d_status4, void* d_work,
                                           uint64_t work_bytes, void* stream) {
  if (!ix) return sigax_fail(SIGAX_E_ARG, "bad argument");
  const int rc = ref_usable(ix);
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

extern "C" int sigax_pile_ref_create(sigax_index* ix, sigax_pile_ref** out) {
  if (!ix || !out) return sigax_fail(SIGAX_E_ARG, "bad argument");
  *out = nullptr;
  const int ru = ref_usable(ix);
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
