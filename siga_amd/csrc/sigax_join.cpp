// siga_amd/csrc/sigax_join.cpp -- `siga unitig --scaffold --join-overlaps [--join-mismatches]` on the device: the entry points of
// sigax_join.hip.  sigax_join_* are the max_mismatches = 0 case of sigax_join_approx_*: one set of checks, one launch sequence.
#include <cstring>

#include "sigax_internal.h"

static_assert(sizeof(sigax_join_opts) == 28, "sigax_join_opts must be 28 bytes");
static_assert(sizeof(sigax_join) == 32, "sigax_join must be 32 bytes");
static_assert(sizeof(sigax_join_approx_opts) == 36, "sigax_join_approx_opts must be 36 bytes");

namespace {

// where the pieces of the caller's scratch lie (every piece 16-byte aligned)
struct JoinWork {
  u64 cnt, u32s[7], scans[5], partial, scan_total, gres, plen, psrc, pkey, pshift, acnt, cols, ainfo, amask, bytes;
};
// approx: the pieces of `--join-mismatches` behind the others, which lie where they lie without it
JoinWork join_work(u64 n, bool approx) {
  JoinWork w;
  u64 at = 0;
  auto take = [&](u64 bytes) {
    const u64 here = at;
    at += (bytes + 15) & ~15ull;
    return here;
  };
  w.cnt = take((u64)JOIN_WORDS * 8);
  for (int k = 0; k < 7; ++k) w.u32s[k] = take(n * 4);
  for (int k = 0; k < 5; ++k) w.scans[k] = take((n + 1) * 8);
  w.partial = take(scan_partials_needed(n) * 8);
  w.scan_total = take(8);
  w.gres = take(n * 16);
  w.plen = take(n * 8);
  w.psrc = take(n * 8);
  w.pkey = take((n + 1) * 8);
  w.pshift = take(n * 8);
  w.acnt = w.cols = w.ainfo = w.amask = 0;
  if (approx) {
    w.acnt = take((u64)JOIN_AWORDS * 8);
    w.cols = take(n * JOIN_MAX_COLUMNS * 2);
    w.ainfo = take(n * 4);
    w.amask = take(n * 4);
  }
  w.bytes = at;
  return w;
}

int join_limits(u64 max_unitigs) {
  if (max_unitigs >= (1ull << 31)) return sigax_fail(SIGAX_E_ARG, "max_unitigs: 2^31 unitigs or more");
  return SIGAX_OK;
}

// the options of either entry point; approx: through sigax_join_approx_* (24 status entries, mm, the wider workspace)
struct JoinOpts {
  uint32_t flags, min_overlap, max_overlap, slack, k, min_count, max_mismatches, mismatch_permille, reserved;
  bool approx;
};
bool join_opts_of(const sigax_join_opts* o, JoinOpts* out) {
  if (o) *out = JoinOpts{o->flags, o->min_overlap, o->max_overlap, o->slack, o->k, o->min_count, 0, 0, o->reserved, false};
  return o != nullptr;
}
bool join_opts_of(const sigax_join_approx_opts* o, JoinOpts* out) {
  if (o) *out = JoinOpts{o->flags, o->min_overlap, o->max_overlap, o->slack, o->k, o->min_count, o->max_mismatches, o->mismatch_permille, o->reserved, true};
  return o != nullptr;
}

int join_opts_ok(bool given, const JoinOpts* o) {
  if (!given) return sigax_fail(SIGAX_E_ARG, "NULL where the join options are required");
  if (o->flags != 0 || o->reserved != 0)
    return sigax_fail(SIGAX_E_ARG, o->approx ? "sigax_join_approx_opts.flags and .reserved must be 0" : "sigax_join_opts.flags and .reserved must be 0");
  if (o->approx && o->max_mismatches > JOIN_MAX_COLUMNS) return sigax_fail(SIGAX_E_ARG, "max_mismatches %u: 0 .. 16", o->max_mismatches);
  if (o->approx && (o->mismatch_permille < 1 || o->mismatch_permille > 250))
    return sigax_fail(SIGAX_E_ARG, "mismatch_permille %u: 1 .. 250", o->mismatch_permille);
  if (o->min_overlap < 8 || o->min_overlap > 4096) return sigax_fail(SIGAX_E_ARG, "min_overlap %u: 8 .. 4096", o->min_overlap);
  if (o->max_overlap < o->min_overlap || o->max_overlap > 4096)
    return sigax_fail(SIGAX_E_ARG, "max_overlap %u: min_overlap %u .. 4096", o->max_overlap, o->min_overlap);
  if (o->slack >= (1u << 31)) return sigax_fail(SIGAX_E_ARG, "slack %u: below 2^31", o->slack);
  if (o->k < 8 || o->k > 128) return sigax_fail(SIGAX_E_ARG, "k %u: 8 .. 128", o->k);
  if (o->min_count < 1) return sigax_fail(SIGAX_E_ARG, "min_count %u: at least 1", o->min_count);
  return SIGAX_OK;
}

bool overlap(const void* a, u64 a_bytes, const void* b, u64 b_bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return a && b && a_bytes && b_bytes && x < y + b_bytes && y < x + a_bytes;
}

// every check of the device form; *a is filled when there is something to launch
int join_args(sigax_index* ix, const void* d_n_unitigs, uint64_t max_unitigs, const void* d_seq_offs, const void* d_n_scaffolds, const void* d_sc_offs,
              const void* d_sc_lay_offs, const sigax_placement* d_sc_layout, const void* d_sseqs, uint64_t sseqs_bytes, bool opts_given,
              const JoinOpts* opts, void* d_sc_offs_out, sigax_placement* d_sc_layout_out, void* d_sseqs_out, uint64_t sseqs_capacity,
              sigax_join* d_joins, uint32_t* d_mm, void* d_status16, void* d_work, uint64_t work_bytes, JoinArgs* a) {
  if (!ix) return sigax_fail(SIGAX_E_ARG, "NULL where the index is required");
  const int rl = join_limits(max_unitigs);
  if (rl != SIGAX_OK) return rl;
  const int ro = join_opts_ok(opts_given, opts);
  if (ro != SIGAX_OK) return ro;
  const bool approx = opts->approx;
  const char* status_name = approx ? "d_status24" : "d_status16";
  if (!d_status16) return sigax_fail(SIGAX_E_ARG, "%s: NULL where a buffer is required", status_name);
  if ((uintptr_t)d_status16 & 7) return sigax_fail(SIGAX_E_ARG, "%s must be 8-byte aligned", status_name);
  if ((uintptr_t)d_mm & 3) return sigax_fail(SIGAX_E_ARG, "d_mm must be 4-byte aligned");
  if (!d_sseqs_out && sseqs_capacity) return sigax_fail(SIGAX_E_ARG, "d_sseqs_out: NULL with a capacity of %llu bytes", (u64)sseqs_capacity);
  if (sseqs_capacity >= (1ull << 43)) return sigax_fail(SIGAX_E_ARG, "sseqs_capacity: 2^43 bytes or more");
  if (sseqs_bytes >= (1ull << 43)) return sigax_fail(SIGAX_E_ARG, "sseqs_bytes: 2^43 bytes or more");
  if ((uintptr_t)d_sseqs_out & 15) return sigax_fail(SIGAX_E_ARG, "d_sseqs_out must be 16-byte aligned");
  if (!d_sseqs && sseqs_bytes) return sigax_fail(SIGAX_E_ARG, "d_sseqs: NULL with %llu bytes", (u64)sseqs_bytes);
  if ((uintptr_t)d_sseqs & 15) return sigax_fail(SIGAX_E_ARG, "d_sseqs must be 16-byte aligned");
  if (max_unitigs == 0) return SIGAX_OK;
  const struct { const void* p; const char* name; unsigned align; } bufs[] = {
      {d_n_unitigs, "d_n_unitigs", 8}, {d_seq_offs, "d_seq_offs", 8}, {d_n_scaffolds, "d_n_scaffolds", 8}, {d_sc_offs, "d_sc_offs", 8},
      {d_sc_lay_offs, "d_sc_lay_offs", 8}, {d_sc_layout, "d_sc_layout", 16}, {d_sc_offs_out, "d_sc_offs_out", 8},
      {d_sc_layout_out, "d_sc_layout_out", 16}, {d_joins, "d_joins", 16}, {d_work, "d_work", 16}};
  for (const auto& b : bufs) {
    if (!b.p) return sigax_fail(SIGAX_E_ARG, "%s: NULL where a buffer is required", b.name);
    if ((uintptr_t)b.p & (b.align - 1)) return sigax_fail(SIGAX_E_ARG, "%s must be %u-byte aligned", b.name, b.align);
  }
  if (approx && !d_mm) return sigax_fail(SIGAX_E_ARG, "d_mm: NULL where a buffer is required");
  if (overlap(d_sc_layout, max_unitigs * sizeof(sigax_placement), d_sc_layout_out, max_unitigs * sizeof(sigax_placement)))
    return sigax_fail(SIGAX_E_ARG, "d_sc_layout_out overlaps d_sc_layout");
  if (overlap(d_sc_offs, (max_unitigs + 1) * 8, d_sc_offs_out, (max_unitigs + 1) * 8)) return sigax_fail(SIGAX_E_ARG, "d_sc_offs_out overlaps d_sc_offs");
  if (overlap(d_sseqs, sseqs_bytes, d_sseqs_out, sseqs_capacity)) return sigax_fail(SIGAX_E_ARG, "d_sseqs_out overlaps d_sseqs");
  const JoinWork w = join_work(max_unitigs, approx);
  if (work_bytes < w.bytes)
    return sigax_fail(SIGAX_E_ARG, "workspace of %llu bytes, %llu needed (%s)", (u64)work_bytes, w.bytes,
                      approx ? "sigax_join_approx_workspace" : "sigax_join_workspace");
  char* base = (char*)d_work;
  a->fwd = ix->st[0];
  a->n_unitigs = (const u64*)d_n_unitigs;
  a->n_scaffolds = (const u64*)d_n_scaffolds;
  a->max_unitigs = max_unitigs;
  a->seq_offs = (const u64*)d_seq_offs;
  a->sc_offs_in = (const u64*)d_sc_offs;
  a->sc_lay_offs = (const u64*)d_sc_lay_offs;
  a->sc_layout = d_sc_layout;
  a->sseqs_in = (const unsigned char*)d_sseqs;
  a->sseqs_bytes = d_sseqs ? sseqs_bytes : 0;
  a->min_overlap = opts->min_overlap;
  a->max_overlap = opts->max_overlap;
  a->slack = opts->slack;
  a->k = opts->k;
  a->min_count = opts->min_count;
  a->sc_offs = (u64*)d_sc_offs_out;
  a->sc_layout_out = d_sc_layout_out;
  a->sseqs = (unsigned char*)d_sseqs_out;
  a->sseqs_capacity = d_sseqs_out ? sseqs_capacity : 0;
  a->joins = d_joins;
  a->status = (u64*)d_status16;
  a->cnt = (u64*)(base + w.cnt);
  uint32_t** u32s[7] = {&a->sof, &a->isgap, &a->open, &a->rem, &a->lenlo, &a->lenhi, &a->list};
  for (int k = 0; k < 7; ++k) *u32s[k] = (uint32_t*)(base + w.u32s[k]);
  u64** scans[5] = {&a->gnum, &a->onum, &a->esum, &a->slo, &a->shi};
  for (int k = 0; k < 5; ++k) *scans[k] = (u64*)(base + w.scans[k]);
  a->partial = (u64*)(base + w.partial);
  a->scan_total = (u64*)(base + w.scan_total);
  a->gres = (uint4*)(base + w.gres);
  a->plen = (u64*)(base + w.plen);
  a->psrc = (u64*)(base + w.psrc);
  a->pkey = (u64*)(base + w.pkey);
  a->pshift = (u64*)(base + w.pshift);
  // max_mismatches = 0 is the exact call: its kernels, no piece of the second match
  const bool second = approx && opts->max_mismatches > 0;
  a->max_mismatches = second ? opts->max_mismatches : 0;
  a->mismatch_permille = second ? opts->mismatch_permille : 0;
  a->n_status = approx ? 24 : 16;
  a->mm = approx ? d_mm : nullptr;
  a->acnt = second ? (u64*)(base + w.acnt) : nullptr;
  a->cols = second ? (uint16_t*)(base + w.cols) : nullptr;
  a->ainfo = second ? (uint32_t*)(base + w.ainfo) : nullptr;
  a->amask = second ? (uint32_t*)(base + w.amask) : nullptr;
  return SIGAX_OK;
}

int join_workspace(uint64_t max_unitigs, uint64_t* bytes, bool approx) {
  if (!bytes) return sigax_fail(SIGAX_E_ARG, "bytes: NULL where a result is required");
  const int rc = join_limits(max_unitigs);
  if (rc != SIGAX_OK) return rc;
  *bytes = max_unitigs ? join_work(max_unitigs, approx).bytes : 0;
  return SIGAX_OK;
}

int join_device(sigax_index* ix, const void* d_n_unitigs, uint64_t max_unitigs, const void* d_seq_offs, const void* d_n_scaffolds, const void* d_sc_offs,
                const void* d_sc_lay_offs, const sigax_placement* d_sc_layout, const void* d_sseqs, uint64_t sseqs_bytes, bool opts_given,
                const JoinOpts* opts, void* d_sc_offs_out, sigax_placement* d_sc_layout_out, void* d_sseqs_out, uint64_t sseqs_capacity,
                sigax_join* d_joins, uint32_t* d_mm, void* d_status, void* d_work, uint64_t work_bytes, void* stream) {
  JoinArgs a;
  const int rc = join_args(ix, d_n_unitigs, max_unitigs, d_seq_offs, d_n_scaffolds, d_sc_offs, d_sc_lay_offs, d_sc_layout, d_sseqs, sseqs_bytes, opts_given,
                           opts, d_sc_offs_out, d_sc_layout_out, d_sseqs_out, sseqs_capacity, d_joins, d_mm, d_status, d_work, work_bytes, &a);
  if (rc != SIGAX_OK) return rc;
  HIP_TRY(hipSetDevice(ix->device));
  const hipStream_t st = (hipStream_t)stream;
  if (max_unitigs == 0) {
    HIP_TRY(hipMemsetAsync(d_status, 0, (opts->approx ? 24 : 16) * 8, st));
    if (d_sc_offs_out) HIP_TRY(hipMemsetAsync(d_sc_offs_out, 0, 8, st));  // no scaffolds: the table's one entry, where it is given
    return SIGAX_OK;
  }
  HIP_TRY(launch_join(a, ix->wide, ix->n_cu, st));
  return SIGAX_OK;
}

// mm: NULL through sigax_join_host; n_status 16 or 24
int join_host(sigax_index* ix, uint64_t n_unitigs, const uint64_t* seq_offs, uint64_t n_scaffolds, const uint64_t* sc_offs, const uint64_t* sc_lay_offs,
              const sigax_placement* sc_layout, const char* sseqs, bool opts_given, const JoinOpts* opts, uint64_t** sc_offs_out,
              sigax_placement** sc_layout_out, char** sseqs_out, sigax_join** joins, uint64_t* n_joins, uint32_t** mm, uint64_t* status_out, int n_status) {
  if (!sc_offs_out || !sc_layout_out || !joins || !n_joins || !status_out || (n_status == 24 && !mm))
    return sigax_fail(SIGAX_E_ARG, "NULL where a result is required");
  *sc_offs_out = nullptr;
  *sc_layout_out = nullptr;
  *joins = nullptr;
  *n_joins = 0;
  if (mm) *mm = nullptr;
  if (sseqs_out) *sseqs_out = nullptr;
  for (int k = 0; k < n_status; ++k) status_out[k] = 0;
  if (!ix) return sigax_fail(SIGAX_E_ARG, "NULL where the index is required");
  const int ro = join_opts_ok(opts_given, opts);
  if (ro != SIGAX_OK) return ro;
  const u64 n = n_unitigs, S = n_scaffolds;
  if (n >= (1ull << 31)) return sigax_fail(SIGAX_E_ARG, "n_unitigs: 2^31 unitigs or more");
  if (n && (!seq_offs || !sc_offs || !sc_lay_offs)) return sigax_fail(SIGAX_E_ARG, "seq_offs, sc_offs, sc_lay_offs: NULL where a buffer is required");
  if (S > n) return sigax_fail(SIGAX_E_ARG, "n_scaffolds %llu above n_unitigs %llu", S, n);
  const u64 P = n && S ? sc_lay_offs[S] : 0;
  if (P > n) return sigax_fail(SIGAX_E_ARG, "sc_lay_offs[n_scaffolds] %llu above n_unitigs %llu", P, n);
  if (P && !sc_layout) return sigax_fail(SIGAX_E_ARG, "sc_layout: NULL where a buffer is required");
  const u64 sbytes = n ? sc_offs[S] : 0;
  if (sbytes && !sseqs) return sigax_fail(SIGAX_E_ARG, "sseqs: NULL where a buffer is required");
  if (sbytes >= (1ull << 43)) return sigax_fail(SIGAX_E_ARG, "sc_offs[n_scaffolds]: 2^43 bytes or more");
  HostGuard hg;
  u64 status[24];
  memset(status, 0, sizeof status);
  uint64_t* h_so = nullptr;
  sigax_placement* h_lay = nullptr;
  sigax_join* h_joins = nullptr;
  uint32_t* h_mm = nullptr;
  char* h_seqs = nullptr;
  if (n) {
    HIP_TRY(hipSetDevice(ix->device));
    const JoinWork w = join_work(n, opts->approx);
    DevGuard g;
    void *d_cnt, *d_so, *d_sin, *d_sco, *d_slo, *d_lay, *d_scoo, *d_layo, *d_joins, *d_mm = nullptr, *d_st, *d_work, *d_out = nullptr;
    HIP_TRY(g.alloc(&d_cnt, 16));  // {n_unitigs, n_scaffolds}
    HIP_TRY(g.alloc(&d_so, ((size_t)n + 1) * 8));
    HIP_TRY(g.alloc(&d_sin, (size_t)sbytes));
    HIP_TRY(g.alloc(&d_sco, ((size_t)n + 1) * 8));
    HIP_TRY(g.alloc(&d_slo, ((size_t)n + 1) * 8));
    HIP_TRY(g.alloc(&d_lay, (size_t)n * sizeof(sigax_placement)));
    HIP_TRY(g.alloc(&d_scoo, ((size_t)n + 1) * 8));
    HIP_TRY(g.alloc(&d_layo, (size_t)n * sizeof(sigax_placement)));
    HIP_TRY(g.alloc(&d_joins, (size_t)n * sizeof(sigax_join)));
    if (mm) HIP_TRY(g.alloc(&d_mm, (size_t)n * 4));
    HIP_TRY(g.alloc(&d_st, 24 * 8));
    HIP_TRY(g.alloc(&d_work, (size_t)w.bytes));
    const u64 counts[2] = {n, S};
    HIP_TRY(hipMemcpy(d_cnt, counts, 16, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_so, seq_offs, ((size_t)n + 1) * 8, hipMemcpyHostToDevice));
    if (sbytes) HIP_TRY(hipMemcpy(d_sin, sseqs, (size_t)sbytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(d_sco, 0, ((size_t)n + 1) * 8));
    HIP_TRY(hipMemcpy(d_sco, sc_offs, ((size_t)S + 1) * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(d_slo, 0, ((size_t)n + 1) * 8));
    HIP_TRY(hipMemcpy(d_slo, sc_lay_offs, ((size_t)S + 1) * 8, hipMemcpyHostToDevice));
    if (P) HIP_TRY(hipMemcpy(d_lay, sc_layout, (size_t)P * sizeof(sigax_placement), hipMemcpyHostToDevice));
    // the tables, then the bases into a buffer of exactly their size
    JoinArgs a;
    int rc = join_args(ix, d_cnt, n, d_so, (u64*)d_cnt + 1, d_sco, d_slo, (const sigax_placement*)d_lay, d_sin, sbytes, opts_given, opts, d_scoo,
                       (sigax_placement*)d_layo, nullptr, 0, (sigax_join*)d_joins, (uint32_t*)d_mm, d_st, d_work, w.bytes, &a);
    if (rc != SIGAX_OK) return rc;
    HIP_TRY(launch_join(a, ix->wide, ix->n_cu, nullptr));
    HIP_TRY(hipMemcpy(status, d_st, (size_t)n_status * 8, hipMemcpyDeviceToHost));  // (waits for the null stream's kernels)
    const u64 ng = status[0], total = status[11];
    if (ng > n) return sigax_fail(SIGAX_E_DEVICE, "joins beyond their buffer");
    status[14] = 0;
    h_so = hg.alloc<uint64_t>(((size_t)S + 1) * 8);
    h_lay = hg.alloc<sigax_placement>((size_t)P * sizeof(sigax_placement));
    h_joins = hg.alloc<sigax_join>((size_t)ng * sizeof(sigax_join));
    if (mm) h_mm = hg.alloc<uint32_t>((size_t)ng * 4);
    if (sseqs_out) h_seqs = hg.alloc<char>((size_t)total);
    if (!hg.ok) return sigax_fail(SIGAX_E_CAPACITY, "out of host memory");
    HIP_TRY(hipMemcpy(h_so, d_scoo, ((size_t)S + 1) * 8, hipMemcpyDeviceToHost));
    if (P) HIP_TRY(hipMemcpy(h_lay, d_layo, (size_t)P * sizeof(sigax_placement), hipMemcpyDeviceToHost));
    if (ng) HIP_TRY(hipMemcpy(h_joins, d_joins, (size_t)ng * sizeof(sigax_join), hipMemcpyDeviceToHost));
    if (mm && ng) HIP_TRY(hipMemcpy(h_mm, d_mm, (size_t)ng * 4, hipMemcpyDeviceToHost));
    if (sseqs_out && total) {
      if (total >= (1ull << 43)) return sigax_fail(SIGAX_E_ARG, "scaffold bases: 2^43 bytes or more");
      HIP_TRY(g.alloc(&d_out, (size_t)total));
      a.sseqs = (unsigned char*)d_out;
      a.sseqs_capacity = total;
      launch_join_bases(a, nullptr);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpy(h_seqs, d_out, (size_t)total, hipMemcpyDeviceToHost));
    }
    *n_joins = ng;
  } else {
    h_so = hg.alloc<uint64_t>(8);
    h_lay = hg.alloc<sigax_placement>(0);
    h_joins = hg.alloc<sigax_join>(0);
    if (mm) h_mm = hg.alloc<uint32_t>(0);
    if (sseqs_out) h_seqs = hg.alloc<char>(0);
    if (!hg.ok) return sigax_fail(SIGAX_E_CAPACITY, "out of host memory");
    h_so[0] = 0;
  }
  for (int k = 0; k < n_status; ++k) status_out[k] = status[k];
  *sc_offs_out = h_so;
  *sc_layout_out = h_lay;
  *joins = h_joins;
  if (mm) *mm = h_mm;
  if (sseqs_out) *sseqs_out = h_seqs;
  hg.release();
  return SIGAX_OK;
}

}  // namespace

extern "C" int sigax_join_workspace(uint64_t max_unitigs, uint64_t* bytes) { return join_workspace(max_unitigs, bytes, false); }
extern "C" int sigax_join_approx_workspace(uint64_t max_unitigs, uint64_t* bytes) { return join_workspace(max_unitigs, bytes, true); }

extern "C" int sigax_join_device(sigax_index* ix, const void* d_n_unitigs, uint64_t max_unitigs, const void* d_seq_offs, const void* d_n_scaffolds,
                                 const void* d_sc_offs, const void* d_sc_lay_offs, const sigax_placement* d_sc_layout, const void* d_sseqs,
                                 uint64_t sseqs_bytes, const sigax_join_opts* opts, void* d_sc_offs_out, sigax_placement* d_sc_layout_out,
                                 void* d_sseqs_out, uint64_t sseqs_capacity, sigax_join* d_joins, void* d_status16, void* d_work, uint64_t work_bytes,
                                 void* stream) {
  JoinOpts o{};
  const bool given = join_opts_of(opts, &o);
  return join_device(ix, d_n_unitigs, max_unitigs, d_seq_offs, d_n_scaffolds, d_sc_offs, d_sc_lay_offs, d_sc_layout, d_sseqs, sseqs_bytes, given, &o,
                     d_sc_offs_out, d_sc_layout_out, d_sseqs_out, sseqs_capacity, d_joins, nullptr, d_status16, d_work, work_bytes, stream);
}

extern "C" int sigax_join_approx_device(sigax_index* ix, const void* d_n_unitigs, uint64_t max_unitigs, const void* d_seq_offs, const void* d_n_scaffolds,
                                        const void* d_sc_offs, const void* d_sc_lay_offs, const sigax_placement* d_sc_layout, const void* d_sseqs,
                                        uint64_t sseqs_bytes, const sigax_join_approx_opts* opts, void* d_sc_offs_out,
                                        sigax_placement* d_sc_layout_out, void* d_sseqs_out, uint64_t sseqs_capacity, sigax_join* d_joins, uint32_t* d_mm,
                                        void* d_status24, void* d_work, uint64_t work_bytes, void* stream) {
  JoinOpts o{};
  const bool given = join_opts_of(opts, &o);
  return join_device(ix, d_n_unitigs, max_unitigs, d_seq_offs, d_n_scaffolds, d_sc_offs, d_sc_lay_offs, d_sc_layout, d_sseqs, sseqs_bytes, given, &o,
                     d_sc_offs_out, d_sc_layout_out, d_sseqs_out, sseqs_capacity, d_joins, d_mm, d_status24, d_work, work_bytes, stream);
}

extern "C" int sigax_join_host(sigax_index* ix, uint64_t n_unitigs, const uint64_t* seq_offs, uint64_t n_scaffolds, const uint64_t* sc_offs,
                               const uint64_t* sc_lay_offs, const sigax_placement* sc_layout, const char* sseqs, const sigax_join_opts* opts,
                               uint64_t** sc_offs_out, sigax_placement** sc_layout_out, char** sseqs_out, sigax_join** joins, uint64_t* n_joins,
                               uint64_t status16[16]) {
  JoinOpts o{};
  const bool given = join_opts_of(opts, &o);
  return join_host(ix, n_unitigs, seq_offs, n_scaffolds, sc_offs, sc_lay_offs, sc_layout, sseqs, given, &o, sc_offs_out, sc_layout_out, sseqs_out, joins,
                   n_joins, nullptr, status16, 16);
}

extern "C" int sigax_join_approx_host(sigax_index* ix, uint64_t n_unitigs, const uint64_t* seq_offs, uint64_t n_scaffolds, const uint64_t* sc_offs,
                                      const uint64_t* sc_lay_offs, const sigax_placement* sc_layout, const char* sseqs,
                                      const sigax_join_approx_opts* opts, uint64_t** sc_offs_out, sigax_placement** sc_layout_out, char** sseqs_out,
                                      sigax_join** joins, uint64_t* n_joins, uint32_t** mm, uint64_t status24[24]) {
  JoinOpts o{};
  const bool given = join_opts_of(opts, &o);
  return join_host(ix, n_unitigs, seq_offs, n_scaffolds, sc_offs, sc_lay_offs, sc_layout, sseqs, given, &o, sc_offs_out, sc_layout_out, sseqs_out, joins,
                   n_joins, mm, status24, 24);
}
