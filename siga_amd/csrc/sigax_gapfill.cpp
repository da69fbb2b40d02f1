// siga_amd/csrc/sigax_gapfill.cpp -- `siga unitig --scaffold --gapfill` on the device: the entry points of sigax_gapfill.hip.
#include <cstring>

#include "sigax_internal.h"

static_assert(sizeof(sigax_gapfill_opts) == 24, "sigax_gapfill_opts must be 24 bytes");
static_assert(sizeof(sigax_gap) == 32, "sigax_gap must be 32 bytes");

namespace {

// where the pieces of the caller's scratch lie (every piece 16-byte aligned)
struct GapWork {
  u64 cnt, sof, u32s[6], scans[6], partial, scan_total, gres, gap_g, win, pdst, psrc, plen, walk, bytes;
};
GapWork gap_work(u64 n, u64 walk_bases) {
  GapWork w;
  u64 at = 0;
  auto take = [&](u64 bytes) {
    const u64 here = at;
    at += (bytes + 15) & ~15ull;
    return here;
  };
  w.cnt = take((u64)GAP_WORDS * 8);
  w.sof = take(n * 4);
  for (int k = 0; k < 6; ++k) w.u32s[k] = take(n * 4);
  for (int k = 0; k < 6; ++k) w.scans[k] = take((n + 1) * 8);
  w.partial = take(scan_partials_needed(n) * 8);
  w.scan_total = take(8);
  w.gres = take(n * 8);
  w.gap_g = take(n * 8);
  w.win = take(n * 128);
  w.pdst = take((n + 1) * 8);
  w.psrc = take(n * 8);
  w.plen = take(n * 8);
  w.walk = take(walk_bases);
  w.bytes = at;
  return w;
}

int gap_limits(u64 max_unitigs, u64 max_walk_bases) {
  if (max_unitigs >= (1ull << 31)) return sigax_fail(SIGAX_E_ARG, "max_unitigs: 2^31 unitigs or more");
  if (max_walk_bases >= (1ull << 43)) return sigax_fail(SIGAX_E_ARG, "max_walk_bases: 2^43 bytes or more");
  return SIGAX_OK;
}

int gap_opts_ok(const sigax_gapfill_opts* o) {
  if (!o) return sigax_fail(SIGAX_E_ARG, "NULL where the gapfill options are required");
  if (o->flags != 0 || o->reserved != 0) return sigax_fail(SIGAX_E_ARG, "sigax_gapfill_opts.flags and .reserved must be 0");
  if (o->k < 8 || o->k > 128) return sigax_fail(SIGAX_E_ARG, "k %u: 8 .. 128", o->k);
  if (o->min_count < 1) return sigax_fail(SIGAX_E_ARG, "min_count %u: at least 1", o->min_count);
  if (o->slack >= (1u << 31)) return sigax_fail(SIGAX_E_ARG, "slack %u: below 2^31", o->slack);
  if (o->max_fill >= (1u << 31)) return sigax_fail(SIGAX_E_ARG, "max_fill %u: below 2^31", o->max_fill);
  return SIGAX_OK;
}

// every check of the device form; *a is filled when there is something to launch
int gap_args(sigax_index* ix, const void* d_n_unitigs, uint64_t max_unitigs, const void* d_seq_offs, const void* d_useqs, uint64_t useqs_bytes,
             const void* d_n_scaffolds, const void* d_sc_lay_offs, const sigax_placement* d_sc_layout, const sigax_gapfill_opts* opts, void* d_sc_offs,
             sigax_placement* d_sc_layout_out, void* d_sseqs, uint64_t sseqs_capacity, sigax_gap* d_gaps, void* d_status24, void* d_work,
             uint64_t work_bytes, uint64_t max_walk_bases, GapfillArgs* a) {
  if (!ix) return sigax_fail(SIGAX_E_ARG, "NULL where the index is required");
  const int rl = gap_limits(max_unitigs, max_walk_bases);
  if (rl != SIGAX_OK) return rl;
  const int ro = gap_opts_ok(opts);
  if (ro != SIGAX_OK) return ro;
  if (!d_status24) return sigax_fail(SIGAX_E_ARG, "d_status24: NULL where a buffer is required");
  if ((uintptr_t)d_status24 & 7) return sigax_fail(SIGAX_E_ARG, "d_status24 must be 8-byte aligned");
  if (!d_sseqs && sseqs_capacity) return sigax_fail(SIGAX_E_ARG, "d_sseqs: NULL with a capacity of %llu bytes", (u64)sseqs_capacity);
  if (sseqs_capacity >= (1ull << 43)) return sigax_fail(SIGAX_E_ARG, "sseqs_capacity: 2^43 bytes or more");
  if ((uintptr_t)d_sseqs & 15) return sigax_fail(SIGAX_E_ARG, "d_sseqs must be 16-byte aligned");
  if (max_unitigs == 0) return SIGAX_OK;
  const struct { const void* p; const char* name; unsigned align; } bufs[] = {
      {d_n_unitigs, "d_n_unitigs", 8}, {d_seq_offs, "d_seq_offs", 8}, {d_useqs, "d_useqs", 16}, {d_n_scaffolds, "d_n_scaffolds", 8},
      {d_sc_lay_offs, "d_sc_lay_offs", 8}, {d_sc_layout, "d_sc_layout", 16}, {d_sc_offs, "d_sc_offs", 8}, {d_sc_layout_out, "d_sc_layout_out", 16},
      {d_gaps, "d_gaps", 16}, {d_work, "d_work", 16}};
  for (const auto& b : bufs) {
    if (!b.p) return sigax_fail(SIGAX_E_ARG, "%s: NULL where a buffer is required", b.name);
    if ((uintptr_t)b.p & (b.align - 1)) return sigax_fail(SIGAX_E_ARG, "%s must be %u-byte aligned", b.name, b.align);
  }
  const uintptr_t li = (uintptr_t)d_sc_layout, lo = (uintptr_t)d_sc_layout_out, lb = (uintptr_t)max_unitigs * sizeof(sigax_placement);
  if (li < lo + lb && lo < li + lb) return sigax_fail(SIGAX_E_ARG, "d_sc_layout_out overlaps d_sc_layout");
  const GapWork w = gap_work(max_unitigs, max_walk_bases);
  if (work_bytes < w.bytes)
    return sigax_fail(SIGAX_E_ARG, "workspace of %llu bytes, %llu needed (sigax_gapfill_workspace)", (u64)work_bytes, w.bytes);
  char* base = (char*)d_work;
  a->fwd = ix->st[0];
  a->n_unitigs = (const u64*)d_n_unitigs;
  a->n_scaffolds = (const u64*)d_n_scaffolds;
  a->max_unitigs = max_unitigs;
  a->seq_offs = (const u64*)d_seq_offs;
  a->useqs = (const unsigned char*)d_useqs;
  a->useqs_bytes = useqs_bytes;
  a->sc_lay_offs = (const u64*)d_sc_lay_offs;
  a->sc_layout = d_sc_layout;
  a->k = opts->k;
  a->min_count = opts->min_count;
  a->slack = opts->slack;
  a->max_fill = opts->max_fill;
  a->sc_offs = (u64*)d_sc_offs;
  a->sc_layout_out = d_sc_layout_out;
  a->sseqs = (unsigned char*)d_sseqs;
  a->sseqs_capacity = d_sseqs ? sseqs_capacity : 0;
  a->gaps = d_gaps;
  a->status = (u64*)d_status24;
  a->cnt = (u64*)(base + w.cnt);
  a->sof = (uint32_t*)(base + w.sof);
  uint32_t** u32s[6] = {&a->isgap, &a->need, &a->fillc, &a->remc, &a->lenlo, &a->lenhi};
  u64** scans[6] = {&a->gnum, &a->soff, &a->fsum, &a->rsum, &a->slo, &a->shi};
  for (int k = 0; k < 6; ++k) {
    *u32s[k] = (uint32_t*)(base + w.u32s[k]);
    *scans[k] = (u64*)(base + w.scans[k]);
  }
  a->partial = (u64*)(base + w.partial);
  a->scan_total = (u64*)(base + w.scan_total);
  a->gres = (uint2*)(base + w.gres);
  a->gap_g = (u64*)(base + w.gap_g);
  a->win = (u64*)(base + w.win);
  a->pdst = (u64*)(base + w.pdst);
  a->psrc = (u64*)(base + w.psrc);
  a->plen = (u64*)(base + w.plen);
  a->walk = (unsigned char*)(base + w.walk);
  a->max_walk_bases = max_walk_bases;
  return SIGAX_OK;
}

}  // namespace

extern "C" int sigax_gapfill_workspace(uint64_t max_unitigs, uint64_t max_walk_bases, uint64_t* bytes) {
  if (!bytes) return sigax_fail(SIGAX_E_ARG, "bytes: NULL where a result is required");
  const int rc = gap_limits(max_unitigs, max_walk_bases);
  if (rc != SIGAX_OK) return rc;
  *bytes = max_unitigs ? gap_work(max_unitigs, max_walk_bases).bytes : 0;
  return SIGAX_OK;
}

extern "C" int sigax_gapfill_device(sigax_index* ix, const void* d_n_unitigs, uint64_t max_unitigs, const void* d_seq_offs, const void* d_useqs,
                                    uint64_t useqs_bytes, const void* d_n_scaffolds, const void* d_sc_lay_offs, const sigax_placement* d_sc_layout,
                                    const sigax_gapfill_opts* opts, void* d_sc_offs, sigax_placement* d_sc_layout_out, void* d_sseqs,
                                    uint64_t sseqs_capacity, sigax_gap* d_gaps, void* d_status24, void* d_work, uint64_t work_bytes,
                                    uint64_t max_walk_bases, void* stream) {
  GapfillArgs a;
  const int rc = gap_args(ix, d_n_unitigs, max_unitigs, d_seq_offs, d_useqs, useqs_bytes, d_n_scaffolds, d_sc_lay_offs, d_sc_layout, opts, d_sc_offs,
                          d_sc_layout_out, d_sseqs, sseqs_capacity, d_gaps, d_status24, d_work, work_bytes, max_walk_bases, &a);
  if (rc != SIGAX_OK) return rc;
  HIP_TRY(hipSetDevice(ix->device));
  const hipStream_t st = (hipStream_t)stream;
  if (max_unitigs == 0) {
    HIP_TRY(hipMemsetAsync(d_status24, 0, 24 * 8, st));
    if (d_sc_offs) HIP_TRY(hipMemsetAsync(d_sc_offs, 0, 8, st));  // no scaffolds: the table's one entry, where it is given
    return SIGAX_OK;
  }
  HIP_TRY(launch_gapfill(a, ix->wide, ix->n_cu, st));
  return SIGAX_OK;
}

extern "C" int sigax_gapfill_host(sigax_index* ix, uint64_t n_unitigs, const uint64_t* seq_offs, const char* useqs, uint64_t n_scaffolds,
                                  const uint64_t* sc_lay_offs, const sigax_placement* sc_layout, const sigax_gapfill_opts* opts,
                                  uint64_t max_walk_bases, uint64_t** sc_offs, sigax_placement** sc_layout_out, char** sseqs, sigax_gap** gaps,
                                  uint64_t* n_gaps, uint64_t status24[24]) {
  if (!sc_offs || !sc_layout_out || !gaps || !n_gaps || !status24) return sigax_fail(SIGAX_E_ARG, "NULL where a result is required");
  *sc_offs = nullptr;
  *sc_layout_out = nullptr;
  *gaps = nullptr;
  *n_gaps = 0;
  if (sseqs) *sseqs = nullptr;
  for (int k = 0; k < 24; ++k) status24[k] = 0;
  if (!ix) return sigax_fail(SIGAX_E_ARG, "NULL where the index is required");
  const int ro = gap_opts_ok(opts);
  if (ro != SIGAX_OK) return ro;
  const u64 n = n_unitigs, S = n_scaffolds;
  if (n >= (1ull << 31)) return sigax_fail(SIGAX_E_ARG, "n_unitigs: 2^31 unitigs or more");
  if (n && (!seq_offs || !sc_lay_offs)) return sigax_fail(SIGAX_E_ARG, "seq_offs, sc_lay_offs: NULL where a buffer is required");
  if (S > n) return sigax_fail(SIGAX_E_ARG, "n_scaffolds %llu above n_unitigs %llu", S, n);
  const u64 P = n && S ? sc_lay_offs[S] : 0;
  if (P > n) return sigax_fail(SIGAX_E_ARG, "sc_lay_offs[n_scaffolds] %llu above n_unitigs %llu", P, n);
  if (P && !sc_layout) return sigax_fail(SIGAX_E_ARG, "sc_layout: NULL where a buffer is required");
  const u64 ubytes = n ? seq_offs[n] : 0;
  if (ubytes && !useqs) return sigax_fail(SIGAX_E_ARG, "useqs: NULL where a buffer is required");
  HostGuard hg;
  u64 status[24];
  memset(status, 0, sizeof status);
  uint64_t* h_so = nullptr;
  sigax_placement* h_lay = nullptr;
  sigax_gap* h_gaps = nullptr;
  char* h_seqs = nullptr;
  if (n) {
    if (max_walk_bases == SIGAX_GAPFILL_AUTO) {
      // no less than the gaps that come to a walk need, G + slack each: every pair of neighbours with G <= max_fill (a sum
      // over fewer than 2^31 terms below 2^32)
      max_walk_bases = 0;
      for (u64 p = 0; p + 1 < P; ++p) {
        const u64 u = sc_layout[p].read;
        const u64 G = sc_layout[p + 1].offset - sc_layout[p].offset - (u < n ? seq_offs[u + 1] - seq_offs[u] : 0ull);
        if (G <= opts->max_fill) max_walk_bases += G + opts->slack;
      }
    }
    const int rl = gap_limits(n, max_walk_bases);
    if (rl != SIGAX_OK) return rl;
    HIP_TRY(hipSetDevice(ix->device));
    const GapWork w = gap_work(n, max_walk_bases);
    DevGuard g;
    void *d_cnt, *d_so, *d_us, *d_slo, *d_lay, *d_sco, *d_layo, *d_gaps, *d_st, *d_work, *d_out = nullptr;
    HIP_TRY(g.alloc(&d_cnt, 16));  // {n_unitigs, n_scaffolds}
    HIP_TRY(g.alloc(&d_so, ((size_t)n + 1) * 8));
    HIP_TRY(g.alloc(&d_us, (size_t)ubytes));
    HIP_TRY(g.alloc(&d_slo, ((size_t)n + 1) * 8));
    HIP_TRY(g.alloc(&d_lay, (size_t)n * sizeof(sigax_placement)));
    HIP_TRY(g.alloc(&d_sco, ((size_t)n + 1) * 8));
    HIP_TRY(g.alloc(&d_layo, (size_t)n * sizeof(sigax_placement)));
    HIP_TRY(g.alloc(&d_gaps, (size_t)n * sizeof(sigax_gap)));
    HIP_TRY(g.alloc(&d_st, 24 * 8));
    HIP_TRY(g.alloc(&d_work, (size_t)w.bytes));
    const u64 counts[2] = {n, S};
    HIP_TRY(hipMemcpy(d_cnt, counts, 16, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_so, seq_offs, ((size_t)n + 1) * 8, hipMemcpyHostToDevice));
    if (ubytes) HIP_TRY(hipMemcpy(d_us, useqs, (size_t)ubytes, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(d_slo, 0, ((size_t)n + 1) * 8));
    HIP_TRY(hipMemcpy(d_slo, sc_lay_offs, ((size_t)S + 1) * 8, hipMemcpyHostToDevice));
    if (P) HIP_TRY(hipMemcpy(d_lay, sc_layout, (size_t)P * sizeof(sigax_placement), hipMemcpyHostToDevice));
    // the walks and the tables, then the bases into a buffer of exactly their size
    GapfillArgs a;
    int rc = gap_args(ix, d_cnt, n, d_so, d_us, ubytes, (u64*)d_cnt + 1, d_slo, (const sigax_placement*)d_lay, opts, d_sco, (sigax_placement*)d_layo,
                      nullptr, 0, (sigax_gap*)d_gaps, d_st, d_work, w.bytes, max_walk_bases, &a);
    if (rc != SIGAX_OK) return rc;
    HIP_TRY(launch_gapfill(a, ix->wide, ix->n_cu, nullptr));
    HIP_TRY(hipMemcpy(status, d_st, 24 * 8, hipMemcpyDeviceToHost));  // (waits for the null stream's kernels)
    const u64 ng = status[0], total = status[16];
    if (ng > n) return sigax_fail(SIGAX_E_DEVICE, "gaps beyond their buffer");
    status[20] = 0;
    h_so = hg.alloc<uint64_t>(((size_t)S + 1) * 8);
    h_lay = hg.alloc<sigax_placement>((size_t)P * sizeof(sigax_placement));
    h_gaps = hg.alloc<sigax_gap>((size_t)ng * sizeof(sigax_gap));
    if (sseqs) h_seqs = hg.alloc<char>((size_t)total);
    if (!hg.ok) return sigax_fail(SIGAX_E_CAPACITY, "out of host memory");
    HIP_TRY(hipMemcpy(h_so, d_sco, ((size_t)S + 1) * 8, hipMemcpyDeviceToHost));
    if (P) HIP_TRY(hipMemcpy(h_lay, d_layo, (size_t)P * sizeof(sigax_placement), hipMemcpyDeviceToHost));
    if (ng) HIP_TRY(hipMemcpy(h_gaps, d_gaps, (size_t)ng * sizeof(sigax_gap), hipMemcpyDeviceToHost));
    if (sseqs && total) {
      if (total >= (1ull << 43)) return sigax_fail(SIGAX_E_ARG, "scaffold bases: 2^43 bytes or more");
      HIP_TRY(g.alloc(&d_out, (size_t)total));
      a.sseqs = (unsigned char*)d_out;
      a.sseqs_capacity = total;
      launch_gapfill_bases(a, nullptr);
      HIP_TRY(hipGetLastError());
      HIP_TRY(hipMemcpy(h_seqs, d_out, (size_t)total, hipMemcpyDeviceToHost));
    }
    *n_gaps = ng;
  } else {
    h_so = hg.alloc<uint64_t>(8);
    h_lay = hg.alloc<sigax_placement>(0);
    h_gaps = hg.alloc<sigax_gap>(0);
    if (sseqs) h_seqs = hg.alloc<char>(0);
    if (!hg.ok) return sigax_fail(SIGAX_E_CAPACITY, "out of host memory");
    h_so[0] = 0;
  }
  for (int k = 0; k < 24; ++k) status24[k] = status[k];
  *sc_offs = h_so;
  *sc_layout_out = h_lay;
  *gaps = h_gaps;
  if (sseqs) *sseqs = h_seqs;
  hg.release();
  return SIGAX_OK;
}
