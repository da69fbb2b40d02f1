// siga_amd/csrc/sigax_scaffold.cpp -- `siga unitig --scaffold` on the device: the entry points of sigax_scaffold.hip.
#include <cstring>

#include "sigax_internal.h"

static_assert(sizeof(sigax_scaffold_opts) == 32, "sigax_scaffold_opts must be 32 bytes");

namespace {

// where the pieces of the caller's scratch lie (every piece 16-byte aligned)
struct ScafWork {
  u64 cnt, best, deg, link, closing, rank[2], dist[2], hcnt, scan, partial, scan_total, pdst, psrc, plen, bytes;
};
ScafWork scaf_work(u64 n) {
  ScafWork w;
  u64 at = 0;
  auto take = [&](u64 bytes) {
    const u64 here = at;
    at += (bytes + 15) & ~15ull;
    return here;
  };
  w.cnt = take((u64)SCAF_WORDS * 8);
  w.best = take(2 * n * 4);
  w.deg = take(2 * n * 4);
  w.link = take(2 * n * 8);
  w.closing = take(n * 4);
  for (int k = 0; k < 2; ++k) w.rank[k] = take(2 * n * 16);
  for (int k = 0; k < 2; ++k) w.dist[k] = take(2 * n * 8);
  w.hcnt = take(4 * (n + 1) * 4);
  w.scan = take(4 * (n + 1) * 8);
  w.partial = take(scan_partials_needed(n) * 8);
  w.scan_total = take(8);
  w.pdst = take((n + 1) * 8);
  w.psrc = take(n * 8);
  w.plen = take(n * 8);
  w.bytes = at;
  return w;
}

int scaf_limits(u64 max_unitigs, u64 max_links) {
  if (max_unitigs >= (1ull << 31)) return sigax_fail(SIGAX_E_ARG, "max_unitigs: 2^31 unitigs or more: a link names a unitig end in 32 bits");
  if (max_links >= (1ull << 32)) return sigax_fail(SIGAX_E_ARG, "max_links: 2^32 links or more");
  return SIGAX_OK;
}

int scaf_opts_ok(const sigax_scaffold_opts* o) {
  if (!o) return sigax_fail(SIGAX_E_ARG, "NULL where the scaffold options are required");
  if (o->flags & ~SIGAX_SCAFFOLD_INSERT_FROM_STATUS)
    return sigax_fail(SIGAX_E_ARG, "sigax_scaffold_opts.flags 0x%x: SIGAX_SCAFFOLD_INSERT_FROM_STATUS or 0", o->flags);
  if ((o->flags & SIGAX_SCAFFOLD_INSERT_FROM_STATUS) && o->insert_size != 0)
    return sigax_fail(SIGAX_E_ARG, "insert_size must be 0 with SIGAX_SCAFFOLD_INSERT_FROM_STATUS");
  if (o->insert_size >= (1ull << 62)) return sigax_fail(SIGAX_E_ARG, "insert_size %llu: below 2^62", (u64)o->insert_size);
  if (o->min_gap < 1u) return sigax_fail(SIGAX_E_ARG, "min_gap %u: at least 1", o->min_gap);
  if (o->max_gap < o->min_gap) return sigax_fail(SIGAX_E_ARG, "max_gap %u below min_gap %u", o->max_gap, o->min_gap);
  if (o->max_gap >= (1u << 31)) return sigax_fail(SIGAX_E_ARG, "max_gap %u: below 2^31", o->max_gap);
  return SIGAX_OK;
}

// every check of the device form; *a is filled when there is something to launch
int scaf_args(const void* d_n_unitigs, uint64_t max_unitigs, const void* d_seq_offs, const void* d_uflags, const void* d_useqs, uint64_t useqs_bytes,
              const sigax_pair_link* d_links, const void* d_n_links, uint64_t max_links, const void* d_status24, const sigax_scaffold_opts* opts,
              void* d_sc_offs, void* d_sc_lay_offs, void* d_sc_flags, sigax_placement* d_sc_layout, void* d_sseqs, uint64_t sseqs_capacity,
              void* d_status16, void* d_work, uint64_t work_bytes, ScaffoldArgs* a) {
  const int rl = scaf_limits(max_unitigs, max_links);
  if (rl != SIGAX_OK) return rl;
  const int ro = scaf_opts_ok(opts);
  if (ro != SIGAX_OK) return ro;
  if (!d_status16) return sigax_fail(SIGAX_E_ARG, "d_status16: NULL where a buffer is required");
  if ((uintptr_t)d_status16 & 7) return sigax_fail(SIGAX_E_ARG, "d_status16 must be 8-byte aligned");
  if (!d_sseqs && sseqs_capacity) return sigax_fail(SIGAX_E_ARG, "d_sseqs: NULL with a capacity of %llu bytes", (u64)sseqs_capacity);
  if (sseqs_capacity >= (1ull << 43)) return sigax_fail(SIGAX_E_ARG, "sseqs_capacity: 2^43 bytes or more");
  if ((uintptr_t)d_sseqs & 15) return sigax_fail(SIGAX_E_ARG, "d_sseqs must be 16-byte aligned");
  if (max_unitigs == 0) return SIGAX_OK;
  const struct { const void* p; const char* name; unsigned align; bool needed; } bufs[] = {
      {d_n_unitigs, "d_n_unitigs", 8, true}, {d_seq_offs, "d_seq_offs", 8, true}, {d_uflags, "d_uflags", 4, true},
      {d_useqs, "d_useqs", 16, d_sseqs != nullptr}, {d_links, "d_links", 8, max_links != 0}, {d_n_links, "d_n_links", 8, max_links != 0},
      {d_status24, "d_status24", 8, (opts->flags & SIGAX_SCAFFOLD_INSERT_FROM_STATUS) != 0}, {d_sc_offs, "d_sc_offs", 8, true},
      {d_sc_lay_offs, "d_sc_lay_offs", 8, true}, {d_sc_flags, "d_sc_flags", 4, true}, {d_sc_layout, "d_sc_layout", 16, true},
      {d_work, "d_work", 16, true}};
  for (const auto& b : bufs) {
    if (b.needed && !b.p) return sigax_fail(SIGAX_E_ARG, "%s: NULL where a buffer is required", b.name);
    if ((uintptr_t)b.p & (b.align - 1)) return sigax_fail(SIGAX_E_ARG, "%s must be %u-byte aligned", b.name, b.align);
  }
  const ScafWork w = scaf_work(max_unitigs);
  if (work_bytes < w.bytes)
    return sigax_fail(SIGAX_E_ARG, "workspace of %llu bytes, %llu needed (sigax_scaffold_workspace)", (u64)work_bytes, w.bytes);
  char* base = (char*)d_work;
  a->n_unitigs = (const u64*)d_n_unitigs;
  a->n_links = (const u64*)d_n_links;
  a->max_unitigs = max_unitigs;
  a->max_links = max_links;
  a->seq_offs = (const u64*)d_seq_offs;
  a->uflags = (const uint32_t*)d_uflags;
  a->useqs = (const unsigned char*)d_useqs;
  a->useqs_bytes = d_useqs ? useqs_bytes : 0;
  a->links = d_links;
  a->status24 = (const u64*)d_status24;
  a->flags = opts->flags;
  a->min_pairs = opts->min_pairs;
  a->link_ratio = opts->link_ratio;
  a->min_unitig_bases = opts->min_unitig_bases;
  a->min_gap = opts->min_gap;
  a->max_gap = opts->max_gap;
  a->insert_size = opts->insert_size;
  a->sc_offs = (u64*)d_sc_offs;
  a->sc_lay_offs = (u64*)d_sc_lay_offs;
  a->sc_flags = (uint32_t*)d_sc_flags;
  a->sc_layout = d_sc_layout;
  a->sseqs = (unsigned char*)d_sseqs;
  a->sseqs_capacity = d_sseqs ? sseqs_capacity : 0;
  a->status = (u64*)d_status16;
  a->cnt = (u64*)(base + w.cnt);
  a->best = (uint32_t*)(base + w.best);
  a->deg = (uint32_t*)(base + w.deg);
  a->link = (uint2*)(base + w.link);
  a->closing = (uint32_t*)(base + w.closing);
  for (int k = 0; k < 2; ++k) {
    a->rank[k] = (u64*)(base + w.rank[k]);
    a->dist[k] = (u64*)(base + w.dist[k]);
  }
  a->hcnt = (uint32_t*)(base + w.hcnt);
  a->scan = (u64*)(base + w.scan);
  a->partial = (u64*)(base + w.partial);
  a->scan_total = (u64*)(base + w.scan_total);
  a->pdst = (u64*)(base + w.pdst);
  a->psrc = (u64*)(base + w.psrc);
  a->plen = (u64*)(base + w.plen);
  return SIGAX_OK;
}

}  // namespace

extern "C" int sigax_scaffold_workspace(uint64_t max_unitigs, uint64_t max_links, uint64_t* bytes) {
  if (!bytes) return sigax_fail(SIGAX_E_ARG, "bytes: NULL where a result is required");
  const int rc = scaf_limits(max_unitigs, max_links);
  if (rc != SIGAX_OK) return rc;
  *bytes = max_unitigs ? scaf_work(max_unitigs).bytes : 0;
  return SIGAX_OK;
}

extern "C" int sigax_scaffold_device(int device, const void* d_n_unitigs, uint64_t max_unitigs, const void* d_seq_offs, const void* d_uflags,
                                     const void* d_useqs, uint64_t useqs_bytes, const sigax_pair_link* d_links, const void* d_n_links,
                                     uint64_t max_links, const void* d_status24, const sigax_scaffold_opts* opts, void* d_sc_offs,
                                     void* d_sc_lay_offs, void* d_sc_flags, sigax_placement* d_sc_layout, void* d_sseqs, uint64_t sseqs_capacity,
                                     void* d_status16, void* d_work, uint64_t work_bytes, void* stream) {
  ScaffoldArgs a;
  const int rc = scaf_args(d_n_unitigs, max_unitigs, d_seq_offs, d_uflags, d_useqs, useqs_bytes, d_links, d_n_links, max_links, d_status24, opts,
                           d_sc_offs, d_sc_lay_offs, d_sc_flags, d_sc_layout, d_sseqs, sseqs_capacity, d_status16, d_work, work_bytes, &a);
  if (rc != SIGAX_OK) return rc;
  HIP_TRY(hipSetDevice(device));
  const hipStream_t st = (hipStream_t)stream;
  if (max_unitigs == 0) {
    HIP_TRY(hipMemsetAsync(d_status16, 0, 16 * 8, st));
    if (d_sc_offs) HIP_TRY(hipMemsetAsync(d_sc_offs, 0, 8, st));  // no scaffolds: the tables' one entry, where they are given
    if (d_sc_lay_offs) HIP_TRY(hipMemsetAsync(d_sc_lay_offs, 0, 8, st));
    return SIGAX_OK;
  }
  HIP_TRY(launch_scaffold(a, st));
  return SIGAX_OK;
}

extern "C" int sigax_scaffold_bases_device(int device, const void* d_n_unitigs, uint64_t max_unitigs, const void* d_seq_offs, const void* d_uflags,
                                           const void* d_useqs, uint64_t useqs_bytes, const sigax_pair_link* d_links, const void* d_n_links,
                                           uint64_t max_links, const void* d_status24, const sigax_scaffold_opts* opts, void* d_sc_offs,
                                           void* d_sc_lay_offs, void* d_sc_flags, sigax_placement* d_sc_layout, void* d_sseqs,
                                           uint64_t sseqs_capacity, void* d_status16, void* d_work, uint64_t work_bytes, void* stream) {
  ScaffoldArgs a;
  const int rc = scaf_args(d_n_unitigs, max_unitigs, d_seq_offs, d_uflags, d_useqs, useqs_bytes, d_links, d_n_links, max_links, d_status24, opts,
                           d_sc_offs, d_sc_lay_offs, d_sc_flags, d_sc_layout, d_sseqs, sseqs_capacity, d_status16, d_work, work_bytes, &a);
  if (rc != SIGAX_OK) return rc;
  if (max_unitigs == 0) return SIGAX_OK;
  HIP_TRY(hipSetDevice(device));
  launch_scaffold_bases(a, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return SIGAX_OK;
}

extern "C" int sigax_scaffold_host(int device, uint64_t n_unitigs, const uint64_t* seq_offs, const uint32_t* uflags, const char* useqs,
                                   const sigax_pair_link* links, uint64_t n_links, const uint64_t* status24, const sigax_scaffold_opts* opts,
                                   uint64_t* n_scaffolds, uint64_t** sc_offs, uint64_t** sc_lay_offs, uint32_t** sc_flags,
                                   sigax_placement** sc_layout, char** sseqs, uint64_t status16[16]) {
  if (!n_scaffolds || !sc_offs || !sc_lay_offs || !sc_flags || !sc_layout || !status16)
    return sigax_fail(SIGAX_E_ARG, "NULL where a result is required");
  *n_scaffolds = 0;
  *sc_offs = *sc_lay_offs = nullptr;
  *sc_flags = nullptr;
  *sc_layout = nullptr;
  if (sseqs) *sseqs = nullptr;
  for (int k = 0; k < 16; ++k) status16[k] = 0;
  const int rl = scaf_limits(n_unitigs, n_links);
  if (rl != SIGAX_OK) return rl;
  const int ro = scaf_opts_ok(opts);
  if (ro != SIGAX_OK) return ro;
  const u64 n = n_unitigs;
  if (n && (!seq_offs || !uflags)) return sigax_fail(SIGAX_E_ARG, "seq_offs, uflags: NULL where a buffer is required");
  if (n && n_links && !links) return sigax_fail(SIGAX_E_ARG, "links: NULL where a buffer is required");
  if ((opts->flags & SIGAX_SCAFFOLD_INSERT_FROM_STATUS) && !status24) return sigax_fail(SIGAX_E_ARG, "status24: NULL with SIGAX_SCAFFOLD_INSERT_FROM_STATUS");
  const u64 ubytes = n ? seq_offs[n] : 0;
  if (n && sseqs && ubytes && !useqs) return sigax_fail(SIGAX_E_ARG, "useqs: NULL where the bases are asked for");
  HostGuard hg;
  u64 status[16];
  memset(status, 0, sizeof status);
  uint64_t *h_so = nullptr, *h_lo = nullptr;
  uint32_t* h_fl = nullptr;
  sigax_placement* h_lay = nullptr;
  char* h_seqs = nullptr;
  if (n) {
    HIP_TRY(hipSetDevice(device));
    const ScafWork w = scaf_work(n);
    DevGuard g;
    void *d_cnt, *d_so, *d_uf, *d_us = nullptr, *d_links = nullptr, *d_s24, *d_sco, *d_scl, *d_scf, *d_lay, *d_st, *d_work, *d_out = nullptr;
    HIP_TRY(g.alloc(&d_cnt, 16));  // {n_unitigs, n_links}
    HIP_TRY(g.alloc(&d_so, ((size_t)n + 1) * 8));
    HIP_TRY(g.alloc(&d_uf, (size_t)n * 4));
    if (sseqs) HIP_TRY(g.alloc(&d_us, (size_t)ubytes));
    if (n_links) HIP_TRY(g.alloc(&d_links, (size_t)n_links * sizeof(sigax_pair_link)));
    HIP_TRY(g.alloc(&d_s24, 24 * 8));
    HIP_TRY(g.alloc(&d_sco, ((size_t)n + 1) * 8));
    HIP_TRY(g.alloc(&d_scl, ((size_t)n + 1) * 8));
    HIP_TRY(g.alloc(&d_scf, (size_t)n * 4));
    HIP_TRY(g.alloc(&d_lay, (size_t)n * sizeof(sigax_placement)));
    HIP_TRY(g.alloc(&d_st, 16 * 8));
    HIP_TRY(g.alloc(&d_work, (size_t)w.bytes));
    const u64 counts[2] = {n, n_links};
    HIP_TRY(hipMemcpy(d_cnt, counts, 16, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_so, seq_offs, ((size_t)n + 1) * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_uf, uflags, (size_t)n * 4, hipMemcpyHostToDevice));
    if (sseqs && ubytes) HIP_TRY(hipMemcpy(d_us, useqs, (size_t)ubytes, hipMemcpyHostToDevice));
    if (n_links) HIP_TRY(hipMemcpy(d_links, links, (size_t)n_links * sizeof(sigax_pair_link), hipMemcpyHostToDevice));
    if (status24) HIP_TRY(hipMemcpy(d_s24, status24, 24 * 8, hipMemcpyHostToDevice));
    else HIP_TRY(hipMemset(d_s24, 0, 24 * 8));
    // the layout alone, then the bases into a buffer of exactly their size
    int rc = sigax_scaffold_device(device, d_cnt, n, d_so, d_uf, nullptr, 0, (const sigax_pair_link*)d_links, (u64*)d_cnt + 1, n_links, d_s24, opts, d_sco,
                                   d_scl, d_scf, (sigax_placement*)d_lay, nullptr, 0, d_st, d_work, w.bytes, nullptr);
    if (rc != SIGAX_OK) return rc;
    HIP_TRY(hipMemcpy(status, d_st, 16 * 8, hipMemcpyDeviceToHost));  // (waits for the null stream's kernels)
    const u64 S = status[0], total = status[1];
    if (S > n) return sigax_fail(SIGAX_E_DEVICE, "scaffolds beyond their buffer");
    status[15] = 0;
    h_so = hg.alloc<uint64_t>(((size_t)S + 1) * 8);
    h_lo = hg.alloc<uint64_t>(((size_t)S + 1) * 8);
    h_fl = hg.alloc<uint32_t>((size_t)S * 4);
    h_lay = hg.alloc<sigax_placement>((size_t)n * sizeof(sigax_placement));
    if (sseqs) h_seqs = hg.alloc<char>((size_t)total);
    if (!hg.ok) return sigax_fail(SIGAX_E_CAPACITY, "out of host memory");
    HIP_TRY(hipMemcpy(h_so, d_sco, ((size_t)S + 1) * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(h_lo, d_scl, ((size_t)S + 1) * 8, hipMemcpyDeviceToHost));
    if (S) HIP_TRY(hipMemcpy(h_fl, d_scf, (size_t)S * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(h_lay, d_lay, (size_t)n * sizeof(sigax_placement), hipMemcpyDeviceToHost));
    if (sseqs && total) {
      HIP_TRY(g.alloc(&d_out, (size_t)total));
      rc = sigax_scaffold_bases_device(device, d_cnt, n, d_so, d_uf, d_us, ubytes, (const sigax_pair_link*)d_links, (u64*)d_cnt + 1, n_links, d_s24, opts,
                                       d_sco, d_scl, d_scf, (sigax_placement*)d_lay, d_out, total, d_st, d_work, w.bytes, nullptr);
      if (rc != SIGAX_OK) return rc;
      HIP_TRY(hipMemcpy(h_seqs, d_out, (size_t)total, hipMemcpyDeviceToHost));
    }
  } else {
    h_so = hg.alloc<uint64_t>(8);
    h_lo = hg.alloc<uint64_t>(8);
    h_fl = hg.alloc<uint32_t>(0);
    h_lay = hg.alloc<sigax_placement>(0);
    if (sseqs) h_seqs = hg.alloc<char>(0);
    if (!hg.ok) return sigax_fail(SIGAX_E_CAPACITY, "out of host memory");
    h_so[0] = h_lo[0] = 0;
  }
  for (int k = 0; k < 16; ++k) status16[k] = status[k];
  *n_scaffolds = status[0];
  *sc_offs = h_so;
  *sc_lay_offs = h_lo;
  *sc_flags = h_fl;
  *sc_layout = h_lay;
  if (sseqs) *sseqs = h_seqs;
  hg.release();
  return SIGAX_OK;
}
