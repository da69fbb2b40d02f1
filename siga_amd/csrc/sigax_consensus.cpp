// siga_amd/csrc/sigax_consensus.cpp -- the consensus pass of `siga unitig -e` on the device: the entry points of sigax_consensus.hip.
#include <cstring>

#include "sigax_consensus.h"
#include "sigax_internal.h"

static_assert(sizeof(sigax_consensus_opts) == 16, "sigax_consensus_opts must be 16 bytes");

namespace {

constexpr u64 CONS_WORK_BYTES = ((u64)CONS_WORDS * 8 + 15) & ~15ull;  // the counters: the same for every read set

int cons_limits(u64 n_reads) {
  if (n_reads >= (1ull << 31)) return sigax_fail(SIGAX_E_ARG, "2^31 reads or more: a placement names its read in 32 bits");
  return SIGAX_OK;
}

int cons_opts_ok(const sigax_consensus_opts* o) {
  if (!o) return sigax_fail(SIGAX_E_ARG, "NULL where the consensus options are required");
  if (o->min_votes == 0) return sigax_fail(SIGAX_E_ARG, "min_votes 0: at least 1");
  if (o->reserved[0] | o->reserved[1] | o->reserved[2]) return sigax_fail(SIGAX_E_ARG, "sigax_consensus_opts.reserved must be 0");
  return SIGAX_OK;
}

}  // namespace

extern "C" int sigax_consensus_workspace(uint64_t n_reads, uint64_t n_unitigs_max, uint64_t* bytes) {
  if (!bytes) return sigax_fail(SIGAX_E_ARG, "bad argument");
  (void)n_unitigs_max;
  const int rc = cons_limits(n_reads);
  if (rc != SIGAX_OK) return rc;
  *bytes = CONS_WORK_BYTES;
  return SIGAX_OK;
}

extern "C" int sigax_consensus_device(int device, const void* d_n_unitigs, uint64_t max_unitigs, const void* d_seq_offs, const void* d_lay_offs,
                                      const sigax_placement* d_layout, const void* d_lengths, const void* d_seqs, const void* d_offs,
                                      uint64_t n_reads, const sigax_consensus_opts* opts, void* d_useqs, void* d_changed, void* d_support,
                                      void* d_status8, void* d_work, uint64_t work_bytes, void* stream) {
  const int rl = cons_limits(n_reads);
  if (rl != SIGAX_OK) return rl;
  const int ro = cons_opts_ok(opts);
  if (ro != SIGAX_OK) return ro;
  if (!d_status8) return sigax_fail(SIGAX_E_ARG, "NULL where a buffer is required");
  if ((uintptr_t)d_status8 & 7) return sigax_fail(SIGAX_E_ARG, "d_status8 must be 8-byte aligned");
  const bool work = n_reads != 0 && max_unitigs != 0;
  if (work && (!d_n_unitigs || !d_seq_offs || !d_lay_offs || !d_layout || !d_lengths || !d_seqs || !d_offs || !d_useqs || !d_changed || !d_work))
    return sigax_fail(SIGAX_E_ARG, "NULL where a buffer is required");
  if (work && (((uintptr_t)d_layout | (uintptr_t)d_useqs | (uintptr_t)d_support | (uintptr_t)d_work) & 15))
    return sigax_fail(SIGAX_E_ARG, "d_layout, d_useqs, d_support and d_work must be 16-byte aligned");
  if (work && (((uintptr_t)d_n_unitigs | (uintptr_t)d_seq_offs | (uintptr_t)d_lay_offs | (uintptr_t)d_offs) & 7))
    return sigax_fail(SIGAX_E_ARG, "d_n_unitigs, d_seq_offs, d_lay_offs and d_offs must be 8-byte aligned");
  if (work && (((uintptr_t)d_lengths | (uintptr_t)d_changed) & 3)) return sigax_fail(SIGAX_E_ARG, "d_lengths and d_changed must be 4-byte aligned");
  if (work && work_bytes < CONS_WORK_BYTES)
    return sigax_fail(SIGAX_E_ARG, "workspace of %llu bytes, %llu needed (sigax_consensus_workspace)", (u64)work_bytes, CONS_WORK_BYTES);
  HIP_TRY(hipSetDevice(device));
  const hipStream_t st = (hipStream_t)stream;
  if (!work) {
    HIP_TRY(hipMemsetAsync(d_status8, 0, 8 * 8, st));
    return SIGAX_OK;
  }
  ConsArgs a;
  a.n_unitigs = (const u64*)d_n_unitigs;
  a.max_unitigs = max_unitigs;
  a.seq_offs = (const u64*)d_seq_offs;
  a.lay_offs = (const u64*)d_lay_offs;
  a.layout = d_layout;
  a.lengths = (const uint32_t*)d_lengths;
  a.seqs = (const unsigned char*)d_seqs;
  a.offs = (const u64*)d_offs;
  a.n_reads = n_reads;
  a.min_votes = opts->min_votes;
  a.useqs = (unsigned char*)d_useqs;
  a.changed = (uint32_t*)d_changed;
  a.support = (unsigned char*)d_support;
  a.status = (u64*)d_status8;
  a.cnt = (u64*)d_work;
  HIP_TRY(hipMemsetAsync(d_work, 0, (size_t)CONS_WORK_BYTES, st));
  HIP_TRY(hipMemsetAsync(d_changed, 0, (size_t)max_unitigs * 4, st));
  HIP_TRY(launch_consensus(a, st));
  return SIGAX_OK;
}

extern "C" int sigax_consensus_host(int device, uint64_t n_unitigs, const uint64_t* seq_offs, const uint64_t* lay_offs, const sigax_placement* layout,
                                    const uint32_t* lengths, const char* seqs, const uint64_t* offs, uint64_t n_reads,
                                    const sigax_consensus_opts* opts, char* useqs, uint32_t** changed, uint8_t** support, uint64_t status8[8]) {
  if (!changed || !status8) return sigax_fail(SIGAX_E_ARG, "NULL where a buffer is required");
  *changed = nullptr;
  if (support) *support = nullptr;
  for (int k = 0; k < 8; ++k) status8[k] = 0;
  const int rl = cons_limits(n_reads);
  if (rl != SIGAX_OK) return rl;
  const int ro = cons_opts_ok(opts);
  if (ro != SIGAX_OK) return ro;
  const u64 n = n_reads, nu = n_unitigs;
  if (nu > n) return sigax_fail(SIGAX_E_ARG, "%llu unitigs of %llu reads", nu, n);
  if (n && (!lengths || !offs || !seq_offs || !lay_offs)) return sigax_fail(SIGAX_E_ARG, "NULL where a buffer is required");
  const u64 placed = n ? lay_offs[nu] : 0, bases = n ? seq_offs[nu] : 0;
  if (placed > n) return sigax_fail(SIGAX_E_ARG, "%llu placements of %llu reads", placed, n);
  if (n && offs[n] < offs[0]) return sigax_fail(SIGAX_E_ARG, "bad offsets");
  const u64 cap = n ? offs[n] - offs[0] : 0;
  if (bases > cap) return sigax_fail(SIGAX_E_ARG, "%llu unitig bases of %llu read bases", bases, cap);
  if ((placed && !layout) || (cap && !seqs) || (bases && !useqs)) return sigax_fail(SIGAX_E_ARG, "NULL where a buffer is required");
  HostGuard hg;
  uint32_t* h_changed = hg.alloc<uint32_t>((size_t)nu * 4);
  uint8_t* h_support = support ? hg.alloc<uint8_t>((size_t)bases) : nullptr;
  if (!hg.ok) return sigax_fail(SIGAX_E_CAPACITY, "out of host memory");
  if (n && nu) {
    HIP_TRY(hipSetDevice(device));
    DevGuard g;
    void *d_so, *d_lo, *d_lay, *d_len, *d_seqs, *d_offs, *d_us, *d_ch, *d_sup = nullptr, *d_status, *d_work;
    HIP_TRY(g.alloc(&d_so, ((size_t)nu + 1) * 8));
    HIP_TRY(g.alloc(&d_lo, ((size_t)nu + 1) * 8));
    HIP_TRY(g.alloc(&d_lay, (size_t)n * sizeof(sigax_placement)));
    HIP_TRY(g.alloc(&d_len, (size_t)n * 4));
    HIP_TRY(g.alloc(&d_seqs, (size_t)cap + 16));
    HIP_TRY(g.alloc(&d_offs, ((size_t)n + 1) * 8));
    HIP_TRY(g.alloc(&d_us, (size_t)cap + 16));
    HIP_TRY(g.alloc(&d_ch, (size_t)nu * 4));
    if (support) HIP_TRY(g.alloc(&d_sup, (size_t)cap + 16));
    HIP_TRY(g.alloc(&d_status, 16 * 8));
    HIP_TRY(g.alloc(&d_work, (size_t)CONS_WORK_BYTES));
    HIP_TRY(hipMemcpy(d_so, seq_offs, ((size_t)nu + 1) * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_lo, lay_offs, ((size_t)nu + 1) * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(d_lay, 0xFF, (size_t)n * sizeof(sigax_placement)));  // (what lies behind the placements names no read)
    if (placed) HIP_TRY(hipMemcpy(d_lay, layout, (size_t)placed * sizeof(sigax_placement), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_len, lengths, (size_t)n * 4, hipMemcpyHostToDevice));
    if (cap) HIP_TRY(hipMemcpy(d_seqs, seqs + offs[0], (size_t)cap, hipMemcpyHostToDevice));
    // the device's copy of the bases begins at 0: its offsets are the caller's less offs[0]
    std::vector<u64> rel((size_t)n + 1);
    for (u64 i = 0; i <= n; ++i) rel[i] = offs[i] - offs[0];
    HIP_TRY(hipMemcpy(d_offs, rel.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice));
    if (bases) HIP_TRY(hipMemcpy(d_us, useqs, (size_t)bases, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy((u64*)d_status + 8, &nu, 8, hipMemcpyHostToDevice));  // the count the device reads: behind the 8 status words
    const int rc = sigax_consensus_device(device, (u64*)d_status + 8, nu, d_so, d_lo, (const sigax_placement*)d_lay, d_len, d_seqs, d_offs, n, opts,
                                          d_us, d_ch, d_sup, d_status, d_work, CONS_WORK_BYTES, nullptr);
    if (rc != SIGAX_OK) return rc;
    HIP_TRY(hipMemcpy(status8, d_status, 8 * 8, hipMemcpyDeviceToHost));  // (waits for the null stream's kernels)
    HIP_TRY(hipMemcpy(h_changed, d_ch, (size_t)nu * 4, hipMemcpyDeviceToHost));
    if (bases) HIP_TRY(hipMemcpy(useqs, d_us, (size_t)bases, hipMemcpyDeviceToHost));
    if (support && bases) HIP_TRY(hipMemcpy(h_support, d_sup, (size_t)bases, hipMemcpyDeviceToHost));
  }
  *changed = h_changed;
  if (support) *support = h_support;
  hg.release();
  return SIGAX_OK;
}
