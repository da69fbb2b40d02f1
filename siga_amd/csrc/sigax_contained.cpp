// siga_amd/csrc/sigax_contained.cpp -- contained reads placed in a unitig call's layout: the entry points of sigax_contained.hip.
#include <algorithm>
#include <cstring>

#include "sigax_contained.h"
#include "sigax_internal.h"

static_assert(sizeof(sigax_contained_opts) == 16, "sigax_contained_opts must be 16 bytes");

namespace {

struct ContWork {
  u64 best1, best2, slot, owner, state0, state1, pu, pflags, poff, keys0, keys1, vals0, vals1, kept, keptscan, cnt, partial, words, sort_tmp,
      sort_tmp_bytes, bytes;
};

int cont_limits(u64 n_reads, u64 n_conts) {
  if (n_reads >= (1ull << 31)) return sigax_fail(SIGAX_E_ARG, "2^31 reads or more: a placement names its read in 32 bits");
  if (n_conts > 0xFFFFFFFFull) return sigax_fail(SIGAX_E_ARG, "n_conts %llu: at most 2^32 - 1 containment records", n_conts);
  return SIGAX_OK;
}

int cont_opts_ok(const sigax_contained_opts* o) {
  if (!o) return sigax_fail(SIGAX_E_ARG, "NULL where the placement options are required");
  if (o->reserved[0] | o->reserved[1] | o->reserved[2] | o->reserved[3]) return sigax_fail(SIGAX_E_ARG, "sigax_contained_opts.reserved must be 0");
  return SIGAX_OK;
}

int cont_work(u64 n, u64 m, ContWork* out) {
  ContWork w;
  u64 at = 0;
  auto take = [&at](u64 bytes) {
    const u64 here = at;
    at += (bytes + 15) & ~15ull;
    return here;
  };
  w.best1 = take(n * 8);  // best1 and best2 lie together: one fill
  w.best2 = take(n * 8);
  w.slot = take(n * 4);
  w.owner = take(n * 4);
  w.state0 = take(n * 16);
  w.state1 = take(n * 16);
  w.pu = take(n * 4);
  w.pflags = take(n * 4);
  w.poff = take(n * 8);
  w.keys0 = take(n * 8);
  w.keys1 = take(n * 8);
  w.vals0 = take(n * 4);
  w.vals1 = take(n * 4);
  w.kept = take(n * 4);
  w.keptscan = take((n + 1) * 8);
  w.cnt = take(m * 4);
  w.partial = take(scan_partials_needed(std::max(n, m)) * 8);
  w.words = take(CP_WORDS * 8);
  u64 tb = 0;
  const hipError_t e = contained_sort_bytes(n, &tb);
  if (e != hipSuccess) return sigax_fail(SIGAX_E_DEVICE, "the sort's workspace: %s", hipGetErrorString(e));
  w.sort_tmp_bytes = tb;
  w.sort_tmp = take(tb);
  w.bytes = at + 16;
  *out = w;
  return SIGAX_OK;
}

}  // namespace

extern "C" int sigax_contained_place_workspace(uint64_t n_reads, uint64_t max_unitigs, uint64_t n_conts, uint64_t* bytes) {
  if (!bytes) return sigax_fail(SIGAX_E_ARG, "bad argument");
  const int rc = cont_limits(n_reads, n_conts);
  if (rc != SIGAX_OK) return rc;
  if (max_unitigs > n_reads) max_unitigs = n_reads;
  ContWork w;
  const int rw = cont_work(n_reads, max_unitigs, &w);
  if (rw != SIGAX_OK) return rw;
  *bytes = w.bytes;
  return SIGAX_OK;
}

extern "C" int sigax_contained_place_device(int device, const void* d_n_unitigs, uint64_t max_unitigs, const void* d_seq_offs, const void* d_lay_offs,
                                            const sigax_placement* d_layout, const void* d_lengths, uint64_t n_reads, const void* d_contained,
                                            const sigax_mm_edge* d_conts, uint64_t n_conts, const sigax_contained_opts* opts, void* d_lay_offs2,
                                            sigax_placement* d_layout2, void* d_place_class, void* d_status8, void* d_work, uint64_t work_bytes,
                                            void* stream) {
  const int rl = cont_limits(n_reads, n_conts);
  if (rl != SIGAX_OK) return rl;
  const int ro = cont_opts_ok(opts);
  if (ro != SIGAX_OK) return ro;
  if (!d_status8) return sigax_fail(SIGAX_E_ARG, "NULL where a buffer is required");
  if ((uintptr_t)d_status8 & 7) return sigax_fail(SIGAX_E_ARG, "d_status8 must be 8-byte aligned");
  const bool work = n_reads != 0 && max_unitigs != 0;
  if (work && (!d_n_unitigs || !d_seq_offs || !d_lay_offs || !d_layout || !d_lengths || !d_contained || (!d_conts && n_conts) || !d_lay_offs2 ||
               !d_layout2 || !d_place_class || !d_work))
    return sigax_fail(SIGAX_E_ARG, "NULL where a buffer is required");
  if (work && (((uintptr_t)d_layout | (uintptr_t)d_layout2 | (uintptr_t)d_work) & 15))
    return sigax_fail(SIGAX_E_ARG, "d_layout, d_layout2 and d_work must be 16-byte aligned");
  if (work && (((uintptr_t)d_n_unitigs | (uintptr_t)d_seq_offs | (uintptr_t)d_lay_offs | (uintptr_t)d_lay_offs2 | (uintptr_t)d_conts) & 7))
    return sigax_fail(SIGAX_E_ARG, "d_n_unitigs, d_seq_offs, d_lay_offs, d_lay_offs2 and d_conts must be 8-byte aligned");
  if (work && ((uintptr_t)d_lengths & 3)) return sigax_fail(SIGAX_E_ARG, "d_lengths must be 4-byte aligned");
  HIP_TRY(hipSetDevice(device));
  const hipStream_t st = (hipStream_t)stream;
  if (!work) {
    HIP_TRY(hipMemsetAsync(d_status8, 0, 8 * 8, st));
    return SIGAX_OK;
  }
  if (max_unitigs > n_reads) max_unitigs = n_reads;  // a unitig holds a read: the tables' entries beyond are never read
  ContWork w;
  const int rw = cont_work(n_reads, max_unitigs, &w);
  if (rw != SIGAX_OK) return rw;
  if (work_bytes < w.bytes)
    return sigax_fail(SIGAX_E_ARG, "workspace of %llu bytes, %llu needed (sigax_contained_place_workspace)", (u64)work_bytes, w.bytes);
  char* base = (char*)d_work;
  ContArgs a;
  a.n_unitigs = (const u64*)d_n_unitigs;
  a.max_unitigs = max_unitigs;
  a.seq_offs = (const u64*)d_seq_offs;
  a.lay_offs = (const u64*)d_lay_offs;
  a.layout = d_layout;
  a.lengths = (const uint32_t*)d_lengths;
  a.n_reads = n_reads;
  a.contained = (const unsigned char*)d_contained;
  a.conts = d_conts;
  a.n_conts = n_conts;
  a.lay_offs2 = (u64*)d_lay_offs2;
  a.layout2 = d_layout2;
  a.place_class = (unsigned char*)d_place_class;
  a.status = (u64*)d_status8;
  a.best1 = (u64*)(base + w.best1);
  a.best2 = (u64*)(base + w.best2);
  a.slot = (uint32_t*)(base + w.slot);
  a.owner = (uint32_t*)(base + w.owner);
  a.state[0] = (uint4*)(base + w.state0);
  a.state[1] = (uint4*)(base + w.state1);
  a.pu = (uint32_t*)(base + w.pu);
  a.pflags = (uint32_t*)(base + w.pflags);
  a.poff = (u64*)(base + w.poff);
  a.keys[0] = (u64*)(base + w.keys0);
  a.keys[1] = (u64*)(base + w.keys1);
  a.vals[0] = (uint32_t*)(base + w.vals0);
  a.vals[1] = (uint32_t*)(base + w.vals1);
  a.kept = (uint32_t*)(base + w.kept);
  a.keptscan = (u64*)(base + w.keptscan);
  a.cnt = (uint32_t*)(base + w.cnt);
  a.partial = (u64*)(base + w.partial);
  a.words = (u64*)(base + w.words);
  a.sort_tmp = base + w.sort_tmp;
  a.sort_tmp_bytes = w.sort_tmp_bytes;
  a.rounds = unitig_rounds(n_reads);
  // best1, best2 and slot: no record and no placement seen yet; layout2: nothing placed
  HIP_TRY(hipMemsetAsync(base + w.best1, 0xFF, (size_t)(w.owner - w.best1), st));
  HIP_TRY(hipMemsetAsync(base + w.words, 0, CP_WORDS * 8, st));
  HIP_TRY(hipMemsetAsync(d_layout2, 0xFF, (size_t)n_reads * sizeof(sigax_placement), st));
  const hipError_t e = launch_contained_place(a, st);
  if (e != hipSuccess) return sigax_fail(SIGAX_E_DEVICE, "placing the contained reads: %s", hipGetErrorString(e));
  return SIGAX_OK;
}

extern "C" int sigax_contained_place_host(int device, uint64_t n_unitigs, const uint64_t* seq_offs, const uint64_t* lay_offs,
                                          const sigax_placement* layout, const uint32_t* lengths, uint64_t n_reads, const uint8_t* contained,
                                          const sigax_mm_edge* conts, uint64_t n_conts, const sigax_contained_opts* opts, uint64_t** lay_offs2,
                                          sigax_placement** layout2, uint8_t** place_class, uint64_t status8[8]) {
  if (!lay_offs2 || !layout2 || !place_class || !status8) return sigax_fail(SIGAX_E_ARG, "NULL where a buffer is required");
  *lay_offs2 = nullptr;
  *layout2 = nullptr;
  *place_class = nullptr;
  for (int k = 0; k < 8; ++k) status8[k] = 0;
  const int rl = cont_limits(n_reads, n_conts);
  if (rl != SIGAX_OK) return rl;
  const int ro = cont_opts_ok(opts);
  if (ro != SIGAX_OK) return ro;
  const u64 n = n_reads, nu = n_unitigs;
  if (nu > n) return sigax_fail(SIGAX_E_ARG, "%llu unitigs of %llu reads", nu, n);
  if (n && (!lengths || !contained || !seq_offs || !lay_offs || (n_conts && !conts))) return sigax_fail(SIGAX_E_ARG, "NULL where a buffer is required");
  const u64 placed = n ? lay_offs[nu] : 0;
  if (placed > n) return sigax_fail(SIGAX_E_ARG, "%llu placements of %llu reads", placed, n);
  if (placed && !layout) return sigax_fail(SIGAX_E_ARG, "NULL where a buffer is required");
  HostGuard hg;
  uint64_t* h_lo2 = hg.alloc<uint64_t>(((size_t)nu + 1) * 8);
  sigax_placement* h_lay2 = hg.alloc<sigax_placement>((size_t)std::max<u64>(n, 1) * sizeof(sigax_placement));
  uint8_t* h_class = hg.alloc<uint8_t>((size_t)std::max<u64>(n, 1));
  if (!hg.ok) return sigax_fail(SIGAX_E_CAPACITY, "out of host memory");
  memset(h_lo2, 0, ((size_t)nu + 1) * 8);
  memset(h_class, 0, (size_t)std::max<u64>(n, 1));
  memset(h_lay2, 0xFF, (size_t)std::max<u64>(n, 1) * sizeof(sigax_placement));
  if (n && nu) {
    HIP_TRY(hipSetDevice(device));
    uint64_t wb = 0;
    const int rw = sigax_contained_place_workspace(n, nu, n_conts, &wb);
    if (rw != SIGAX_OK) return rw;
    DevGuard g;
    void *d_so, *d_lo, *d_lay, *d_len, *d_cont, *d_recs = nullptr, *d_lo2, *d_lay2, *d_class, *d_status, *d_work;
    HIP_TRY(g.alloc(&d_so, ((size_t)nu + 1) * 8));
    HIP_TRY(g.alloc(&d_lo, ((size_t)nu + 1) * 8));
    HIP_TRY(g.alloc(&d_lay, (size_t)n * sizeof(sigax_placement)));
    HIP_TRY(g.alloc(&d_len, (size_t)n * 4));
    HIP_TRY(g.alloc(&d_cont, (size_t)n));
    if (n_conts) HIP_TRY(g.alloc(&d_recs, (size_t)n_conts * sizeof(sigax_mm_edge)));
    HIP_TRY(g.alloc(&d_lo2, ((size_t)nu + 1) * 8));
    HIP_TRY(g.alloc(&d_lay2, (size_t)n * sizeof(sigax_placement)));
    HIP_TRY(g.alloc(&d_class, (size_t)n));
    HIP_TRY(g.alloc(&d_status, 16 * 8));
    HIP_TRY(g.alloc(&d_work, (size_t)wb));
    HIP_TRY(hipMemcpy(d_so, seq_offs, ((size_t)nu + 1) * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_lo, lay_offs, ((size_t)nu + 1) * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(d_lay, 0xFF, (size_t)n * sizeof(sigax_placement)));  // (what lies behind the placements names no read)
    if (placed) HIP_TRY(hipMemcpy(d_lay, layout, (size_t)placed * sizeof(sigax_placement), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_len, lengths, (size_t)n * 4, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_cont, contained, (size_t)n, hipMemcpyHostToDevice));
    if (n_conts) HIP_TRY(hipMemcpy(d_recs, conts, (size_t)n_conts * sizeof(sigax_mm_edge), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy((u64*)d_status + 8, &nu, 8, hipMemcpyHostToDevice));  // the count the device reads: behind the 8 status words
    const int rc = sigax_contained_place_device(device, (u64*)d_status + 8, nu, d_so, d_lo, (const sigax_placement*)d_lay, d_len, n, d_cont,
                                                (const sigax_mm_edge*)d_recs, n_conts, opts, d_lo2, (sigax_placement*)d_lay2, d_class, d_status, d_work,
                                                wb, nullptr);
    if (rc != SIGAX_OK) return rc;
    HIP_TRY(hipMemcpy(status8, d_status, 8 * 8, hipMemcpyDeviceToHost));  // (waits for the null stream's kernels)
    HIP_TRY(hipMemcpy(h_lo2, d_lo2, ((size_t)nu + 1) * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(h_lay2, d_lay2, (size_t)n * sizeof(sigax_placement), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(h_class, d_class, (size_t)n, hipMemcpyDeviceToHost));
  }
  *lay_offs2 = h_lo2;
  *layout2 = h_lay2;
  *place_class = h_class;
  hg.release();
  return SIGAX_OK;
}
