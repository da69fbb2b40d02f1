// siga_amd/csrc/sigax_unitig.cpp -- `siga unitig` on the device: the entry points of sigax_unitig.hip.
#include <cstring>

#include "sigax_internal.h"

static_assert(sizeof(sigax_placement) == 16, "sigax_placement must be 16 bytes");

namespace {

// where the pieces of the caller's scratch lie (every piece 16-byte aligned)
struct UnitigWork {
  u64 rank[2], dist[2], link, dst, src, scan, partial, scan_total, counts, deg, closing, cnt, bytes;
  u64 zero_from, zero_bytes;  // deg, closing and counts lie together: one memset
};
UnitigWork unitig_work(u64 n) {
  UnitigWork w;
  u64 at = 0;
  auto take = [&](u64 bytes) {
    const u64 here = at;
    at += (bytes + 15) & ~15ull;
    return here;
  };
  for (int k = 0; k < 2; ++k) w.rank[k] = take(2 * n * 16);
  for (int k = 0; k < 2; ++k) w.dist[k] = take(2 * n * 8);
  w.link = take(2 * n * 8);
  w.dst = take((n + 1) * 8);
  w.src = take(n * 8);
  w.scan = take(4 * (n + 1) * 8);
  w.partial = take(scan_partials_needed(n) * 8);
  w.scan_total = take(8);
  w.zero_from = at;
  w.counts = take(4 * 8);
  w.deg = take(2 * n * 4);
  w.closing = take(n * 4);
  w.zero_bytes = at - w.zero_from;
  w.cnt = take(4 * (n + 1) * 4);
  w.bytes = at;
  return w;
}

UnitigArgs unitig_args(const sigax_edge* d_edges, u64 n_edges, const void* d_lengths, const void* d_seqs, const void* d_offs, u64 n,
                       uint32_t min_overlap, void* d_seq_offs, void* d_lay_offs, void* d_uflags, sigax_placement* d_layout, void* d_useqs,
                       void* d_status6, void* d_work) {
  const UnitigWork w = unitig_work(n);
  char* base = (char*)d_work;
  UnitigArgs a;
  a.edges = d_edges;
  a.n_edges = n_edges;
  a.n_reads = n;
  a.lengths = (const uint32_t*)d_lengths;
  a.seqs = (const unsigned char*)d_seqs;
  a.offs = (const u64*)d_offs;
  a.min_overlap = min_overlap;
  a.seq_offs = (u64*)d_seq_offs;
  a.lay_offs = (u64*)d_lay_offs;
  a.uflags = (uint32_t*)d_uflags;
  a.layout = d_layout;
  a.useqs = (unsigned char*)d_useqs;
  a.status = (u64*)d_status6;
  a.deg = (uint32_t*)(base + w.deg);
  a.link = (uint2*)(base + w.link);
  for (int k = 0; k < 2; ++k) {
    a.rank[k] = base + w.rank[k];
    a.dist[k] = (u64*)(base + w.dist[k]);
  }
  a.closing = (uint32_t*)(base + w.closing);
  a.cnt = (uint32_t*)(base + w.cnt);
  a.scan = (u64*)(base + w.scan);
  a.partial = (u64*)(base + w.partial);
  a.scan_total = (u64*)(base + w.scan_total);
  a.dst = (u64*)(base + w.dst);
  a.src = (u64*)(base + w.src);
  a.counts = (u64*)(base + w.counts);
  return a;
}

// the trim calls' scratch: the unitig call's, then what the rounds and the lifted records need
struct TrimWork {
  UnitigWork u;
  u64 trim, verdict, umap, eflag, escan, epartial, bytes;
};
TrimWork trim_work(u64 n, u64 n_edges, bool graph) {
  TrimWork w;
  w.u = unitig_work(n);
  u64 at = w.u.bytes;
  auto take = [&](u64 bytes) {
    const u64 here = at;
    at += (bytes + 15) & ~15ull;
    return here;
  };
  w.trim = take(TRIM_WORDS * 8);
  w.verdict = take(n * 4);
  w.umap = take(n * 4);
  w.eflag = w.escan = w.epartial = at;
  if (graph) {
    w.eflag = take(n_edges * 4);
    w.escan = take((n_edges + 1) * 8);
    w.epartial = take(scan_partials_needed(n_edges) * 8);
  }
  w.bytes = at;
  return w;
}

// the prune calls' scratch: the trim calls', then what a round's cut step needs
struct PruneWork {
  TrimWork t;
  u64 prune, maxlen, uniq, maxself, keys, key_cap, bytes;
};
PruneWork prune_work(u64 n, u64 n_edges, bool graph, bool careful) {
  PruneWork w;
  w.t = trim_work(n, n_edges, graph);
  u64 at = w.t.bytes;
  auto take = [&](u64 bytes) {
    const u64 here = at;
    at += (bytes + 15) & ~15ull;
    return here;
  };
  w.prune = take(PRUNE_WORDS * 8);
  w.maxlen = take(2 * n * 4);
  w.uniq = take(n * 4);
  w.maxself = w.keys = at;
  w.key_cap = 0;
  if (careful) {
    w.maxself = take(2 * n * 4);
    w.key_cap = 16;
    while (w.key_cap < 4 * n_edges) w.key_cap <<= 1;
    w.keys = take(w.key_cap * 8);
  }
  w.bytes = at;
  return w;
}

// the chimeric calls' scratch: the prune calls', then what a round's chimeric step needs
struct ChimericWork {
  PruneWork p;
  u64 chim, aside, nbr, minb[2], mink[2], bytes;
};
ChimericWork chimeric_work(u64 n, u64 n_edges, bool graph, bool careful) {
  ChimericWork w;
  w.p = prune_work(n, n_edges, graph, careful);
  u64 at = w.p.bytes;
  auto take = [&](u64 bytes) {
    const u64 here = at;
    at += (bytes + 15) & ~15ull;
    return here;
  };
  w.chim = take(CHIM_WORDS * 8);
  w.aside = take(PRUNE_WORDS * 8);
  w.nbr = take(2 * n * 4);
  for (int k = 0; k < 2; ++k) w.minb[k] = take(2 * n * 8);
  for (int k = 0; k < 2; ++k) w.mink[k] = take(2 * n * 8);
  w.bytes = at;
  return w;
}

// the bubble calls' scratch: the chimeric calls', then what a round's bubble step needs
struct BubbleWork {
  ChimericWork c;
  u64 bub, bnbr, blen, arm, where, aside, gslot, losers, table, best, group_cap, bytes;
};
BubbleWork bubble_work(u64 n, u64 n_edges, bool graph, bool careful) {
  BubbleWork w;
  w.c = chimeric_work(n, n_edges, graph, careful);
  u64 at = w.c.bytes;
  auto take = [&](u64 bytes) {
    const u64 here = at;
    at += (bytes + 15) & ~15ull;
    return here;
  };
  w.bub = take(BUB_WORDS * 8);
  w.bnbr = take(2 * n * 4);
  w.blen = take(2 * n * 4);
  w.arm = take(n * 16);
  w.where = take(n * 16);
  w.aside = take(n * 4);
  w.gslot = take(n * 4);
  w.losers = take(n * 4);
  w.group_cap = 16;
  while (w.group_cap < 2 * n) w.group_cap <<= 1;
  w.table = take(w.group_cap * 4);
  w.best = take(w.group_cap * 8);
  w.bytes = at;
  return w;
}

int unitig_limits(u64 n_reads, u64 n_edges) {
  if (n_reads >= (1ull << 31)) return sigax_fail(SIGAX_E_ARG, "2^31 reads or more: a state names a read end in 32 bits");
  if (n_edges > (1ull << 32)) return sigax_fail(SIGAX_E_ARG, "more than 2^32 records");
  return SIGAX_OK;
}

thread_local u64 t_last_status[6] = {0, 0, 0, 0, 0, 0};

int trim_opts_ok(const sigax_trim_opts* o) {
  if (!o) return sigax_fail(SIGAX_E_ARG, "NULL where the trim options are required");
  if (o->reserved != 0) return sigax_fail(SIGAX_E_ARG, "sigax_trim_opts.reserved must be 0");
  if (o->max_rounds > TRIM_MAX_ROUNDS) return sigax_fail(SIGAX_E_ARG, "max_rounds %u: at most %d", o->max_rounds, (int)TRIM_MAX_ROUNDS);
  return SIGAX_OK;
}

int prune_opts_ok(const sigax_prune_opts* o, u64 n_reads) {
  if (!o) return sigax_fail(SIGAX_E_ARG, "NULL where the prune options are required");
  if (o->reserved != 0) return sigax_fail(SIGAX_E_ARG, "sigax_prune_opts.reserved must be 0");
  if (o->careful > 1) return sigax_fail(SIGAX_E_ARG, "careful %u: 0 or 1", o->careful);
  if (o->max_rounds > TRIM_MAX_ROUNDS) return sigax_fail(SIGAX_E_ARG, "max_rounds %u: at most %d", o->max_rounds, (int)TRIM_MAX_ROUNDS);
  if (o->num_reads < n_reads) return sigax_fail(SIGAX_E_ARG, "num_reads %llu below the %llu reads given", (u64)o->num_reads, n_reads);
  if (o->delta > 0 && o->genome_size == 0) return sigax_fail(SIGAX_E_ARG, "genome_size must be given with delta > 0");
  return SIGAX_OK;
}

int chimeric_opts_ok(const sigax_chimeric_opts* o, u64 n_reads) {
  if (!o) return sigax_fail(SIGAX_E_ARG, "NULL where the chimeric options are required");
  const int rc = prune_opts_ok(&o->prune, n_reads);
  if (rc != SIGAX_OK) return rc;
  if (o->reserved2 != 0) return sigax_fail(SIGAX_E_ARG, "sigax_chimeric_opts.reserved2 must be 0");
  if (o->min_chimeric_length > 0 && o->prune.genome_size == 0)
    return sigax_fail(SIGAX_E_ARG, "genome_size must be given with min_chimeric_length > 0");
  return SIGAX_OK;
}

// the chimeric call's refusals with Lc = 0 where the bubble step alone runs: it needs neither G nor N
int bubble_opts_ok(const sigax_bubble_opts* o, u64 n_reads) {
  if (!o) return sigax_fail(SIGAX_E_ARG, "NULL where the bubble options are required");
  const int rc = chimeric_opts_ok(&o->chimeric, n_reads);
  if (rc != SIGAX_OK) return rc;
  if (o->reserved3[0] != 0 || o->reserved3[1] != 0) return sigax_fail(SIGAX_E_ARG, "sigax_bubble_opts.reserved3 must be 0");
  return SIGAX_OK;
}

}  // namespace

extern "C" int sigax_unitigs_workspace(uint64_t n_reads, uint64_t n_edges, uint64_t* bytes) {
  if (!bytes) return sigax_fail(SIGAX_E_ARG, "bad argument");
  const int rc = unitig_limits(n_reads, n_edges);
  if (rc != SIGAX_OK) return rc;
  *bytes = unitig_work(n_reads).bytes;
  return SIGAX_OK;
}

extern "C" int sigax_unitigs_device(int device, const sigax_edge* d_edges, uint64_t n_edges, const void* d_lengths, const void* d_seqs,
                                    const void* d_offs, uint64_t n_reads, uint32_t min_overlap, void* d_seq_offs, void* d_lay_offs,
                                    void* d_uflags, sigax_placement* d_layout, void* d_useqs, void* d_status6, void* d_work,
                                    uint64_t work_bytes, void* stream) {
  const int rl = unitig_limits(n_reads, n_edges);
  if (rl != SIGAX_OK) return rl;
  if (n_reads && (!d_lengths || !d_seqs || !d_offs || !d_seq_offs || !d_lay_offs || !d_uflags || !d_layout || !d_status6 || !d_work ||
                  (n_edges && !d_edges)))
    return sigax_fail(SIGAX_E_ARG, "NULL where a buffer is required");
  if (n_reads && (((uintptr_t)d_edges | (uintptr_t)d_layout | (uintptr_t)d_useqs | (uintptr_t)d_work) & 15))
    return sigax_fail(SIGAX_E_ARG, "d_edges, d_layout, d_useqs and d_work must be 16-byte aligned");
  if (n_reads && (((uintptr_t)d_offs | (uintptr_t)d_seq_offs | (uintptr_t)d_lay_offs | (uintptr_t)d_status6) & 7))
    return sigax_fail(SIGAX_E_ARG, "d_offs, d_seq_offs, d_lay_offs and d_status6 must be 8-byte aligned");
  const UnitigWork w = unitig_work(n_reads);
  if (n_reads && work_bytes < w.bytes)
    return sigax_fail(SIGAX_E_ARG, "workspace of %llu bytes, %llu needed (sigax_unitigs_workspace)", (u64)work_bytes, w.bytes);
  HIP_TRY(hipSetDevice(device));
  const hipStream_t st = (hipStream_t)stream;
  if (n_reads == 0) {
    if (d_status6) HIP_TRY(hipMemsetAsync(d_status6, 0, 48, st));
    return SIGAX_OK;
  }
  const UnitigArgs a = unitig_args(d_edges, n_edges, d_lengths, d_seqs, d_offs, n_reads, min_overlap, d_seq_offs, d_lay_offs, d_uflags,
                                   d_layout, d_useqs, d_status6, d_work);
  char* base = (char*)d_work;
  HIP_TRY(hipMemsetAsync(base + w.zero_from, 0, (size_t)w.zero_bytes, st));
  HIP_TRY(hipMemsetAsync(a.link, 0xFF, (size_t)n_reads * 16, st));
  launch_unitigs(a, st);
  HIP_TRY(hipGetLastError());
  return SIGAX_OK;
}

extern "C" int sigax_unitigs_bases_device(int device, const void* d_seqs, const void* d_offs, uint64_t n_reads, uint64_t n_edges,
                                          void* d_useqs, void* d_work, uint64_t work_bytes, void* stream) {
  const int rl = unitig_limits(n_reads, n_edges);
  if (rl != SIGAX_OK) return rl;
  if (n_reads && (!d_seqs || !d_offs || !d_useqs || !d_work)) return sigax_fail(SIGAX_E_ARG, "NULL where a buffer is required");
  if (n_reads && ((((uintptr_t)d_useqs | (uintptr_t)d_work) & 15) || ((uintptr_t)d_offs & 7)))
    return sigax_fail(SIGAX_E_ARG, "d_useqs and d_work must be 16-byte aligned, d_offs 8-byte aligned");
  if (n_reads && work_bytes < unitig_work(n_reads).bytes) return sigax_fail(SIGAX_E_ARG, "workspace too small (sigax_unitigs_workspace)");
  HIP_TRY(hipSetDevice(device));
  if (n_reads == 0) return SIGAX_OK;
  const UnitigArgs a = unitig_args(nullptr, n_edges, nullptr, d_seqs, d_offs, n_reads, 0, nullptr, nullptr, nullptr, nullptr, d_useqs, nullptr, d_work);
  launch_unitig_bases(a, (hipStream_t)stream);
  HIP_TRY(hipGetLastError());
  return SIGAX_OK;
}

extern "C" int sigax_unitigs_last_status(uint64_t status6[6]) {
  if (!status6) return sigax_fail(SIGAX_E_ARG, "bad argument");
  for (int k = 0; k < 6; ++k) status6[k] = t_last_status[k];
  return SIGAX_OK;
}

extern "C" int sigax_unitigs_host(int device, const sigax_edge* edges, uint64_t n_edges, const uint32_t* lengths, const char* seqs,
                                  const uint64_t* offs, uint64_t n_reads, uint32_t min_overlap, uint64_t* n_unitigs, uint64_t** seq_offs,
                                  uint64_t** lay_offs, uint32_t** uflags, sigax_placement** layout, char** useqs) {
  if (!n_unitigs || !seq_offs || !lay_offs || !uflags || !layout || (n_reads && (!lengths || !seqs || !offs)) || (n_edges && !edges))
    return sigax_fail(SIGAX_E_ARG, "NULL where a buffer is required");
  *n_unitigs = 0;
  *seq_offs = nullptr;
  *lay_offs = nullptr;
  *uflags = nullptr;
  *layout = nullptr;
  if (useqs) *useqs = nullptr;
  const int rl = unitig_limits(n_reads, n_edges);
  if (rl != SIGAX_OK) return rl;
  const u64 n = n_reads;
  for (u64 i = 0; i < n; ++i)
    if (offs[i + 1] < offs[i] || offs[i + 1] - offs[i] != lengths[i]) return sigax_fail(SIGAX_E_ARG, "read %llu: offsets and length disagree", i);
  // offs[0] need not be 0 (a window of a longer table): the device gets the window's bytes and offsets from 0
  const u64 b0 = n ? offs[0] : 0, nb = n ? offs[n] - b0 : 0;
  std::vector<uint64_t> rebased;
  if (b0) {
    rebased.resize((size_t)n + 1);
    for (u64 i = 0; i <= n; ++i) rebased[i] = offs[i] - b0;
    offs = rebased.data();
  }
  u64 status[6] = {0, 0, 0, 0, 0, 0};
  DevGuard g;
  void *d_edges = nullptr, *d_lengths = nullptr, *d_seqs = nullptr, *d_offs = nullptr, *d_so = nullptr, *d_lo = nullptr, *d_uf = nullptr,
       *d_lay = nullptr, *d_us = nullptr, *d_status = nullptr, *d_work = nullptr;
  if (n) {
    HIP_TRY(hipSetDevice(device));
    const u64 wb = unitig_work(n).bytes;
    HIP_TRY(g.alloc(&d_edges, (size_t)n_edges * sizeof(sigax_edge)));
    HIP_TRY(g.alloc(&d_lengths, (size_t)n * 4));
    HIP_TRY(g.alloc(&d_seqs, (size_t)nb + 16));
    HIP_TRY(g.alloc(&d_offs, ((size_t)n + 1) * 8));
    HIP_TRY(g.alloc(&d_so, ((size_t)n + 1) * 8));
    HIP_TRY(g.alloc(&d_lo, ((size_t)n + 1) * 8));
    HIP_TRY(g.alloc(&d_uf, (size_t)n * 4));
    HIP_TRY(g.alloc(&d_lay, (size_t)n * sizeof(sigax_placement)));
    if (useqs) HIP_TRY(g.alloc(&d_us, (size_t)nb + 16));
    HIP_TRY(g.alloc(&d_status, 48));
    HIP_TRY(g.alloc(&d_work, (size_t)wb));
    if (n_edges) HIP_TRY(hipMemcpy(d_edges, edges, (size_t)n_edges * sizeof(sigax_edge), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_lengths, lengths, (size_t)n * 4, hipMemcpyHostToDevice));
    if (nb) HIP_TRY(hipMemcpy(d_seqs, seqs + b0, (size_t)nb, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_offs, offs, ((size_t)n + 1) * 8, hipMemcpyHostToDevice));
    const int rc = sigax_unitigs_device(device, (const sigax_edge*)d_edges, n_edges, d_lengths, d_seqs, d_offs, n, min_overlap, d_so, d_lo, d_uf,
                                        (sigax_placement*)d_lay, d_us, d_status, d_work, wb, nullptr);
    if (rc != SIGAX_OK) return rc;
    HIP_TRY(hipMemcpy(status, d_status, 48, hipMemcpyDeviceToHost));  // (waits for the null stream's kernels)
    if (status[0] > n || status[1] > nb) return sigax_fail(SIGAX_E_DEVICE, "unitig counts beyond their buffers");
  }
  const u64 nu = status[0], bases = status[1];
  uint64_t* h_so = (uint64_t*)malloc(((size_t)nu + 1) * 8);
  uint64_t* h_lo = (uint64_t*)malloc(((size_t)nu + 1) * 8);
  uint32_t* h_uf = (uint32_t*)malloc(nu ? (size_t)nu * 4 : 4);
  sigax_placement* h_lay = (sigax_placement*)malloc(n ? (size_t)n * sizeof(sigax_placement) : sizeof(sigax_placement));
  char* h_us = useqs ? (char*)malloc(bases ? (size_t)bases : 1) : nullptr;
  auto drop = [&] {
    free(h_so);
    free(h_lo);
    free(h_uf);
    free(h_lay);
    free(h_us);
  };
  if (!h_so || !h_lo || !h_uf || !h_lay || (useqs && !h_us)) {
    drop();
    return sigax_fail(SIGAX_E_CAPACITY, "out of host memory");
  }
  h_so[0] = 0;
  h_lo[0] = 0;
  hipError_t e = hipSuccess;
  if (n) {
    e = hipMemcpy(h_so, d_so, ((size_t)nu + 1) * 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(h_lo, d_lo, ((size_t)nu + 1) * 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess && nu) e = hipMemcpy(h_uf, d_uf, (size_t)nu * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(h_lay, d_lay, (size_t)n * sizeof(sigax_placement), hipMemcpyDeviceToHost);
    if (e == hipSuccess && useqs && bases) e = hipMemcpy(h_us, d_us, (size_t)bases, hipMemcpyDeviceToHost);
  }
  if (e != hipSuccess) {
    drop();
    return sigax_fail(SIGAX_E_DEVICE, "copying the unitigs: %s", hipGetErrorString(e));
  }
  for (int k = 0; k < 6; ++k) t_last_status[k] = status[k];
  *n_unitigs = nu;
  *seq_offs = h_so;
  *lay_offs = h_lo;
  *uflags = h_uf;
  *layout = h_lay;
  if (useqs) *useqs = h_us;
  return SIGAX_OK;
}

// ---- tip trimming and the lifted records ----
extern "C" int sigax_unitigs_trim_workspace(uint64_t n_reads, uint64_t n_edges, int want_graph, uint64_t* bytes) {
  if (!bytes) return sigax_fail(SIGAX_E_ARG, "bad argument");
  const int rc = unitig_limits(n_reads, n_edges);
  if (rc != SIGAX_OK) return rc;
  *bytes = trim_work(n_reads, n_edges, want_graph != 0).bytes;
  return SIGAX_OK;
}

// paced: the host form's loop -- it reads each round's flag and stops after the first round that removed nothing, where the
// device form enqueues every round and lets the idle ones leave at once
static int unitigs_trim_run(int device, const sigax_edge* d_edges, uint64_t n_edges, const void* d_lengths, const void* d_seqs,
                            const void* d_offs, uint64_t n_reads, uint32_t min_overlap, const sigax_trim_opts* opts, void* d_seq_offs,
                            void* d_lay_offs, void* d_uflags, sigax_placement* d_layout, void* d_useqs, void* d_removed, sigax_edge* d_uedges,
                            void* d_status12, void* d_work, uint64_t work_bytes, void* stream, bool paced) {
  const int rl = unitig_limits(n_reads, n_edges);
  if (rl != SIGAX_OK) return rl;
  const int ro = trim_opts_ok(opts);
  if (ro != SIGAX_OK) return ro;
  if (n_reads && (!d_lengths || !d_seqs || !d_offs || !d_seq_offs || !d_lay_offs || !d_uflags || !d_layout || !d_removed || !d_status12 ||
                  !d_work || (n_edges && !d_edges)))
    return sigax_fail(SIGAX_E_ARG, "NULL where a buffer is required");
  if (n_reads && (((uintptr_t)d_edges | (uintptr_t)d_layout | (uintptr_t)d_useqs | (uintptr_t)d_uedges | (uintptr_t)d_work) & 15))
    return sigax_fail(SIGAX_E_ARG, "d_edges, d_layout, d_useqs, d_uedges and d_work must be 16-byte aligned");
  if (n_reads && (((uintptr_t)d_offs | (uintptr_t)d_seq_offs | (uintptr_t)d_lay_offs | (uintptr_t)d_status12) & 7))
    return sigax_fail(SIGAX_E_ARG, "d_offs, d_seq_offs, d_lay_offs and d_status12 must be 8-byte aligned");
  if (n_reads && ((uintptr_t)d_removed & 3)) return sigax_fail(SIGAX_E_ARG, "d_removed must be 4-byte aligned");
  const TrimWork w = trim_work(n_reads, n_edges, d_uedges != nullptr);
  if (n_reads && work_bytes < w.bytes)
    return sigax_fail(SIGAX_E_ARG, "workspace of %llu bytes, %llu needed (sigax_unitigs_trim_workspace)", (u64)work_bytes, w.bytes);
  HIP_TRY(hipSetDevice(device));
  const hipStream_t st = (hipStream_t)stream;
  if (n_reads == 0) {
    if (d_status12) HIP_TRY(hipMemsetAsync(d_status12, 0, 96, st));
    return SIGAX_OK;
  }
  UnitigTrimArgs a;
  static_cast<UnitigArgs&>(a) = unitig_args(d_edges, n_edges, d_lengths, d_seqs, d_offs, n_reads, min_overlap, d_seq_offs, d_lay_offs, d_uflags,
                                            d_layout, d_useqs, d_status12, d_work);
  char* base = (char*)d_work;
  a.removed = (uint32_t*)d_removed;
  a.trim = (u64*)(base + w.trim);
  a.verdict = (uint32_t*)(base + w.verdict);
  a.umap = (uint32_t*)(base + w.umap);
  a.round = 0;
  a.min_branch_length = opts->min_branch_length;
  a.min_branch_coverage = opts->min_branch_coverage;
  a.uedges = d_uedges;
  a.eflag = (uint32_t*)(base + w.eflag);
  a.escan = (u64*)(base + w.escan);
  a.epartial = (u64*)(base + w.epartial);
  HIP_TRY(hipMemsetAsync(d_removed, 0, (size_t)n_reads * 4, st));
  HIP_TRY(hipMemsetAsync(a.trim, 0, TRIM_WORDS * 8, st));
  auto reset = [&]() -> hipError_t {  // every pass over degrees, links and counts of its own
    const hipError_t e = hipMemsetAsync(base + w.u.zero_from, 0, (size_t)w.u.zero_bytes, st);
    return e != hipSuccess ? e : hipMemsetAsync(a.link, 0xFF, (size_t)n_reads * 16, st);
  };
  for (uint32_t r = 1; r <= opts->max_rounds; ++r) {
    a.round = r;
    HIP_TRY(reset());
    launch_trim_round(a, st);
    if (paced) {
      u64 flag = 0;
      HIP_TRY(hipMemcpyAsync(&flag, a.trim + TRIM_ROUND0 + r, 8, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      if (flag == 0) break;
    }
  }
  a.round = 0;  // the unitigs of what is left
  HIP_TRY(reset());
  launch_unitigs_trim(a, st);
  launch_unitig_lift(a, st);
  HIP_TRY(hipGetLastError());
  return SIGAX_OK;
}

extern "C" int sigax_unitigs_trim_device(int device, const sigax_edge* d_edges, uint64_t n_edges, const void* d_lengths, const void* d_seqs,
                                         const void* d_offs, uint64_t n_reads, uint32_t min_overlap, const sigax_trim_opts* opts,
                                         void* d_seq_offs, void* d_lay_offs, void* d_uflags, sigax_placement* d_layout, void* d_useqs,
                                         void* d_removed, sigax_edge* d_uedges, void* d_status12, void* d_work, uint64_t work_bytes,
                                         void* stream) {
  return unitigs_trim_run(device, d_edges, n_edges, d_lengths, d_seqs, d_offs, n_reads, min_overlap, opts, d_seq_offs, d_lay_offs, d_uflags,
                          d_layout, d_useqs, d_removed, d_uedges, d_status12, d_work, work_bytes, stream, false);
}

static int unitigs_prune_run(int device, const sigax_edge* d_edges, uint64_t n_edges, const void* d_lengths, const void* d_seqs,
                             const void* d_offs, uint64_t n_reads, uint32_t min_overlap, const sigax_prune_opts* opts, void* d_seq_offs,
                             void* d_lay_offs, void* d_uflags, sigax_placement* d_layout, void* d_useqs, void* d_removed, void* d_cut,
                             sigax_edge* d_uedges, void* d_status16, void* d_work, uint64_t work_bytes, void* stream, bool paced);
static int unitigs_chimeric_run(int device, const sigax_edge* d_edges, uint64_t n_edges, const void* d_lengths, const void* d_seqs,
                                const void* d_offs, uint64_t n_reads, uint32_t min_overlap, const sigax_chimeric_opts* opts, void* d_seq_offs,
                                void* d_lay_offs, void* d_uflags, sigax_placement* d_layout, void* d_useqs, void* d_removed, void* d_cut,
                                sigax_edge* d_uedges, void* d_status20, void* d_work, uint64_t work_bytes, void* stream, bool paced);

static int unitigs_bubble_run(int device, const sigax_edge* d_edges, uint64_t n_edges, const void* d_lengths, const void* d_seqs,
                              const void* d_offs, uint64_t n_reads, uint32_t min_overlap, const sigax_bubble_opts* opts, void* d_seq_offs,
                              void* d_lay_offs, void* d_uflags, sigax_placement* d_layout, void* d_useqs, void* d_removed, void* d_cut,
                              sigax_edge* d_uedges, void* d_status24, void* d_work, uint64_t work_bytes, void* stream, bool paced);

// The host form of the four calls.  The bubble call passes bopts, &bopts->chimeric for copts, its prune for popts, and cut; `status`
// then holds 24.  The trim call passes opts, and NULL for popts, copts and cut; `status` then holds 12 counts.  The
// prune call passes popts and cut, and NULL for opts and copts; `status` then holds 16.  The chimeric call passes copts, &copts->prune
// for popts, and cut; `status` then holds 20.
static int unitigs_rounds_host(int device, const sigax_edge* edges, uint64_t n_edges, const uint32_t* lengths, const char* seqs,
                               const uint64_t* offs, uint64_t n_reads, uint32_t min_overlap, const sigax_trim_opts* opts,
                               const sigax_prune_opts* popts, const sigax_chimeric_opts* copts, const sigax_bubble_opts* bopts,
                               uint64_t* n_unitigs, uint64_t** seq_offs,
                               uint64_t** lay_offs, uint32_t** uflags, sigax_placement** layout, char** useqs, uint32_t** removed,
                               uint32_t** cut, sigax_edge** uedges, uint64_t* status_out) {
  const int n_status = bopts ? 24 : copts ? 20 : popts ? 16 : 12;
  if (!n_unitigs || !seq_offs || !lay_offs || !uflags || !layout || !removed || !status_out || (popts && !cut) ||
      (n_reads && (!lengths || !seqs || !offs)) || (n_edges && !edges))
    return sigax_fail(SIGAX_E_ARG, "NULL where a buffer is required");
  if (cut) *cut = nullptr;
  *n_unitigs = 0;
  *seq_offs = nullptr;
  *lay_offs = nullptr;
  *uflags = nullptr;
  *layout = nullptr;
  *removed = nullptr;
  if (useqs) *useqs = nullptr;
  if (uedges) *uedges = nullptr;
  for (int k = 0; k < n_status; ++k) status_out[k] = 0;
  const int rl = unitig_limits(n_reads, n_edges);
  if (rl != SIGAX_OK) return rl;
  const int ro = bopts ? bubble_opts_ok(bopts, n_reads) : copts ? chimeric_opts_ok(copts, n_reads) : popts ? prune_opts_ok(popts, n_reads) : trim_opts_ok(opts);
  if (ro != SIGAX_OK) return ro;
  const u64 n = n_reads;
  for (u64 i = 0; i < n; ++i)
    if (offs[i + 1] < offs[i] || offs[i + 1] - offs[i] != lengths[i]) return sigax_fail(SIGAX_E_ARG, "read %llu: offsets and length disagree", i);
  const u64 b0 = n ? offs[0] : 0, nb = n ? offs[n] - b0 : 0;
  std::vector<uint64_t> rebased;
  if (b0) {
    rebased.resize((size_t)n + 1);
    for (u64 i = 0; i <= n; ++i) rebased[i] = offs[i] - b0;
    offs = rebased.data();
  }
  u64 status[24] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  DevGuard g;
  void *d_edges = nullptr, *d_lengths = nullptr, *d_seqs = nullptr, *d_offs = nullptr, *d_so = nullptr, *d_lo = nullptr, *d_uf = nullptr,
       *d_lay = nullptr, *d_us = nullptr, *d_rm = nullptr, *d_ct = nullptr, *d_ue = nullptr, *d_status = nullptr, *d_work = nullptr;
  if (n) {
    HIP_TRY(hipSetDevice(device));
    const u64 wb = bopts   ? bubble_work(n, n_edges, uedges != nullptr, popts->careful != 0).bytes
                   : copts ? chimeric_work(n, n_edges, uedges != nullptr, popts->careful != 0).bytes
                   : popts ? prune_work(n, n_edges, uedges != nullptr, popts->careful != 0).bytes
                           : trim_work(n, n_edges, uedges != nullptr).bytes;
    if (popts) HIP_TRY(g.alloc(&d_ct, (size_t)n_edges * 4 + 16));
    HIP_TRY(g.alloc(&d_edges, (size_t)n_edges * sizeof(sigax_edge)));
    HIP_TRY(g.alloc(&d_lengths, (size_t)n * 4));
    HIP_TRY(g.alloc(&d_seqs, (size_t)nb + 16));
    HIP_TRY(g.alloc(&d_offs, ((size_t)n + 1) * 8));
    HIP_TRY(g.alloc(&d_so, ((size_t)n + 1) * 8));
    HIP_TRY(g.alloc(&d_lo, ((size_t)n + 1) * 8));
    HIP_TRY(g.alloc(&d_uf, (size_t)n * 4));
    HIP_TRY(g.alloc(&d_lay, (size_t)n * sizeof(sigax_placement)));
    if (useqs) HIP_TRY(g.alloc(&d_us, (size_t)nb + 16));
    HIP_TRY(g.alloc(&d_rm, (size_t)n * 4));
    if (uedges) HIP_TRY(g.alloc(&d_ue, (size_t)n_edges * sizeof(sigax_edge) + 16));
    HIP_TRY(g.alloc(&d_status, (size_t)n_status * 8));
    HIP_TRY(g.alloc(&d_work, (size_t)wb));
    if (n_edges) HIP_TRY(hipMemcpy(d_edges, edges, (size_t)n_edges * sizeof(sigax_edge), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_lengths, lengths, (size_t)n * 4, hipMemcpyHostToDevice));
    if (nb) HIP_TRY(hipMemcpy(d_seqs, seqs + b0, (size_t)nb, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(d_offs, offs, ((size_t)n + 1) * 8, hipMemcpyHostToDevice));
    const int rc = bopts ? unitigs_bubble_run(device, (const sigax_edge*)d_edges, n_edges, d_lengths, d_seqs, d_offs, n, min_overlap, bopts, d_so,
                                              d_lo, d_uf, (sigax_placement*)d_lay, d_us, d_rm, d_ct, (sigax_edge*)d_ue, d_status, d_work, wb,
                                              nullptr, true)
                   : copts ? unitigs_chimeric_run(device, (const sigax_edge*)d_edges, n_edges, d_lengths, d_seqs, d_offs, n, min_overlap, copts, d_so,
                                                d_lo, d_uf, (sigax_placement*)d_lay, d_us, d_rm, d_ct, (sigax_edge*)d_ue, d_status, d_work, wb,
                                                nullptr, true)
                   : popts ? unitigs_prune_run(device, (const sigax_edge*)d_edges, n_edges, d_lengths, d_seqs, d_offs, n, min_overlap, popts, d_so,
                                             d_lo, d_uf, (sigax_placement*)d_lay, d_us, d_rm, d_ct, (sigax_edge*)d_ue, d_status, d_work, wb,
                                             nullptr, true)
                         : unitigs_trim_run(device, (const sigax_edge*)d_edges, n_edges, d_lengths, d_seqs, d_offs, n, min_overlap, opts, d_so, d_lo,
                                            d_uf, (sigax_placement*)d_lay, d_us, d_rm, (sigax_edge*)d_ue, d_status, d_work, wb, nullptr, true);
    if (rc != SIGAX_OK) return rc;
    HIP_TRY(hipMemcpy(status, d_status, (size_t)n_status * 8, hipMemcpyDeviceToHost));  // (waits for the null stream's kernels)
    if (status[0] > n || status[1] > nb || status[9] > n || status[11] > n_edges)
      return sigax_fail(SIGAX_E_DEVICE, "unitig counts beyond their buffers");
  }
  const u64 nu = status[0], bases = status[1], placed = n - status[9], ne = uedges ? status[11] : 0;
  uint64_t* h_so = (uint64_t*)malloc(((size_t)nu + 1) * 8);
  uint64_t* h_lo = (uint64_t*)malloc(((size_t)nu + 1) * 8);
  uint32_t* h_uf = (uint32_t*)malloc(nu ? (size_t)nu * 4 : 4);
  sigax_placement* h_lay = (sigax_placement*)malloc(placed ? (size_t)placed * sizeof(sigax_placement) : sizeof(sigax_placement));
  char* h_us = useqs ? (char*)malloc(bases ? (size_t)bases : 1) : nullptr;
  uint32_t* h_rm = (uint32_t*)malloc(n ? (size_t)n * 4 : 4);
  uint32_t* h_ct = cut ? (uint32_t*)malloc(n_edges ? (size_t)n_edges * 4 : 4) : nullptr;
  sigax_edge* h_ue = uedges ? (sigax_edge*)malloc(ne ? (size_t)ne * sizeof(sigax_edge) : sizeof(sigax_edge)) : nullptr;
  auto drop = [&] {
    free(h_so);
    free(h_lo);
    free(h_uf);
    free(h_lay);
    free(h_us);
    free(h_rm);
    free(h_ct);
    free(h_ue);
  };
  if (!h_so || !h_lo || !h_uf || !h_lay || !h_rm || (cut && !h_ct) || (useqs && !h_us) || (uedges && !h_ue)) {
    drop();
    return sigax_fail(SIGAX_E_CAPACITY, "out of host memory");
  }
  h_so[0] = 0;
  h_lo[0] = 0;
  hipError_t e = hipSuccess;
  if (n) {
    e = hipMemcpy(h_so, d_so, ((size_t)nu + 1) * 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(h_lo, d_lo, ((size_t)nu + 1) * 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess && nu) e = hipMemcpy(h_uf, d_uf, (size_t)nu * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess && placed) e = hipMemcpy(h_lay, d_lay, (size_t)placed * sizeof(sigax_placement), hipMemcpyDeviceToHost);
    if (e == hipSuccess && useqs && bases) e = hipMemcpy(h_us, d_us, (size_t)bases, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(h_rm, d_rm, (size_t)n * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess && cut && n_edges) e = hipMemcpy(h_ct, d_ct, (size_t)n_edges * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess && ne) e = hipMemcpy(h_ue, d_ue, (size_t)ne * sizeof(sigax_edge), hipMemcpyDeviceToHost);
  }
  if (e != hipSuccess) {
    drop();
    return sigax_fail(SIGAX_E_DEVICE, "copying the unitigs: %s", hipGetErrorString(e));
  }
  if (cut && n == 0 && n_edges) memset(h_ct, 0, (size_t)n_edges * 4);
  for (int k = 0; k < n_status; ++k) status_out[k] = status[k];
  if (cut) *cut = h_ct;
  *n_unitigs = nu;
  *seq_offs = h_so;
  *lay_offs = h_lo;
  *uflags = h_uf;
  *layout = h_lay;
  *removed = h_rm;
  if (useqs) *useqs = h_us;
  if (uedges) *uedges = h_ue;
  return SIGAX_OK;
}

extern "C" int sigax_unitigs_trim_host(int device, const sigax_edge* edges, uint64_t n_edges, const uint32_t* lengths, const char* seqs,
                                       const uint64_t* offs, uint64_t n_reads, uint32_t min_overlap, const sigax_trim_opts* opts,
                                       uint64_t* n_unitigs, uint64_t** seq_offs, uint64_t** lay_offs, uint32_t** uflags,
                                       sigax_placement** layout, char** useqs, uint32_t** removed, sigax_edge** uedges,
                                       uint64_t status12[12]) {
  return unitigs_rounds_host(device, edges, n_edges, lengths, seqs, offs, n_reads, min_overlap, opts, nullptr, nullptr, nullptr, n_unitigs,
                             seq_offs, lay_offs, uflags, layout, useqs, removed, nullptr, uedges, status12);
}

// ---- non-maximal overlap cutting ----
extern "C" int sigax_unitigs_prune_workspace(uint64_t n_reads, uint64_t n_edges, int want_graph, int careful, uint64_t* bytes) {
  if (!bytes) return sigax_fail(SIGAX_E_ARG, "bad argument");
  const int rc = unitig_limits(n_reads, n_edges);
  if (rc != SIGAX_OK) return rc;
  *bytes = prune_work(n_reads, n_edges, want_graph != 0, careful != 0).bytes;
  return SIGAX_OK;
}

static int unitigs_prune_run(int device, const sigax_edge* d_edges, uint64_t n_edges, const void* d_lengths, const void* d_seqs,
                             const void* d_offs, uint64_t n_reads, uint32_t min_overlap, const sigax_prune_opts* opts, void* d_seq_offs,
                             void* d_lay_offs, void* d_uflags, sigax_placement* d_layout, void* d_useqs, void* d_removed, void* d_cut,
                             sigax_edge* d_uedges, void* d_status16, void* d_work, uint64_t work_bytes, void* stream, bool paced) {
  const int rl = unitig_limits(n_reads, n_edges);
  if (rl != SIGAX_OK) return rl;
  const int ro = prune_opts_ok(opts, n_reads);
  if (ro != SIGAX_OK) return ro;
  if (n_reads && n_edges && !d_cut) return sigax_fail(SIGAX_E_ARG, "NULL where a buffer is required");
  if (n_reads && ((uintptr_t)d_cut & 3)) return sigax_fail(SIGAX_E_ARG, "d_cut must be 4-byte aligned");
  const PruneWork w = prune_work(n_reads, n_edges, d_uedges != nullptr, opts->careful != 0);
  if (n_reads && work_bytes < w.bytes)
    return sigax_fail(SIGAX_E_ARG, "workspace of %llu bytes, %llu needed (sigax_unitigs_prune_workspace)", (u64)work_bytes, w.bytes);
  const hipStream_t st = (hipStream_t)stream;
  const sigax_trim_opts topts = {opts->max_rounds, opts->min_branch_length, opts->min_branch_coverage, 0};
  if (n_reads == 0 || opts->delta == 0) {  // no cut step: the trim call, cut all zero
    const int rc = unitigs_trim_run(device, d_edges, n_edges, d_lengths, d_seqs, d_offs, n_reads, min_overlap, &topts, d_seq_offs, d_lay_offs,
                                    d_uflags, d_layout, d_useqs, d_removed, d_uedges, d_status16, d_work, work_bytes, stream, paced);
    if (rc != SIGAX_OK) return rc;
    if (d_status16) HIP_TRY(hipMemsetAsync((char*)d_status16 + 96, 0, 32, st));
    if (n_reads && n_edges) HIP_TRY(hipMemsetAsync(d_cut, 0, (size_t)n_edges * 4, st));
    return SIGAX_OK;
  }
  if (!d_lengths || !d_seqs || !d_offs || !d_seq_offs || !d_lay_offs || !d_uflags || !d_layout || !d_removed || !d_status16 || !d_work ||
      (n_edges && !d_edges))
    return sigax_fail(SIGAX_E_ARG, "NULL where a buffer is required");
  if (((uintptr_t)d_edges | (uintptr_t)d_layout | (uintptr_t)d_useqs | (uintptr_t)d_uedges | (uintptr_t)d_work) & 15)
    return sigax_fail(SIGAX_E_ARG, "d_edges, d_layout, d_useqs, d_uedges and d_work must be 16-byte aligned");
  if (((uintptr_t)d_offs | (uintptr_t)d_seq_offs | (uintptr_t)d_lay_offs | (uintptr_t)d_status16) & 7)
    return sigax_fail(SIGAX_E_ARG, "d_offs, d_seq_offs, d_lay_offs and d_status16 must be 8-byte aligned");
  if ((uintptr_t)d_removed & 3) return sigax_fail(SIGAX_E_ARG, "d_removed must be 4-byte aligned");
  HIP_TRY(hipSetDevice(device));
  UnitigPruneArgs a;
  static_cast<UnitigArgs&>(a) = unitig_args(d_edges, n_edges, d_lengths, d_seqs, d_offs, n_reads, min_overlap, d_seq_offs, d_lay_offs, d_uflags,
                                            d_layout, d_useqs, d_status16, d_work);
  char* base = (char*)d_work;
  a.removed = (uint32_t*)d_removed;
  a.trim = (u64*)(base + w.t.trim);
  a.verdict = (uint32_t*)(base + w.t.verdict);
  a.umap = (uint32_t*)(base + w.t.umap);
  a.round = 0;
  a.min_branch_length = opts->min_branch_length;
  a.min_branch_coverage = opts->min_branch_coverage;
  a.uedges = d_uedges;
  a.eflag = (uint32_t*)(base + w.t.eflag);
  a.escan = (u64*)(base + w.t.escan);
  a.epartial = (u64*)(base + w.t.epartial);
  a.cut = (uint32_t*)d_cut;
  a.maxlen = nullptr;
  a.maxself = (uint32_t*)(base + w.maxself);
  a.uniq = (uint32_t*)(base + w.uniq);
  a.keys = (u64*)(base + w.keys);
  a.key_cap = w.key_cap;
  a.prune = (u64*)(base + w.prune);
  a.delta = opts->delta;
  a.careful = opts->careful;
  a.num_reads = opts->num_reads;
  a.genome_size = opts->genome_size;
  a.uniq_threshold = opts->uniq_threshold;
  uint32_t* const maxlen = (uint32_t*)(base + w.maxlen);
  HIP_TRY(hipMemsetAsync(d_removed, 0, (size_t)n_reads * 4, st));
  if (n_edges) HIP_TRY(hipMemsetAsync(d_cut, 0, (size_t)n_edges * 4, st));
  HIP_TRY(hipMemsetAsync(a.trim, 0, TRIM_WORDS * 8, st));
  HIP_TRY(hipMemsetAsync(a.prune, 0, PRUNE_WORDS * 8, st));
  auto reset = [&]() -> hipError_t {
    const hipError_t e = hipMemsetAsync(base + w.t.u.zero_from, 0, (size_t)w.t.u.zero_bytes, st);
    return e != hipSuccess ? e : hipMemsetAsync(a.link, 0xFF, (size_t)n_reads * 16, st);
  };
  for (uint32_t r = 1; r <= opts->max_rounds; ++r) {
    a.round = r;
    {  // the cut step
      HIP_TRY(reset());
      a.maxlen = maxlen;
      launch_prune_cut_round(a, st);
      a.maxlen = nullptr;
    }
    HIP_TRY(reset());  // the trim step, over what the cut step left
    launch_prune_trim_round(a, st);
    if (paced) {
      u64 flag = 0;
      HIP_TRY(hipMemcpyAsync(&flag, a.trim + TRIM_ROUND0 + r, 8, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      if (flag == 0) break;
    }
  }
  a.round = 0;  // the unitigs of what is left
  HIP_TRY(reset());
  launch_unitigs_prune(a, st);
  launch_unitig_prune_lift(a, st);
  HIP_TRY(hipGetLastError());
  return SIGAX_OK;
}

extern "C" int sigax_unitigs_prune_device(int device, const sigax_edge* d_edges, uint64_t n_edges, const void* d_lengths, const void* d_seqs,
                                          const void* d_offs, uint64_t n_reads, uint32_t min_overlap, const sigax_prune_opts* opts,
                                          void* d_seq_offs, void* d_lay_offs, void* d_uflags, sigax_placement* d_layout, void* d_useqs,
                                          void* d_removed, void* d_cut, sigax_edge* d_uedges, void* d_status16, void* d_work,
                                          uint64_t work_bytes, void* stream) {
  return unitigs_prune_run(device, d_edges, n_edges, d_lengths, d_seqs, d_offs, n_reads, min_overlap, opts, d_seq_offs, d_lay_offs, d_uflags,
                           d_layout, d_useqs, d_removed, d_cut, d_uedges, d_status16, d_work, work_bytes, stream, false);
}

extern "C" int sigax_unitigs_prune_host(int device, const sigax_edge* edges, uint64_t n_edges, const uint32_t* lengths, const char* seqs,
                                        const uint64_t* offs, uint64_t n_reads, uint32_t min_overlap, const sigax_prune_opts* opts,
                                        uint64_t* n_unitigs, uint64_t** seq_offs, uint64_t** lay_offs, uint32_t** uflags,
                                        sigax_placement** layout, char** useqs, uint32_t** removed, uint32_t** cut, sigax_edge** uedges,
                                        uint64_t status16[16]) {
  if (!opts) return sigax_fail(SIGAX_E_ARG, "NULL where the prune options are required");
  return unitigs_rounds_host(device, edges, n_edges, lengths, seqs, offs, n_reads, min_overlap, nullptr, opts, nullptr, nullptr, n_unitigs,
                             seq_offs, lay_offs, uflags, layout, useqs, removed, cut, uedges, status16);
}

// ---- chimeric unitig removal ----
extern "C" int sigax_unitigs_chimeric_workspace(uint64_t n_reads, uint64_t n_edges, int want_graph, int careful, uint64_t* bytes) {
  if (!bytes) return sigax_fail(SIGAX_E_ARG, "bad argument");
  const int rc = unitig_limits(n_reads, n_edges);
  if (rc != SIGAX_OK) return rc;
  *bytes = chimeric_work(n_reads, n_edges, want_graph != 0, careful != 0).bytes;
  return SIGAX_OK;
}

static int unitigs_chimeric_run(int device, const sigax_edge* d_edges, uint64_t n_edges, const void* d_lengths, const void* d_seqs,
                                const void* d_offs, uint64_t n_reads, uint32_t min_overlap, const sigax_chimeric_opts* opts, void* d_seq_offs,
                                void* d_lay_offs, void* d_uflags, sigax_placement* d_layout, void* d_useqs, void* d_removed, void* d_cut,
                                sigax_edge* d_uedges, void* d_status20, void* d_work, uint64_t work_bytes, void* stream, bool paced) {
  const int rl = unitig_limits(n_reads, n_edges);
  if (rl != SIGAX_OK) return rl;
  const int ro = chimeric_opts_ok(opts, n_reads);
  if (ro != SIGAX_OK) return ro;
  const sigax_prune_opts* po = &opts->prune;
  const ChimericWork w = chimeric_work(n_reads, n_edges, d_uedges != nullptr, po->careful != 0);
  if (n_reads && work_bytes < w.bytes)
    return sigax_fail(SIGAX_E_ARG, "workspace of %llu bytes, %llu needed (sigax_unitigs_chimeric_workspace)", (u64)work_bytes, w.bytes);
  const hipStream_t st = (hipStream_t)stream;
  if (n_reads == 0 || opts->min_chimeric_length == 0) {  // no chimeric step: the prune call
    const int rc = unitigs_prune_run(device, d_edges, n_edges, d_lengths, d_seqs, d_offs, n_reads, min_overlap, po, d_seq_offs, d_lay_offs, d_uflags,
                                     d_layout, d_useqs, d_removed, d_cut, d_uedges, d_status20, d_work, work_bytes, stream, paced);
    if (rc != SIGAX_OK) return rc;
    if (d_status20) HIP_TRY(hipMemsetAsync((char*)d_status20 + 128, 0, 32, st));
    return SIGAX_OK;
  }
  if (!d_lengths || !d_seqs || !d_offs || !d_seq_offs || !d_lay_offs || !d_uflags || !d_layout || !d_removed || !d_status20 || !d_work ||
      (n_edges && (!d_edges || !d_cut)))
    return sigax_fail(SIGAX_E_ARG, "NULL where a buffer is required");
  if (((uintptr_t)d_edges | (uintptr_t)d_layout | (uintptr_t)d_useqs | (uintptr_t)d_uedges | (uintptr_t)d_work) & 15)
    return sigax_fail(SIGAX_E_ARG, "d_edges, d_layout, d_useqs, d_uedges and d_work must be 16-byte aligned");
  if (((uintptr_t)d_offs | (uintptr_t)d_seq_offs | (uintptr_t)d_lay_offs | (uintptr_t)d_status20) & 7)
    return sigax_fail(SIGAX_E_ARG, "d_offs, d_seq_offs, d_lay_offs and d_status20 must be 8-byte aligned");
  if ((uintptr_t)d_removed & 3) return sigax_fail(SIGAX_E_ARG, "d_removed must be 4-byte aligned");
  if ((uintptr_t)d_cut & 3) return sigax_fail(SIGAX_E_ARG, "d_cut must be 4-byte aligned");
  HIP_TRY(hipSetDevice(device));
  UnitigChimericArgs a;
  static_cast<UnitigArgs&>(a) = unitig_args(d_edges, n_edges, d_lengths, d_seqs, d_offs, n_reads, min_overlap, d_seq_offs, d_lay_offs, d_uflags,
                                            d_layout, d_useqs, d_status20, d_work);
  char* base = (char*)d_work;
  const PruneWork& pw = w.p;
  a.removed = (uint32_t*)d_removed;
  a.trim = (u64*)(base + pw.t.trim);
  a.verdict = (uint32_t*)(base + pw.t.verdict);
  a.umap = (uint32_t*)(base + pw.t.umap);
  a.round = 0;
  a.min_branch_length = po->min_branch_length;
  a.min_branch_coverage = po->min_branch_coverage;
  a.uedges = d_uedges;
  a.eflag = (uint32_t*)(base + pw.t.eflag);
  a.escan = (u64*)(base + pw.t.escan);
  a.epartial = (u64*)(base + pw.t.epartial);
  a.cut = (uint32_t*)d_cut;
  a.maxlen = nullptr;
  a.maxself = (uint32_t*)(base + pw.maxself);
  a.uniq = (uint32_t*)(base + pw.uniq);
  a.keys = (u64*)(base + pw.keys);
  a.key_cap = pw.key_cap;
  a.prune = (u64*)(base + pw.prune);
  a.delta = po->delta;
  a.careful = po->careful;
  a.num_reads = po->num_reads;
  a.genome_size = po->genome_size;
  a.uniq_threshold = po->uniq_threshold;
  a.nbr = (uint32_t*)(base + w.nbr);
  for (int k = 0; k < 2; ++k) {
    a.minb[k] = (u64*)(base + w.minb[k]);
    a.mink[k] = (u64*)(base + w.mink[k]);
  }
  a.chim = (u64*)(base + w.chim);
  a.prune_aside = (u64*)(base + w.aside);
  a.min_chimeric_length = opts->min_chimeric_length;
  a.min_chimeric_coverage = opts->min_chimeric_coverage;
  a.chimeric_delta = opts->chimeric_delta;
  a.chimeric_threshold = opts->chimeric_threshold;
  uint32_t* const maxlen = (uint32_t*)(base + pw.maxlen);
  HIP_TRY(hipMemsetAsync(d_removed, 0, (size_t)n_reads * 4, st));
  if (n_edges) HIP_TRY(hipMemsetAsync(d_cut, 0, (size_t)n_edges * 4, st));
  HIP_TRY(hipMemsetAsync(a.trim, 0, TRIM_WORDS * 8, st));
  HIP_TRY(hipMemsetAsync(a.prune, 0, PRUNE_WORDS * 8, st));
  HIP_TRY(hipMemsetAsync(a.chim, 0, CHIM_WORDS * 8, st));
  HIP_TRY(hipMemsetAsync(a.prune_aside, 0, PRUNE_WORDS * 8, st));
  auto reset = [&]() -> hipError_t {
    const hipError_t e = hipMemsetAsync(base + pw.t.u.zero_from, 0, (size_t)pw.t.u.zero_bytes, st);
    return e != hipSuccess ? e : hipMemsetAsync(a.link, 0xFF, (size_t)n_reads * 16, st);
  };
  for (uint32_t r = 1; r <= po->max_rounds; ++r) {
    a.round = r;
    if (po->delta > 0) {  // the cut step
      HIP_TRY(reset());
      a.maxlen = maxlen;
      launch_prune_cut_round(a, st);
      a.maxlen = nullptr;
    }
    HIP_TRY(reset());  // the trim step, over what the cut step left
    launch_prune_trim_round(a, st);
    HIP_TRY(reset());  // the chimeric step, over what the trim step left
    launch_chimeric_round(a, st);
    if (paced) {
      u64 flag = 0;
      HIP_TRY(hipMemcpyAsync(&flag, a.trim + TRIM_ROUND0 + r, 8, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      if (flag == 0) break;
    }
  }
  a.round = 0;  // the unitigs of what is left
  HIP_TRY(reset());
  launch_unitigs_prune(a, st);
  launch_unitig_prune_lift(a, st);
  launch_chimeric_status(a, st);
  HIP_TRY(hipGetLastError());
  return SIGAX_OK;
}

extern "C" int sigax_unitigs_chimeric_device(int device, const sigax_edge* d_edges, uint64_t n_edges, const void* d_lengths, const void* d_seqs,
                                             const void* d_offs, uint64_t n_reads, uint32_t min_overlap, const sigax_chimeric_opts* opts,
                                             void* d_seq_offs, void* d_lay_offs, void* d_uflags, sigax_placement* d_layout, void* d_useqs,
                                             void* d_removed, void* d_cut, sigax_edge* d_uedges, void* d_status20, void* d_work,
                                             uint64_t work_bytes, void* stream) {
  return unitigs_chimeric_run(device, d_edges, n_edges, d_lengths, d_seqs, d_offs, n_reads, min_overlap, opts, d_seq_offs, d_lay_offs, d_uflags,
                              d_layout, d_useqs, d_removed, d_cut, d_uedges, d_status20, d_work, work_bytes, stream, false);
}

extern "C" int sigax_unitigs_chimeric_host(int device, const sigax_edge* edges, uint64_t n_edges, const uint32_t* lengths, const char* seqs,
                                           const uint64_t* offs, uint64_t n_reads, uint32_t min_overlap, const sigax_chimeric_opts* opts,
                                           uint64_t* n_unitigs, uint64_t** seq_offs, uint64_t** lay_offs, uint32_t** uflags,
                                           sigax_placement** layout, char** useqs, uint32_t** removed, uint32_t** cut, sigax_edge** uedges,
                                           uint64_t status20[20]) {
  if (!opts) return sigax_fail(SIGAX_E_ARG, "NULL where the chimeric options are required");
  return unitigs_rounds_host(device, edges, n_edges, lengths, seqs, offs, n_reads, min_overlap, nullptr, &opts->prune, opts, nullptr, n_unitigs,
                             seq_offs, lay_offs, uflags, layout, useqs, removed, cut, uedges, status20);
}

// ---- bubble popping ----
extern "C" int sigax_unitigs_bubble_workspace(uint64_t n_reads, uint64_t n_edges, int want_graph, int careful, uint64_t* bytes) {
  if (!bytes) return sigax_fail(SIGAX_E_ARG, "bad argument");
  const int rc = unitig_limits(n_reads, n_edges);
  if (rc != SIGAX_OK) return rc;
  *bytes = bubble_work(n_reads, n_edges, want_graph != 0, careful != 0).bytes;
  return SIGAX_OK;
}

static int unitigs_bubble_run(int device, const sigax_edge* d_edges, uint64_t n_edges, const void* d_lengths, const void* d_seqs,
                              const void* d_offs, uint64_t n_reads, uint32_t min_overlap, const sigax_bubble_opts* opts, void* d_seq_offs,
                              void* d_lay_offs, void* d_uflags, sigax_placement* d_layout, void* d_useqs, void* d_removed, void* d_cut,
                              sigax_edge* d_uedges, void* d_status24, void* d_work, uint64_t work_bytes, void* stream, bool paced) {
  const int rl = unitig_limits(n_reads, n_edges);
  if (rl != SIGAX_OK) return rl;
  const int ro = bubble_opts_ok(opts, n_reads);
  if (ro != SIGAX_OK) return ro;
  const sigax_chimeric_opts* co = &opts->chimeric;
  const sigax_prune_opts* po = &co->prune;
  const BubbleWork w = bubble_work(n_reads, n_edges, d_uedges != nullptr, po->careful != 0);
  if (n_reads && work_bytes < w.bytes)
    return sigax_fail(SIGAX_E_ARG, "workspace of %llu bytes, %llu needed (sigax_unitigs_bubble_workspace)", (u64)work_bytes, w.bytes);
  const hipStream_t st = (hipStream_t)stream;
  if (n_reads == 0 || opts->max_bubble_span == 0) {  // no bubble step: the chimeric call
    const int rc = unitigs_chimeric_run(device, d_edges, n_edges, d_lengths, d_seqs, d_offs, n_reads, min_overlap, co, d_seq_offs, d_lay_offs,
                                        d_uflags, d_layout, d_useqs, d_removed, d_cut, d_uedges, d_status24, d_work, work_bytes, stream, paced);
    if (rc != SIGAX_OK) return rc;
    if (d_status24) HIP_TRY(hipMemsetAsync((char*)d_status24 + 160, 0, 32, st));
    return SIGAX_OK;
  }
  if (!d_lengths || !d_seqs || !d_offs || !d_seq_offs || !d_lay_offs || !d_uflags || !d_layout || !d_removed || !d_status24 || !d_work ||
      (n_edges && (!d_edges || !d_cut)))
    return sigax_fail(SIGAX_E_ARG, "NULL where a buffer is required");
  if (((uintptr_t)d_edges | (uintptr_t)d_layout | (uintptr_t)d_useqs | (uintptr_t)d_uedges | (uintptr_t)d_work) & 15)
    return sigax_fail(SIGAX_E_ARG, "d_edges, d_layout, d_useqs, d_uedges and d_work must be 16-byte aligned");
  if (((uintptr_t)d_offs | (uintptr_t)d_seq_offs | (uintptr_t)d_lay_offs | (uintptr_t)d_status24) & 7)
    return sigax_fail(SIGAX_E_ARG, "d_offs, d_seq_offs, d_lay_offs and d_status24 must be 8-byte aligned");
  if ((uintptr_t)d_removed & 3) return sigax_fail(SIGAX_E_ARG, "d_removed must be 4-byte aligned");
  if ((uintptr_t)d_cut & 3) return sigax_fail(SIGAX_E_ARG, "d_cut must be 4-byte aligned");
  HIP_TRY(hipSetDevice(device));
  UnitigBubbleArgs a;
  static_cast<UnitigArgs&>(a) = unitig_args(d_edges, n_edges, d_lengths, d_seqs, d_offs, n_reads, min_overlap, d_seq_offs, d_lay_offs, d_uflags,
                                            d_layout, d_useqs, d_status24, d_work);
  char* base = (char*)d_work;
  const ChimericWork& cw = w.c;
  const PruneWork& pw = cw.p;
  a.removed = (uint32_t*)d_removed;
  a.trim = (u64*)(base + pw.t.trim);
  a.verdict = (uint32_t*)(base + pw.t.verdict);
  a.umap = (uint32_t*)(base + pw.t.umap);
  a.round = 0;
  a.min_branch_length = po->min_branch_length;
  a.min_branch_coverage = po->min_branch_coverage;
  a.uedges = d_uedges;
  a.eflag = (uint32_t*)(base + pw.t.eflag);
  a.escan = (u64*)(base + pw.t.escan);
  a.epartial = (u64*)(base + pw.t.epartial);
  a.cut = (uint32_t*)d_cut;
  a.maxlen = nullptr;
  a.maxself = (uint32_t*)(base + pw.maxself);
  a.uniq = (uint32_t*)(base + pw.uniq);
  a.keys = (u64*)(base + pw.keys);
  a.key_cap = pw.key_cap;
  a.prune = (u64*)(base + pw.prune);
  a.delta = po->delta;
  a.careful = po->careful;
  a.num_reads = po->num_reads;
  a.genome_size = po->genome_size;
  a.uniq_threshold = po->uniq_threshold;
  a.nbr = (uint32_t*)(base + cw.nbr);
  for (int k = 0; k < 2; ++k) {
    a.minb[k] = (u64*)(base + cw.minb[k]);
    a.mink[k] = (u64*)(base + cw.mink[k]);
  }
  a.chim = (u64*)(base + cw.chim);
  a.prune_aside = (u64*)(base + cw.aside);
  a.min_chimeric_length = co->min_chimeric_length;
  a.min_chimeric_coverage = co->min_chimeric_coverage;
  a.chimeric_delta = co->chimeric_delta;
  a.chimeric_threshold = co->chimeric_threshold;
  a.bnbr = (uint32_t*)(base + w.bnbr);
  a.blen = (uint32_t*)(base + w.blen);
  a.arm = (uint4*)(base + w.arm);
  a.aside = (uint32_t*)(base + w.aside);
  a.gslot = (uint32_t*)(base + w.gslot);
  a.losers = (uint32_t*)(base + w.losers);
  a.table = (uint32_t*)(base + w.table);
  a.best = (u64*)(base + w.best);
  a.group_cap = w.group_cap;
  a.where = (uint4*)(base + w.where);
  a.bub = (u64*)(base + w.bub);
  a.max_bubble_span = opts->max_bubble_span;
  a.max_divergence_permille = opts->max_divergence_permille;
  uint32_t* const maxlen = (uint32_t*)(base + pw.maxlen);
  HIP_TRY(hipMemsetAsync(d_removed, 0, (size_t)n_reads * 4, st));
  if (n_edges) HIP_TRY(hipMemsetAsync(d_cut, 0, (size_t)n_edges * 4, st));
  HIP_TRY(hipMemsetAsync(a.trim, 0, TRIM_WORDS * 8, st));
  HIP_TRY(hipMemsetAsync(a.prune, 0, PRUNE_WORDS * 8, st));
  HIP_TRY(hipMemsetAsync(a.chim, 0, CHIM_WORDS * 8, st));
  HIP_TRY(hipMemsetAsync(a.prune_aside, 0, PRUNE_WORDS * 8, st));
  HIP_TRY(hipMemsetAsync(a.bub, 0, BUB_WORDS * 8, st));
  auto reset = [&]() -> hipError_t {
    const hipError_t e = hipMemsetAsync(base + pw.t.u.zero_from, 0, (size_t)pw.t.u.zero_bytes, st);
    return e != hipSuccess ? e : hipMemsetAsync(a.link, 0xFF, (size_t)n_reads * 16, st);
  };
  for (uint32_t r = 1; r <= po->max_rounds; ++r) {
    a.round = r;
    if (po->delta > 0) {  // the cut step
      HIP_TRY(reset());
      a.maxlen = maxlen;
      launch_prune_cut_round(a, st);
      a.maxlen = nullptr;
    }
    HIP_TRY(reset());  // the trim step, over what the cut step left
    launch_prune_trim_round(a, st);
    HIP_TRY(reset());  // the bubble step, over what the trim step left
    launch_bubble_round(a, st);
    if (co->min_chimeric_length > 0) {
      HIP_TRY(reset());  // the chimeric step, over what the bubble step left
      launch_chimeric_round(a, st);
    }
    if (paced) {
      u64 flag = 0;
      HIP_TRY(hipMemcpyAsync(&flag, a.trim + TRIM_ROUND0 + r, 8, hipMemcpyDeviceToHost, st));
      HIP_TRY(hipStreamSynchronize(st));
      if (flag == 0) break;
    }
  }
  a.round = 0;  // the unitigs of what is left
  HIP_TRY(reset());
  launch_unitigs_prune(a, st);
  launch_unitig_prune_lift(a, st);
  launch_chimeric_status(a, st);
  launch_bubble_status(a, st);
  HIP_TRY(hipGetLastError());
  return SIGAX_OK;
}

extern "C" int sigax_unitigs_bubble_device(int device, const sigax_edge* d_edges, uint64_t n_edges, const void* d_lengths, const void* d_seqs,
                                           const void* d_offs, uint64_t n_reads, uint32_t min_overlap, const sigax_bubble_opts* opts,
                                           void* d_seq_offs, void* d_lay_offs, void* d_uflags, sigax_placement* d_layout, void* d_useqs,
                                           void* d_removed, void* d_cut, sigax_edge* d_uedges, void* d_status24, void* d_work,
                                           uint64_t work_bytes, void* stream) {
  return unitigs_bubble_run(device, d_edges, n_edges, d_lengths, d_seqs, d_offs, n_reads, min_overlap, opts, d_seq_offs, d_lay_offs, d_uflags,
                            d_layout, d_useqs, d_removed, d_cut, d_uedges, d_status24, d_work, work_bytes, stream, false);
}

extern "C" int sigax_unitigs_bubble_host(int device, const sigax_edge* edges, uint64_t n_edges, const uint32_t* lengths, const char* seqs,
                                         const uint64_t* offs, uint64_t n_reads, uint32_t min_overlap, const sigax_bubble_opts* opts,
                                         uint64_t* n_unitigs, uint64_t** seq_offs, uint64_t** lay_offs, uint32_t** uflags,
                                         sigax_placement** layout, char** useqs, uint32_t** removed, uint32_t** cut, sigax_edge** uedges,
                                         uint64_t status24[24]) {
  if (!opts) return sigax_fail(SIGAX_E_ARG, "NULL where the bubble options are required");
  return unitigs_rounds_host(device, edges, n_edges, lengths, seqs, offs, n_reads, min_overlap, nullptr, &opts->chimeric.prune, &opts->chimeric, opts,
                             n_unitigs, seq_offs, lay_offs, uflags, layout, useqs, removed, cut, uedges, status24);
}
