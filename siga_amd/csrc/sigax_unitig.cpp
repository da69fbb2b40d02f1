// siga_amd/csrc/sigax_unitig.cpp -- `siga unitig` on the device: the entry points of sigax_unitig.hip.
#include <cstring>

#include "sigax_internal.h"

static_assert(sizeof(sigax_placement) == 16, "sigax_placement must be 16 bytes");

namespace {

// What a call does beyond the plain unitigs: every level is the one below it with one more step in its rounds, a longer
// status block (6, 12, 16, 20, 24, 32, 40 counts) and more scratch behind the same pieces.
enum Level { UNITIG = 0, TRIM = 1, PRUNE = 2, CHIMERIC = 3, BUBBLE = 4, INDEL = 5, REDUCE = 6 };
const char* const LEVEL_NAME[] = {"unitig", "trim", "prune", "chimeric", "bubble", "indel", "reduce"};
const char* const WORKSPACE_FN[] = {"sigax_unitigs_workspace", "sigax_unitigs_trim_workspace", "sigax_unitigs_prune_workspace",
                                    "sigax_unitigs_chimeric_workspace", "sigax_unitigs_bubble_workspace", "sigax_unitigs_indel_workspace",
                                    "sigax_unitigs_reduce_workspace"};
u64 status_words(int level) { return level == UNITIG ? 6 : level == REDUCE ? 40 : level == INDEL ? 32 : 8 + 4 * (u64)level; }

// where the pieces of the caller's scratch lie (every piece 16-byte aligned).  A level's pieces follow those of the level below
// at the same offsets: a call whose upper steps are off runs as the lower one over the same scratch.
struct RoundsWork {
  u64 rank[2], dist[2], link, dst, src, scan, partial, scan_total, counts, deg, closing, cnt;  // UNITIG
  u64 zero_from, zero_bytes;                   // deg, closing and counts lie together: one memset
  u64 trim, verdict, umap, eflag, escan, epartial;                                    // TRIM: the rounds and the lifted records
  u64 prune, maxlen, uniq, maxself, keys, key_cap;                                    // PRUNE: a round's cut step
  u64 chim, prune_aside, nbr, minb[2], mink[2];                                       // CHIMERIC: a round's chimeric step
  u64 bub, bnbr, blen, arm, where, aside, gslot, losers, table, best, group_cap;      // BUBBLE: a round's bubble step
  u64 ind, pairs;                                                                     // INDEL: a round's indel step
  u64 red, rcnt, rfill, roff, rpartial, rtotal, radj, rtable, red_cap;                // REDUCE: a reduction pass
  u64 bytes;
};
RoundsWork rounds_work(Level level, u64 n, u64 n_edges, bool graph, bool careful) {
  RoundsWork w = {};
  u64 at = 0;
  auto take = [&](u64 bytes) {
    const u64 here = at;
    at += (bytes + 15) & ~15ull;
    return here;
  };
  auto ends_at = [&](Level l) {  // the level's last piece has been taken
    w.bytes = at;
    return level == l;
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
  if (ends_at(UNITIG)) return w;
  w.trim = take(TRIM_WORDS * 8);
  w.verdict = take(n * 4);
  w.umap = take(n * 4);
  w.eflag = w.escan = w.epartial = at;
  if (graph) {
    w.eflag = take(n_edges * 4);
    w.escan = take((n_edges + 1) * 8);
    w.epartial = take(scan_partials_needed(n_edges) * 8);
  }
  if (ends_at(TRIM)) return w;
  w.prune = take(PRUNE_WORDS * 8);
  w.maxlen = take(2 * n * 4);
  w.uniq = take(n * 4);
  w.maxself = w.keys = at;
  if (careful) {
    w.maxself = take(2 * n * 4);
    w.key_cap = 16;
    while (w.key_cap < 4 * n_edges) w.key_cap <<= 1;
    w.keys = take(w.key_cap * 8);
  }
  if (ends_at(PRUNE)) return w;
  w.chim = take(CHIM_WORDS * 8);
  w.prune_aside = take(PRUNE_WORDS * 8);
  w.nbr = take(2 * n * 4);
  for (int k = 0; k < 2; ++k) w.minb[k] = take(2 * n * 8);
  for (int k = 0; k < 2; ++k) w.mink[k] = take(2 * n * 8);
  if (ends_at(CHIMERIC)) return w;
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
  if (ends_at(BUBBLE)) return w;
  w.ind = take(IND_WORDS * 8);
  w.pairs = take(n * 4);
  if (ends_at(INDEL)) return w;
  w.red = take(RED_WORDS * 8);
  w.rcnt = take((2 * n + 1) * 4);
  w.rfill = take(2 * n * 4);
  w.roff = take((2 * n + 1) * 8);
  w.rpartial = take(scan_partials_needed(2 * n) * 8);
  w.rtotal = take(8);
  w.radj = take(2 * n_edges * 8);
  w.red_cap = 16;
  while (w.red_cap < 4 * n_edges) w.red_cap <<= 1;
  w.rtable = take(w.red_cap * 4);
  ends_at(REDUCE);
  return w;
}

int unitig_limits(u64 n_reads, u64 n_edges) {
  if (n_reads >= (1ull << 31)) return sigax_fail(SIGAX_E_ARG, "2^31 reads or more: a state names a read end in 32 bits");
  if (n_edges > (1ull << 32)) return sigax_fail(SIGAX_E_ARG, "more than 2^32 records");
  return SIGAX_OK;
}

int workspace_of(Level level, u64 n_reads, u64 n_edges, int want_graph, int careful, uint64_t* bytes) {
  if (!bytes) return sigax_fail(SIGAX_E_ARG, "bad argument");
  const int rc = unitig_limits(n_reads, n_edges);
  if (rc != SIGAX_OK) return rc;
  *bytes = rounds_work(level, n_reads, n_edges, want_graph != 0, careful != 0).bytes;
  return SIGAX_OK;
}

// The options of every rounds call as the reduce call's: a lower level leaves the fields of the upper ones zero, and a step
// whose own threshold is zero is off.  NULL stays NULL (opts_ok refuses it).
const sigax_reduce_opts* opts_view(const sigax_trim_opts* o, sigax_reduce_opts* v) {
  if (!o) return nullptr;
  *v = {};
  sigax_prune_opts& p = v->indel.bubble.chimeric.prune;
  p.max_rounds = o->max_rounds;
  p.min_branch_length = o->min_branch_length;
  p.min_branch_coverage = o->min_branch_coverage;
  p.reserved = o->reserved;
  return v;
}
const sigax_reduce_opts* opts_view(const sigax_prune_opts* o, sigax_reduce_opts* v) {
  if (!o) return nullptr;
  *v = {};
  v->indel.bubble.chimeric.prune = *o;
  return v;
}
const sigax_reduce_opts* opts_view(const sigax_chimeric_opts* o, sigax_reduce_opts* v) {
  if (!o) return nullptr;
  *v = {};
  v->indel.bubble.chimeric = *o;
  return v;
}
const sigax_reduce_opts* opts_view(const sigax_bubble_opts* o, sigax_reduce_opts* v) {
  if (!o) return nullptr;
  *v = {};
  v->indel.bubble = *o;
  return v;
}
const sigax_reduce_opts* opts_view(const sigax_indel_opts* o, sigax_reduce_opts* v) {
  if (!o) return nullptr;
  *v = {};
  v->indel = *o;
  return v;
}
const sigax_reduce_opts* opts_view(const sigax_reduce_opts* o, sigax_reduce_opts*) { return o; }

// prune's refusals, then chimeric's, then bubble's, then indel's, then reduce's.  The bubble and the indel step and the reduction
// need neither G nor N.
int opts_ok(Level level, const sigax_reduce_opts* ro, u64 n_reads, u64 n_edges) {
  if (!ro) return sigax_fail(SIGAX_E_ARG, "NULL where the %s options are required", LEVEL_NAME[level]);
  const sigax_indel_opts* io = &ro->indel;
  const sigax_bubble_opts* o = &io->bubble;
  const sigax_prune_opts& p = o->chimeric.prune;
  if (p.reserved != 0) return sigax_fail(SIGAX_E_ARG, "sigax_%s_opts.reserved must be 0", level == TRIM ? "trim" : "prune");
  if (p.careful > 1) return sigax_fail(SIGAX_E_ARG, "careful %u: 0 or 1", p.careful);
  if (p.max_rounds > TRIM_MAX_ROUNDS) return sigax_fail(SIGAX_E_ARG, "max_rounds %u: at most %d", p.max_rounds, (int)TRIM_MAX_ROUNDS);
  if (level >= PRUNE) {
    if (p.num_reads < n_reads) return sigax_fail(SIGAX_E_ARG, "num_reads %llu below the %llu reads given", (u64)p.num_reads, n_reads);
    if (p.delta > 0 && p.genome_size == 0) return sigax_fail(SIGAX_E_ARG, "genome_size must be given with delta > 0");
  }
  if (level >= CHIMERIC) {
    if (o->chimeric.reserved2 != 0) return sigax_fail(SIGAX_E_ARG, "sigax_chimeric_opts.reserved2 must be 0");
    if (o->chimeric.min_chimeric_length > 0 && p.genome_size == 0)
      return sigax_fail(SIGAX_E_ARG, "genome_size must be given with min_chimeric_length > 0");
  }
  if (level >= BUBBLE && (o->reserved3[0] != 0 || o->reserved3[1] != 0)) return sigax_fail(SIGAX_E_ARG, "sigax_bubble_opts.reserved3 must be 0");
  if (level >= INDEL) {
    if (io->reserved4[0] != 0 || io->reserved4[1] != 0) return sigax_fail(SIGAX_E_ARG, "sigax_indel_opts.reserved4 must be 0");
    if (io->max_edits > SIGAX_INDEL_MAX_EDITS) return sigax_fail(SIGAX_E_ARG, "max_edits %u: at most %u", io->max_edits, SIGAX_INDEL_MAX_EDITS);
    if (io->max_edits > 0 && (o->max_bubble_span == 0 || o->max_bubble_span > SIGAX_INDEL_MAX_SPAN))
      return sigax_fail(SIGAX_E_ARG, "max_bubble_span %u with max_edits > 0: 1 to %u", o->max_bubble_span, SIGAX_INDEL_MAX_SPAN);
  }
  if (level >= REDUCE) {
    if (ro->reserved5[0] != 0 || ro->reserved5[1] != 0 || ro->reserved5[2] != 0) return sigax_fail(SIGAX_E_ARG, "sigax_reduce_opts.reserved5 must be 0");
    if (ro->reduce > 1) return sigax_fail(SIGAX_E_ARG, "reduce %u: 0 or 1", ro->reduce);
    if (ro->reduce && n_edges >= (1ull << 32)) return sigax_fail(SIGAX_E_ARG, "reduce with 2^32 records: a table slot names a record in 32 bits");
  }
  return SIGAX_OK;
}

// the caller's device buffers, as every device form names them; a form without one of them leaves it NULL
struct UnitigBufs {
  const sigax_edge* edges;
  const void *lengths, *seqs, *offs;
  void *seq_offs, *lay_offs, *uflags;
  sigax_placement* layout;
  void *useqs, *removed, *cut;
  sigax_edge* uedges;
  void *status, *work;
  u64 work_bytes;
};

// the buffers of a call with reads: the ones it needs are there, all are aligned, and the scratch is as large as the level asks
int bufs_ok(Level level, const UnitigBufs& b, u64 n_edges, const RoundsWork& w) {
  const struct {
    const void* p;
    const char* name;
    unsigned align;
    bool required;
  } bufs[] = {{b.edges, "d_edges", 16, n_edges != 0},
              {b.lengths, "d_lengths", 1, true},
              {b.seqs, "d_seqs", 1, true},
              {b.offs, "d_offs", 8, true},
              {b.seq_offs, "d_seq_offs", 8, true},
              {b.lay_offs, "d_lay_offs", 8, true},
              {b.uflags, "d_uflags", 1, true},
              {b.layout, "d_layout", 16, true},
              {b.useqs, "d_useqs", 16, false},
              {b.removed, "d_removed", 4, level >= TRIM},
              {b.cut, "d_cut", 4, level >= PRUNE && n_edges != 0},
              {b.uedges, "d_uedges", 16, false},
              {b.status, "d_status", 8, true},
              {b.work, "d_work", 16, true}};
  for (const auto& x : bufs)
    if (x.required && !x.p) return sigax_fail(SIGAX_E_ARG, "%s: NULL where a buffer is required", x.name);
  for (const auto& x : bufs)
    if ((uintptr_t)x.p & (x.align - 1)) return sigax_fail(SIGAX_E_ARG, "%s must be %u-byte aligned", x.name, x.align);
  if (b.work_bytes < w.bytes) return sigax_fail(SIGAX_E_ARG, "workspace of %llu bytes, %llu needed (%s)", (u64)b.work_bytes, w.bytes, WORKSPACE_FN[level]);
  return SIGAX_OK;
}

// ---- the argument block, each function the fields of its level ----
UnitigArgs unitig_args(const UnitigBufs& b, const RoundsWork& w, u64 n_edges, u64 n, uint32_t min_overlap) {
  char* base = (char*)b.work;
  UnitigArgs a;
  a.edges = b.edges;
  a.n_edges = n_edges;
  a.n_reads = n;
  a.lengths = (const uint32_t*)b.lengths;
  a.seqs = (const unsigned char*)b.seqs;
  a.offs = (const u64*)b.offs;
  a.min_overlap = min_overlap;
  a.seq_offs = (u64*)b.seq_offs;
  a.lay_offs = (u64*)b.lay_offs;
  a.uflags = (uint32_t*)b.uflags;
  a.layout = b.layout;
  a.useqs = (unsigned char*)b.useqs;
  a.status = (u64*)b.status;
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

void trim_args(UnitigTrimArgs& a, const UnitigBufs& b, const RoundsWork& w, const sigax_prune_opts& o) {
  char* base = (char*)b.work;
  a.removed = (uint32_t*)b.removed;
  a.trim = (u64*)(base + w.trim);
  a.verdict = (uint32_t*)(base + w.verdict);
  a.umap = (uint32_t*)(base + w.umap);
  a.round = 0;
  a.min_branch_length = o.min_branch_length;
  a.min_branch_coverage = o.min_branch_coverage;
  a.uedges = b.uedges;
  a.eflag = (uint32_t*)(base + w.eflag);
  a.escan = (u64*)(base + w.escan);
  a.epartial = (u64*)(base + w.epartial);
}

void prune_args(UnitigPruneArgs& a, const UnitigBufs& b, const RoundsWork& w, const sigax_prune_opts& o) {
  char* base = (char*)b.work;
  a.cut = (uint32_t*)b.cut;
  a.maxlen = nullptr;  // set for a cut step's launch alone
  a.maxself = (uint32_t*)(base + w.maxself);
  a.uniq = (uint32_t*)(base + w.uniq);
  a.keys = (u64*)(base + w.keys);
  a.key_cap = w.key_cap;
  a.prune = (u64*)(base + w.prune);
  a.delta = o.delta;
  a.careful = o.careful;
  a.num_reads = o.num_reads;
  a.genome_size = o.genome_size;
  a.uniq_threshold = o.uniq_threshold;
}

void chimeric_args(UnitigChimericArgs& a, const UnitigBufs& b, const RoundsWork& w, const sigax_chimeric_opts& o) {
  char* base = (char*)b.work;
  a.nbr = (uint32_t*)(base + w.nbr);
  for (int k = 0; k < 2; ++k) {
    a.minb[k] = (u64*)(base + w.minb[k]);
    a.mink[k] = (u64*)(base + w.mink[k]);
  }
  a.chim = (u64*)(base + w.chim);
  a.prune_aside = (u64*)(base + w.prune_aside);
  a.min_chimeric_length = o.min_chimeric_length;
  a.min_chimeric_coverage = o.min_chimeric_coverage;
  a.chimeric_delta = o.chimeric_delta;
  a.chimeric_threshold = o.chimeric_threshold;
}

void bubble_args(UnitigBubbleArgs& a, const UnitigBufs& b, const RoundsWork& w, const sigax_bubble_opts& o) {
  char* base = (char*)b.work;
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
  a.max_bubble_span = o.max_bubble_span;
  a.max_divergence_permille = o.max_divergence_permille;
}

void indel_args(UnitigIndelArgs& a, const UnitigBufs& b, const RoundsWork& w, const sigax_indel_opts& o) {
  char* base = (char*)b.work;
  a.pairs = (uint32_t*)(base + w.pairs);
  a.ind = (u64*)(base + w.ind);
  a.max_edits = o.max_edits;
  a.max_edit_permille = o.max_edit_permille;
}

void reduce_args(UnitigReduceArgs& a, const UnitigBufs& b, const RoundsWork& w) {
  char* base = (char*)b.work;
  a.red = (u64*)(base + w.red);
  a.rcnt = (uint32_t*)(base + w.rcnt);
  a.rfill = (uint32_t*)(base + w.rfill);
  a.roff = (u64*)(base + w.roff);
  a.rpartial = (u64*)(base + w.rpartial);
  a.rtotal = (u64*)(base + w.rtotal);
  a.radj = (uint2*)(base + w.radj);
  a.rtable = (uint32_t*)(base + w.rtable);
  a.red_cap = w.red_cap;
  a.red_prev = 0;
}

// The rounds of every form, device and host.  A round is up to six steps, each over the graph the step before left: reduce (REDUCE,
// reduce = 1: a pass that flags records and removes nothing, so it never keeps the loop going), cut (PRUNE up, delta > 0), trim,
// bubble (BUBBLE up, Lb > 0), indel (INDEL, E > 0), chimeric (CHIMERIC up, Lc > 0); then the unitigs of what is left, the lifted
// records and the counts.  A call whose top step is off runs as the level below -- down to the trim kernels over the trim
// block when nothing cuts -- and the counts of the steps that are off are zeroed behind it; the scratch is still asked for as
// the requested level lays it out.  With reduce = 1 the call runs as PRUNE at the least: the kernels that skip cut[i] != 0.  One more
// reduction pass runs before the final unitigs; it is idle when the last round that ran changed nothing.
// paced: the host form's loop -- it reads each round's flag and stops after the first round that changed nothing, where the
// device form enqueues every round and lets the idle ones leave at once.
int unitigs_rounds(Level level, int device, u64 n_edges, u64 n_reads, uint32_t min_overlap, const sigax_reduce_opts* ropts, const UnitigBufs& b,
                   void* stream, bool paced) {
  const int rl = unitig_limits(n_reads, n_edges);
  if (rl != SIGAX_OK) return rl;
  const int ro = opts_ok(level, ropts, n_reads, n_edges);
  if (ro != SIGAX_OK) return ro;
  const sigax_indel_opts* const iopts = &ropts->indel;
  const sigax_bubble_opts* const opts = &iopts->bubble;
  const sigax_chimeric_opts& co = opts->chimeric;
  const sigax_prune_opts& po = co.prune;
  const RoundsWork w = rounds_work(level, n_reads, n_edges, b.uedges != nullptr, po.careful != 0);
  if (n_reads) {
    const int rb = bufs_ok(level, b, n_edges, w);
    if (rb != SIGAX_OK) return rb;
  }
  HIP_TRY(hipSetDevice(device));
  const hipStream_t st = (hipStream_t)stream;
  if (n_reads == 0) {
    if (b.status) HIP_TRY(hipMemsetAsync(b.status, 0, (size_t)status_words(level) * 8, st));
    return SIGAX_OK;
  }
  int eff = level;  // the level the call runs as
  const bool red = level == REDUCE && ropts->reduce != 0;
  if (eff == REDUCE) eff = INDEL;  // (the reduction is no level of its own below: `red` says whether its passes run)
  if (eff == INDEL && iopts->max_edits == 0) eff = BUBBLE;
  if (eff == BUBBLE && opts->max_bubble_span == 0) eff = CHIMERIC;
  if (eff == CHIMERIC && co.min_chimeric_length == 0) eff = PRUNE;
  if (eff == PRUNE && po.delta == 0) eff = TRIM;
  if (red && eff < PRUNE) eff = PRUNE;

  UnitigReduceArgs a = {};
  static_cast<UnitigArgs&>(a) = unitig_args(b, w, n_edges, n_reads, min_overlap);
  trim_args(a, b, w, po);
  if (eff >= PRUNE) prune_args(a, b, w, po);
  if (eff >= CHIMERIC) chimeric_args(a, b, w, co);
  if (eff >= BUBBLE) bubble_args(a, b, w, *opts);
  if (eff >= INDEL) indel_args(a, b, w, *iopts);
  if (red) reduce_args(a, b, w);
  char* base = (char*)b.work;
  uint32_t* const maxlen = (uint32_t*)(base + w.maxlen);

  HIP_TRY(hipMemsetAsync(b.removed, 0, (size_t)n_reads * 4, st));
  if (eff >= PRUNE && n_edges) HIP_TRY(hipMemsetAsync(b.cut, 0, (size_t)n_edges * 4, st));
  HIP_TRY(hipMemsetAsync(a.trim, 0, TRIM_WORDS * 8, st));
  if (eff >= PRUNE) HIP_TRY(hipMemsetAsync(a.prune, 0, PRUNE_WORDS * 8, st));
  if (eff >= CHIMERIC) {
    HIP_TRY(hipMemsetAsync(a.chim, 0, CHIM_WORDS * 8, st));
    HIP_TRY(hipMemsetAsync(a.prune_aside, 0, PRUNE_WORDS * 8, st));
  }
  if (eff >= BUBBLE) HIP_TRY(hipMemsetAsync(a.bub, 0, BUB_WORDS * 8, st));
  if (eff >= INDEL) HIP_TRY(hipMemsetAsync(a.ind, 0, IND_WORDS * 8, st));
  if (red) HIP_TRY(hipMemsetAsync(a.red, 0, RED_WORDS * 8, st));
  auto reset = [&]() -> hipError_t {  // every pass over degrees, links and counts of its own
    const hipError_t e = hipMemsetAsync(base + w.zero_from, 0, (size_t)w.zero_bytes, st);
    return e != hipSuccess ? e : hipMemsetAsync(a.link, 0xFF, (size_t)n_reads * 16, st);
  };
  uint32_t last = 0;  // the last round that ran
  for (uint32_t r = 1; r <= po.max_rounds; ++r) {
    a.round = last = r;
    if (red) {  // the reduction pass, over what the round before left
      a.red_prev = r - 1;
      launch_reduce_pass(a, st);
    }
    if (eff >= PRUNE && po.delta > 0) {  // the cut step
      HIP_TRY(reset());
      a.maxlen = maxlen;
      launch_prune_cut_round(a, st);
      a.maxlen = nullptr;
    }
    HIP_TRY(reset());  // the trim step, over what the cut step left
    if (eff >= PRUNE)
      launch_prune_trim_round(a, st);
    else
      launch_trim_round(a, st);
    if (eff >= BUBBLE) {
      HIP_TRY(reset());  // the bubble step, over what the trim step left
      launch_bubble_round(a, st);
    }
    if (eff >= INDEL) {
      HIP_TRY(reset());  // the indel step, over what the bubble step left
      launch_indel_round(a, st);
    }
    if (eff >= CHIMERIC && co.min_chimeric_length > 0) {
      HIP_TRY(reset());  // the chimeric step, over what the step before left
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
  if (red) {  // one more pass: a record whose only witnesses went in the last round is live again
    a.red_prev = last;
    launch_reduce_pass(a, st);
  }
  HIP_TRY(reset());
  if (eff >= PRUNE) {
    launch_unitigs_prune(a, st);
    launch_unitig_prune_lift(a, st);
  } else {
    launch_unitigs_trim(a, st);
    launch_unitig_lift(a, st);
  }
  if (eff >= CHIMERIC) launch_chimeric_status(a, st);
  if (eff >= BUBBLE) launch_bubble_status(a, st);
  if (eff >= INDEL) launch_indel_status(a, st);
  if (red) launch_reduce_status(a, st);
  HIP_TRY(hipGetLastError());
  for (int l = eff + 1; l <= level; ++l) {  // the steps that are off: their counts zero, and no record cut
    if (l == REDUCE && red) continue;
    HIP_TRY(hipMemsetAsync((u64*)b.status + status_words(l - 1), 0, (size_t)(status_words(l) - status_words(l - 1)) * 8, st));
    if (l == PRUNE && n_edges) HIP_TRY(hipMemsetAsync(b.cut, 0, (size_t)n_edges * 4, st));
  }
  return SIGAX_OK;
}

thread_local u64 t_last_status[6] = {0, 0, 0, 0, 0, 0};

// The reads and records of a host form on the device, in `g`: the offsets checked against the lengths, then (n > 0) the device
// chosen and the four arrays allocated and copied, the bases with 16 bytes of slack.  offs[0] need not be 0 (a window of a
// longer table): the device gets the window's bytes and offsets from 0.  *nb = the window's bytes.
int stage_reads(DevGuard& g, int device, const sigax_edge* edges, u64 n_edges, const uint32_t* lengths, const char* seqs, const uint64_t* offs, u64 n,
                UnitigBufs* b, u64* nb) {
  for (u64 i = 0; i < n; ++i)
    if (offs[i + 1] < offs[i] || offs[i + 1] - offs[i] != lengths[i]) return sigax_fail(SIGAX_E_ARG, "read %llu: offsets and length disagree", i);
  *nb = 0;
  if (n == 0) return SIGAX_OK;
  const u64 b0 = offs[0];
  *nb = offs[n] - b0;
  std::vector<uint64_t> rebased;
  if (b0) {
    rebased.resize((size_t)n + 1);
    for (u64 i = 0; i <= n; ++i) rebased[i] = offs[i] - b0;
    offs = rebased.data();
  }
  HIP_TRY(hipSetDevice(device));
  void *d_edges, *d_lengths, *d_seqs, *d_offs;
  HIP_TRY(g.alloc(&d_edges, (size_t)n_edges * sizeof(sigax_edge)));
  HIP_TRY(g.alloc(&d_lengths, (size_t)n * 4));
  HIP_TRY(g.alloc(&d_seqs, (size_t)*nb + 16));
  HIP_TRY(g.alloc(&d_offs, ((size_t)n + 1) * 8));
  if (n_edges) HIP_TRY(hipMemcpy(d_edges, edges, (size_t)n_edges * sizeof(sigax_edge), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_lengths, lengths, (size_t)n * 4, hipMemcpyHostToDevice));
  if (*nb) HIP_TRY(hipMemcpy(d_seqs, seqs + b0, (size_t)*nb, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(d_offs, offs, ((size_t)n + 1) * 8, hipMemcpyHostToDevice));
  b->edges = (const sigax_edge*)d_edges;
  b->lengths = d_lengths;
  b->seqs = d_seqs;
  b->offs = d_offs;
  return SIGAX_OK;
}

// The host form of every level.  UNITIG: no options, no removed, cut or uedges, six counts, and *layout holds all n_reads
// placements.  TRIM: no cut.  `status_out` holds status_words(level) counts.
int unitigs_host(Level level, int device, const sigax_edge* edges, uint64_t n_edges, const uint32_t* lengths, const char* seqs, const uint64_t* offs,
                 uint64_t n_reads, uint32_t min_overlap, const sigax_reduce_opts* opts, uint64_t* n_unitigs, uint64_t** seq_offs,
                 uint64_t** lay_offs, uint32_t** uflags, sigax_placement** layout, char** useqs, uint32_t** removed, uint32_t** cut,
                 sigax_edge** uedges, uint64_t* status_out) {
  const u64 n_status = status_words(level);
  if (!n_unitigs || !seq_offs || !lay_offs || !uflags || !layout || !status_out || (level >= TRIM && !removed) || (level >= PRUNE && !cut) ||
      (n_reads && (!lengths || !seqs || !offs)) || (n_edges && !edges))
    return sigax_fail(SIGAX_E_ARG, "NULL where a buffer is required");
  *n_unitigs = 0;
  *seq_offs = nullptr;
  *lay_offs = nullptr;
  *uflags = nullptr;
  *layout = nullptr;
  if (removed) *removed = nullptr;
  if (cut) *cut = nullptr;
  if (useqs) *useqs = nullptr;
  if (uedges) *uedges = nullptr;
  for (u64 k = 0; k < n_status; ++k) status_out[k] = 0;
  const int rl = unitig_limits(n_reads, n_edges);
  if (rl != SIGAX_OK) return rl;
  if (level >= TRIM) {
    const int ro = opts_ok(level, opts, n_reads, n_edges);
    if (ro != SIGAX_OK) return ro;
  }
  const u64 n = n_reads;
  u64 status[40] = {0};
  DevGuard g;
  UnitigBufs b = {};
  u64 nb = 0;
  const int rs = stage_reads(g, device, edges, n_edges, lengths, seqs, offs, n, &b, &nb);
  if (rs != SIGAX_OK) return rs;
  if (n) {
    b.work_bytes = rounds_work(level, n, n_edges, uedges != nullptr, level >= PRUNE && opts->indel.bubble.chimeric.prune.careful != 0).bytes;
    HIP_TRY(g.alloc(&b.seq_offs, ((size_t)n + 1) * 8));
    HIP_TRY(g.alloc(&b.lay_offs, ((size_t)n + 1) * 8));
    HIP_TRY(g.alloc(&b.uflags, (size_t)n * 4));
    HIP_TRY(g.alloc((void**)&b.layout, (size_t)n * sizeof(sigax_placement)));
    if (useqs) HIP_TRY(g.alloc(&b.useqs, (size_t)nb + 16));
    if (level >= TRIM) HIP_TRY(g.alloc(&b.removed, (size_t)n * 4));
    if (level >= PRUNE) HIP_TRY(g.alloc(&b.cut, (size_t)n_edges * 4 + 16));
    if (uedges) HIP_TRY(g.alloc((void**)&b.uedges, (size_t)n_edges * sizeof(sigax_edge) + 16));
    HIP_TRY(g.alloc(&b.status, (size_t)n_status * 8));
    HIP_TRY(g.alloc(&b.work, (size_t)b.work_bytes));
    const int rc = level == UNITIG ? sigax_unitigs_device(device, b.edges, n_edges, b.lengths, b.seqs, b.offs, n, min_overlap, b.seq_offs, b.lay_offs,
                                                          b.uflags, b.layout, b.useqs, b.status, b.work, b.work_bytes, nullptr)
                                   : unitigs_rounds(level, device, n_edges, n, min_overlap, opts, b, nullptr, true);
    if (rc != SIGAX_OK) return rc;
    HIP_TRY(hipMemcpy(status, b.status, (size_t)n_status * 8, hipMemcpyDeviceToHost));  // (waits for the null stream's kernels)
    if (status[0] > n || status[1] > nb || status[9] > n || status[11] > n_edges)
      return sigax_fail(SIGAX_E_DEVICE, "unitig counts beyond their buffers");
  }
  const u64 nu = status[0], bases = status[1], placed = n - status[9], ne = uedges ? status[11] : 0;
  HostGuard hg;
  uint64_t* h_so = hg.alloc<uint64_t>(((size_t)nu + 1) * 8);
  uint64_t* h_lo = hg.alloc<uint64_t>(((size_t)nu + 1) * 8);
  uint32_t* h_uf = hg.alloc<uint32_t>((size_t)nu * 4);
  sigax_placement* h_lay = hg.alloc<sigax_placement>((size_t)placed * sizeof(sigax_placement));
  char* h_us = useqs ? hg.alloc<char>((size_t)bases) : nullptr;
  uint32_t* h_rm = removed ? hg.alloc<uint32_t>((size_t)n * 4) : nullptr;
  uint32_t* h_ct = cut ? hg.alloc<uint32_t>((size_t)n_edges * 4) : nullptr;
  sigax_edge* h_ue = uedges ? hg.alloc<sigax_edge>((size_t)ne * sizeof(sigax_edge)) : nullptr;
  if (!hg.ok) return sigax_fail(SIGAX_E_CAPACITY, "out of host memory");
  h_so[0] = 0;
  h_lo[0] = 0;
  hipError_t e = hipSuccess;
  if (n) {
    e = hipMemcpy(h_so, b.seq_offs, ((size_t)nu + 1) * 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(h_lo, b.lay_offs, ((size_t)nu + 1) * 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess && nu) e = hipMemcpy(h_uf, b.uflags, (size_t)nu * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess && placed) e = hipMemcpy(h_lay, b.layout, (size_t)placed * sizeof(sigax_placement), hipMemcpyDeviceToHost);
    if (e == hipSuccess && useqs && bases) e = hipMemcpy(h_us, b.useqs, (size_t)bases, hipMemcpyDeviceToHost);
    if (e == hipSuccess && removed) e = hipMemcpy(h_rm, b.removed, (size_t)n * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess && cut && n_edges) e = hipMemcpy(h_ct, b.cut, (size_t)n_edges * 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess && ne) e = hipMemcpy(h_ue, b.uedges, (size_t)ne * sizeof(sigax_edge), hipMemcpyDeviceToHost);
  }
  if (e != hipSuccess) return sigax_fail(SIGAX_E_DEVICE, "copying the unitigs: %s", hipGetErrorString(e));
  if (cut && n == 0 && n_edges) memset(h_ct, 0, (size_t)n_edges * 4);
  for (u64 k = 0; k < n_status; ++k) status_out[k] = status[k];
  *n_unitigs = nu;
  *seq_offs = h_so;
  *lay_offs = h_lo;
  *uflags = h_uf;
  *layout = h_lay;
  if (removed) *removed = h_rm;
  if (cut) *cut = h_ct;
  if (useqs) *useqs = h_us;
  if (uedges) *uedges = h_ue;
  hg.release();
  return SIGAX_OK;
}

}  // namespace

extern "C" int sigax_unitigs_workspace(uint64_t n_reads, uint64_t n_edges, uint64_t* bytes) {
  return workspace_of(UNITIG, n_reads, n_edges, 0, 0, bytes);
}

extern "C" int sigax_unitigs_device(int device, const sigax_edge* d_edges, uint64_t n_edges, const void* d_lengths, const void* d_seqs,
                                    const void* d_offs, uint64_t n_reads, uint32_t min_overlap, void* d_seq_offs, void* d_lay_offs,
                                    void* d_uflags, sigax_placement* d_layout, void* d_useqs, void* d_status6, void* d_work,
                                    uint64_t work_bytes, void* stream) {
  const int rl = unitig_limits(n_reads, n_edges);
  if (rl != SIGAX_OK) return rl;
  const UnitigBufs b = {d_edges, d_lengths, d_seqs, d_offs, d_seq_offs, d_lay_offs, d_uflags, d_layout, d_useqs, nullptr, nullptr, nullptr,
                        d_status6, d_work, work_bytes};
  const RoundsWork w = rounds_work(UNITIG, n_reads, n_edges, false, false);
  if (n_reads) {
    const int rb = bufs_ok(UNITIG, b, n_edges, w);
    if (rb != SIGAX_OK) return rb;
  }
  HIP_TRY(hipSetDevice(device));
  const hipStream_t st = (hipStream_t)stream;
  if (n_reads == 0) {
    if (d_status6) HIP_TRY(hipMemsetAsync(d_status6, 0, 48, st));
    return SIGAX_OK;
  }
  const UnitigArgs a = unitig_args(b, w, n_edges, n_reads, min_overlap);
  HIP_TRY(hipMemsetAsync((char*)d_work + w.zero_from, 0, (size_t)w.zero_bytes, st));
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
  const RoundsWork w = rounds_work(UNITIG, n_reads, n_edges, false, false);
  if (n_reads && work_bytes < w.bytes) return sigax_fail(SIGAX_E_ARG, "workspace too small (sigax_unitigs_workspace)");
  HIP_TRY(hipSetDevice(device));
  if (n_reads == 0) return SIGAX_OK;
  UnitigBufs b = {};
  b.seqs = d_seqs;
  b.offs = d_offs;
  b.useqs = d_useqs;
  b.work = d_work;
  launch_unitig_bases(unitig_args(b, w, n_edges, n_reads, 0), (hipStream_t)stream);
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
  uint64_t status[6];
  const int rc = unitigs_host(UNITIG, device, edges, n_edges, lengths, seqs, offs, n_reads, min_overlap, nullptr, n_unitigs, seq_offs, lay_offs,
                              uflags, layout, useqs, nullptr, nullptr, nullptr, status);
  if (rc != SIGAX_OK) return rc;
  for (int k = 0; k < 6; ++k) t_last_status[k] = status[k];
  return SIGAX_OK;
}

// ---- the rounds calls: tip trimming and the lifted records, non-maximal overlap cutting, chimeric unitig removal, bubble
// popping, indel bubble popping, transitive reduction.  Each is the driver at its level over its options seen as the reduce call's. ----
#define SIGAX_ROUNDS_DEVICE(LEVEL, OPTS, CUT)                                                                                          \
  sigax_reduce_opts v;                                                                                                                 \
  const UnitigBufs b = {d_edges, d_lengths, d_seqs, d_offs, d_seq_offs, d_lay_offs, d_uflags, d_layout, d_useqs, d_removed, CUT, d_uedges, \
                        d_status, d_work, work_bytes};                                                                                 \
  return unitigs_rounds(LEVEL, device, n_edges, n_reads, min_overlap, opts_view(OPTS, &v), b, stream, false)
#define SIGAX_ROUNDS_HOST(LEVEL, OPTS, CUT)                                                                                              \
  sigax_reduce_opts v;                                                                                                                 \
  return unitigs_host(LEVEL, device, edges, n_edges, lengths, seqs, offs, n_reads, min_overlap, opts_view(OPTS, &v), n_unitigs, seq_offs, \
                      lay_offs, uflags, layout, useqs, removed, CUT, uedges, status)

extern "C" int sigax_unitigs_trim_workspace(uint64_t n_reads, uint64_t n_edges, int want_graph, uint64_t* bytes) {
  return workspace_of(TRIM, n_reads, n_edges, want_graph, 0, bytes);
}
extern "C" int sigax_unitigs_trim_device(int device, const sigax_edge* d_edges, uint64_t n_edges, const void* d_lengths, const void* d_seqs,
                                         const void* d_offs, uint64_t n_reads, uint32_t min_overlap, const sigax_trim_opts* opts,
                                         void* d_seq_offs, void* d_lay_offs, void* d_uflags, sigax_placement* d_layout, void* d_useqs,
                                         void* d_removed, sigax_edge* d_uedges, void* d_status, void* d_work, uint64_t work_bytes,
                                         void* stream) {
  SIGAX_ROUNDS_DEVICE(TRIM, opts, nullptr);
}
extern "C" int sigax_unitigs_trim_host(int device, const sigax_edge* edges, uint64_t n_edges, const uint32_t* lengths, const char* seqs,
                                       const uint64_t* offs, uint64_t n_reads, uint32_t min_overlap, const sigax_trim_opts* opts,
                                       uint64_t* n_unitigs, uint64_t** seq_offs, uint64_t** lay_offs, uint32_t** uflags,
                                       sigax_placement** layout, char** useqs, uint32_t** removed, sigax_edge** uedges, uint64_t status[12]) {
  SIGAX_ROUNDS_HOST(TRIM, opts, nullptr);
}

extern "C" int sigax_unitigs_prune_workspace(uint64_t n_reads, uint64_t n_edges, int want_graph, int careful, uint64_t* bytes) {
  return workspace_of(PRUNE, n_reads, n_edges, want_graph, careful, bytes);
}
extern "C" int sigax_unitigs_prune_device(int device, const sigax_edge* d_edges, uint64_t n_edges, const void* d_lengths, const void* d_seqs,
                                          const void* d_offs, uint64_t n_reads, uint32_t min_overlap, const sigax_prune_opts* opts,
                                          void* d_seq_offs, void* d_lay_offs, void* d_uflags, sigax_placement* d_layout, void* d_useqs,
                                          void* d_removed, void* d_cut, sigax_edge* d_uedges, void* d_status, void* d_work,
                                          uint64_t work_bytes, void* stream) {
  SIGAX_ROUNDS_DEVICE(PRUNE, opts, d_cut);
}
extern "C" int sigax_unitigs_prune_host(int device, const sigax_edge* edges, uint64_t n_edges, const uint32_t* lengths, const char* seqs,
                                        const uint64_t* offs, uint64_t n_reads, uint32_t min_overlap, const sigax_prune_opts* opts,
                                        uint64_t* n_unitigs, uint64_t** seq_offs, uint64_t** lay_offs, uint32_t** uflags,
                                        sigax_placement** layout, char** useqs, uint32_t** removed, uint32_t** cut, sigax_edge** uedges,
                                        uint64_t status[16]) {
  SIGAX_ROUNDS_HOST(PRUNE, opts, cut);
}

extern "C" int sigax_unitigs_chimeric_workspace(uint64_t n_reads, uint64_t n_edges, int want_graph, int careful, uint64_t* bytes) {
  return workspace_of(CHIMERIC, n_reads, n_edges, want_graph, careful, bytes);
}
extern "C" int sigax_unitigs_chimeric_device(int device, const sigax_edge* d_edges, uint64_t n_edges, const void* d_lengths, const void* d_seqs,
                                             const void* d_offs, uint64_t n_reads, uint32_t min_overlap, const sigax_chimeric_opts* opts,
                                             void* d_seq_offs, void* d_lay_offs, void* d_uflags, sigax_placement* d_layout, void* d_useqs,
                                             void* d_removed, void* d_cut, sigax_edge* d_uedges, void* d_status, void* d_work,
                                             uint64_t work_bytes, void* stream) {
  SIGAX_ROUNDS_DEVICE(CHIMERIC, opts, d_cut);
}
extern "C" int sigax_unitigs_chimeric_host(int device, const sigax_edge* edges, uint64_t n_edges, const uint32_t* lengths, const char* seqs,
                                           const uint64_t* offs, uint64_t n_reads, uint32_t min_overlap, const sigax_chimeric_opts* opts,
                                           uint64_t* n_unitigs, uint64_t** seq_offs, uint64_t** lay_offs, uint32_t** uflags,
                                           sigax_placement** layout, char** useqs, uint32_t** removed, uint32_t** cut, sigax_edge** uedges,
                                           uint64_t status[20]) {
  SIGAX_ROUNDS_HOST(CHIMERIC, opts, cut);
}

extern "C" int sigax_unitigs_bubble_workspace(uint64_t n_reads, uint64_t n_edges, int want_graph, int careful, uint64_t* bytes) {
  return workspace_of(BUBBLE, n_reads, n_edges, want_graph, careful, bytes);
}
extern "C" int sigax_unitigs_bubble_device(int device, const sigax_edge* d_edges, uint64_t n_edges, const void* d_lengths, const void* d_seqs,
                                           const void* d_offs, uint64_t n_reads, uint32_t min_overlap, const sigax_bubble_opts* opts,
                                           void* d_seq_offs, void* d_lay_offs, void* d_uflags, sigax_placement* d_layout, void* d_useqs,
                                           void* d_removed, void* d_cut, sigax_edge* d_uedges, void* d_status, void* d_work,
                                           uint64_t work_bytes, void* stream) {
  SIGAX_ROUNDS_DEVICE(BUBBLE, opts, d_cut);
}
extern "C" int sigax_unitigs_bubble_host(int device, const sigax_edge* edges, uint64_t n_edges, const uint32_t* lengths, const char* seqs,
                                         const uint64_t* offs, uint64_t n_reads, uint32_t min_overlap, const sigax_bubble_opts* opts,
                                         uint64_t* n_unitigs, uint64_t** seq_offs, uint64_t** lay_offs, uint32_t** uflags,
                                         sigax_placement** layout, char** useqs, uint32_t** removed, uint32_t** cut, sigax_edge** uedges,
                                         uint64_t status[24]) {
  SIGAX_ROUNDS_HOST(BUBBLE, opts, cut);
}

extern "C" int sigax_unitigs_indel_workspace(uint64_t n_reads, uint64_t n_edges, int want_graph, int careful, uint64_t* bytes) {
  return workspace_of(INDEL, n_reads, n_edges, want_graph, careful, bytes);
}
extern "C" int sigax_unitigs_indel_device(int device, const sigax_edge* d_edges, uint64_t n_edges, const void* d_lengths, const void* d_seqs,
                                          const void* d_offs, uint64_t n_reads, uint32_t min_overlap, const sigax_indel_opts* opts,
                                          void* d_seq_offs, void* d_lay_offs, void* d_uflags, sigax_placement* d_layout, void* d_useqs,
                                          void* d_removed, void* d_cut, sigax_edge* d_uedges, void* d_status, void* d_work,
                                          uint64_t work_bytes, void* stream) {
  SIGAX_ROUNDS_DEVICE(INDEL, opts, d_cut);
}
extern "C" int sigax_unitigs_indel_host(int device, const sigax_edge* edges, uint64_t n_edges, const uint32_t* lengths, const char* seqs,
                                        const uint64_t* offs, uint64_t n_reads, uint32_t min_overlap, const sigax_indel_opts* opts,
                                        uint64_t* n_unitigs, uint64_t** seq_offs, uint64_t** lay_offs, uint32_t** uflags,
                                        sigax_placement** layout, char** useqs, uint32_t** removed, uint32_t** cut, sigax_edge** uedges,
                                        uint64_t status[32]) {
  SIGAX_ROUNDS_HOST(INDEL, opts, cut);
}

extern "C" int sigax_unitigs_reduce_workspace(uint64_t n_reads, uint64_t n_edges, int want_graph, int careful, uint64_t* bytes) {
  return workspace_of(REDUCE, n_reads, n_edges, want_graph, careful, bytes);
}
extern "C" int sigax_unitigs_reduce_device(int device, const sigax_edge* d_edges, uint64_t n_edges, const void* d_lengths, const void* d_seqs,
                                           const void* d_offs, uint64_t n_reads, uint32_t min_overlap, const sigax_reduce_opts* opts,
                                           void* d_seq_offs, void* d_lay_offs, void* d_uflags, sigax_placement* d_layout, void* d_useqs,
                                           void* d_removed, void* d_cut, sigax_edge* d_uedges, void* d_status, void* d_work,
                                           uint64_t work_bytes, void* stream) {
  SIGAX_ROUNDS_DEVICE(REDUCE, opts, d_cut);
}
extern "C" int sigax_unitigs_reduce_host(int device, const sigax_edge* edges, uint64_t n_edges, const uint32_t* lengths, const char* seqs,
                                         const uint64_t* offs, uint64_t n_reads, uint32_t min_overlap, const sigax_reduce_opts* opts,
                                         uint64_t* n_unitigs, uint64_t** seq_offs, uint64_t** lay_offs, uint32_t** uflags,
                                         sigax_placement** layout, char** useqs, uint32_t** removed, uint32_t** cut, sigax_edge** uedges,
                                         uint64_t status[40]) {
  SIGAX_ROUNDS_HOST(REDUCE, opts, cut);
}
