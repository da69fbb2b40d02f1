// siga_amd/csrc/sigax_api.cpp -- include/sigax.h: the batch object -- its device workspaces and the launch sequence of the
// overlap path (enqueue), runs, results.  The index it runs on: sigax_index.cpp, sigax_tables.cpp.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "sigax_internal.h"

// Slots per chain of the candidate arena for reads of up to max_len bases.  Worst case: overlaps of length max(m,1)..L-1,
// plus one for the containment block.  Given: what the longest chain so far needed plus headroom -- or, before any run has
// finished, a third of the worst case -- never more than the worst case, never less than `floor_slots` records.  Even:
// each chain's slots start on a 64-byte line (k_find's quad stores write whole lines).
static uint32_t worst_cap(uint32_t max_len, uint32_t minov) {
  const uint32_t mm = std::max<uint32_t>(minov, 1u);
  const uint32_t cap = (max_len > mm ? max_len - mm : 0u) + 1u;
  return (cap + 1u) & ~1u;
}
static uint32_t chain_cap(const sigax_index* ix, uint32_t max_len, uint32_t minov, uint32_t floor_slots) {
  const uint32_t worst = worst_cap(max_len, minov);
  const Settings& cfg = settings();  // SIGAX_CAND_CAP: "worst" = the round-2 sizing; a number = slots of the first try (tests)
  if (cfg.cand_cap_worst) return worst;
  const uint32_t seen = ix->cap_seen->load();
  uint32_t want = seen ? seen + seen / 8 + 3 : (cfg.cand_cap ? (uint32_t)*cfg.cand_cap : std::max<uint32_t>(worst / 3, 16u));
  want = std::max(want, floor_slots + 1u);  // + the containment slot
  want = (want + 1u) & ~1u;
  return std::min(worst, std::max(want, 2u));
}

// ------------------------------------------------------------------------------------------------------
// batch workspace
// ------------------------------------------------------------------------------------------------------
struct DevBuf {
  void* p;
  size_t bytes;
  DevBuf() : p(nullptr), bytes(0) {}
};

static int ensure(DevBuf* b, size_t bytes) {
  if (bytes <= b->bytes && b->p) return SIGAX_OK;
  if (b->p) hipFree(b->p);
  b->p = nullptr;
  b->bytes = 0;
  size_t want = bytes ? bytes : 16;
  hipError_t e = hipMalloc(&b->p, want);
  if (e != hipSuccess) return sigax_fail(SIGAX_E_DEVICE, "hipMalloc(%zu bytes): %s", want, hipGetErrorString(e));
  b->bytes = want;
  return SIGAX_OK;
}

enum { EV_START = 0, EV_FX_DONE, EV_ORDER, EV_EDGES, EV_ORD0, EV_ORD1, EV_BLOCKS, EV_COUNT };
// per sub-batch: find begin/end on the find stream, fast begin/end and general end on the filter/extract stream
enum { SV_F0 = 0, SV_F1, SV_X0, SV_X1, SV_G1, SV_COUNT };

struct sigax_batch {
  sigax_index* ix;
  uint32_t max_reads;
  u64 max_bases;
  uint32_t max_len;
  DevBuf seqs_own, offs_own;
  const unsigned char* d_seqs;
  const u64* d_offs;
  uint32_t n_reads;
  u64 n_bases;
  uint32_t cur_max_len;
  // parameters of the last run (for the regrow-and-rerun loop)
  uint32_t read_base, minov, flags;
  const uint32_t* d_ids;  // the reads' ids in the index's read table, or NULL: read_base + r (sigax_batch_set_device_read_ids)
  uint32_t ids_n;         // ... for this many reads
  bool ran;
  // arenas
  DevBuf ids_own;  // sigax_batch_upload_read_ids
  DevBuf arena, chain_cnt, pool, wpool, work, work64, work64b, work64c, work64d, perm, ord_keys, ord_tmp, occ_side, slow_flag, offs2, item_base, fin, fin_cnt, substring, block_offs, outb, edge_cnt,
      edge_offs, edges, partial, dstat;
  uint32_t cap;
  uint32_t cap_floor;  // records the longest chain of this batch's last (overflowed) run needed
  uint32_t pool_cap;
  unsigned fx_grid;
  u64 fin_cap, edge_cap;
  bool fin_grown;
  u64 n_reruns;  // runs repeated because an arena was too small
  hipEvent_t ev[EV_COUNT];
  hipEvent_t sev[SIGAX_MAX_SUB][SV_COUNT];
  unsigned nsub;
  bool perm_valid;    // `perm_cur` (one half of `perm`) holds the locality order of the reads now set, for perm_nsub sub-batches
  const uint32_t* perm_cur;
  unsigned perm_nsub;
  u64 qhint[4];       // items per sub-batch in the four filter/extract queues in the previous run (~0: none yet)
  bool qhint_lean_off;  // ... measured with lean_off in this state
  bool lean_off;      // see sigax_batch_finish
  bool fx_heavy;      // the last run's filter/extract launches took longer than its finder launches (sigax_batch_finish)
  // which finder between 2^30 and 2^31 symbols (want_coop): 0, 1 = per-lane runs (the second one timed), 2, 3 = cooperative runs
  // (the second one timed), 4 = decided
  int coop_tune;
  float coop_t_lane;
  bool coop_pick;
  unsigned lean_off_runs;
  unsigned nsub_req;  // 0 = automatic
  unsigned find_per_sub;  // finder launches per sub-batch (2 = one per strand's two-step table)
  bool last_two_step, last_coop, last_perm, last_ordered;  // what the last enqueued run's finder did (sigax_batch_run_info)
  uint32_t last_deep_k;
  sigax_stats last;
  u64 last_total_blocks, last_total_edges;
  bool finished;
  bool blocks_ordered;  // outb holds the last enqueued run's ordered blocks (order_blocks)
};

// every device buffer a batch object owns
template <class F>
static void each_buffer(sigax_batch* b, F f) {
  DevBuf* all[] = {&b->ids_own, &b->seqs_own, &b->offs_own, &b->arena, &b->chain_cnt, &b->pool, &b->wpool, &b->work, &b->work64, &b->work64b, &b->work64c, &b->work64d, &b->perm,
                   &b->ord_keys, &b->ord_tmp, &b->occ_side, &b->slow_flag, &b->offs2, &b->item_base, &b->fin, &b->fin_cnt, &b->substring, &b->block_offs,
                   &b->outb, &b->edge_cnt, &b->edge_offs, &b->edges, &b->partial, &b->dstat};
  for (DevBuf* d : all) f(d);
}

extern "C" void sigax_batch_destroy(sigax_batch* b) {
  if (!b) return;
  hipSetDevice(b->ix->device);
  each_buffer(b, [](DevBuf* d) {
    if (d->p) hipFree(d->p);
  });
  for (int i = 0; i < EV_COUNT; ++i)
    if (b->ev[i]) hipEventDestroy(b->ev[i]);
  for (int i = 0; i < SIGAX_MAX_SUB; ++i)
    for (int j = 0; j < SV_COUNT; ++j)
      if (b->sev[i][j]) hipEventDestroy(b->sev[i][j]);
  delete b;
}

extern "C" int sigax_batch_create(sigax_index* ix, uint32_t max_reads, uint64_t max_bases, uint32_t max_read_len,
                                  sigax_batch** out) {
  if (!ix || !out) return sigax_fail(SIGAX_E_ARG, "NULL argument");
  *out = nullptr;
  HIP_TRY(hipSetDevice(ix->device));
  sigax_batch* b = new sigax_batch();
  b->ix = ix;
  b->max_reads = max_reads;
  b->max_bases = max_bases;
  b->max_len = max_read_len;
  b->d_seqs = nullptr;
  b->d_offs = nullptr;
  b->n_reads = 0;
  b->n_bases = 0;
  b->cur_max_len = 0;
  b->read_base = b->minov = b->flags = 0;
  b->d_ids = nullptr;
  b->ids_n = 0;
  b->ran = b->finished = b->blocks_ordered = false;
  b->cap = 0;
  b->cap_floor = 0;
  b->pool_cap = 0;
  b->fx_grid = 0;
  b->fin_cap = b->edge_cap = 0;
  b->fin_grown = false;
  b->n_reruns = 0;
  memset(&b->last, 0, sizeof(b->last));
  b->last_total_blocks = b->last_total_edges = 0;
  for (int i = 0; i < EV_COUNT; ++i) b->ev[i] = nullptr;
  for (int i = 0; i < SIGAX_MAX_SUB; ++i)
    for (int j = 0; j < SV_COUNT; ++j) b->sev[i][j] = nullptr;
  b->nsub = 1;
  b->lean_off = false;
  b->lean_off_runs = 0;
  b->fx_heavy = false;
  b->coop_tune = 0;
  b->coop_t_lane = 0.f;
  b->coop_pick = false;
  b->qhint[0] = b->qhint[1] = b->qhint[2] = b->qhint[3] = ~0ull;
  b->qhint_lean_off = false;
  b->perm_valid = false;
  b->perm_cur = nullptr;
  b->perm_nsub = 0;
  b->nsub_req = 0;
  b->find_per_sub = 1;
  b->last_two_step = b->last_coop = b->last_perm = b->last_ordered = false;
  b->last_deep_k = 0;
  {
    hipError_t e = hipSuccess;
    for (int i = 0; i < EV_COUNT && e == hipSuccess; ++i) e = hipEventCreate(&b->ev[i]);
    for (int i = 0; i < SIGAX_MAX_SUB && e == hipSuccess; ++i)
      for (int j = 0; j < SV_COUNT && e == hipSuccess; ++j) e = hipEventCreate(&b->sev[i][j]);
    if (e != hipSuccess) {
      sigax_batch_destroy(b);
      return sigax_fail(SIGAX_E_DEVICE, "creating events/streams: %s", hipGetErrorString(e));
    }
  }
  int rc = ensure(&b->dstat, DS_COUNT * 8);
  if (rc != SIGAX_OK) {
    sigax_batch_destroy(b);
    return rc;
  }
  *out = b;
  return SIGAX_OK;
}

extern "C" int sigax_batch_upload(sigax_batch* b, const char* seqs, const uint64_t* offs, uint32_t n_reads, void* stream) {
  if (!b || (n_reads && (!seqs || !offs))) return sigax_fail(SIGAX_E_ARG, "NULL argument");
  HIP_TRY(hipSetDevice(b->ix->device));
  hipStream_t st = (hipStream_t)stream;
  u64 nb = n_reads ? offs[n_reads] - offs[0] : 0;
  if (n_reads && offs[0] != 0) return sigax_fail(SIGAX_E_ARG, "offs[0] must be 0");
  uint32_t mx = 0;
  for (uint32_t i = 0; i < n_reads; ++i) {
    u64 l = offs[i + 1] - offs[i];
    if (offs[i + 1] < offs[i] || l > 0x0FFFFFFFull) return sigax_fail(SIGAX_E_ARG, "bad offsets at read %u", i);
    mx = std::max<uint32_t>(mx, (uint32_t)l);
  }
  int rc = ensure(&b->seqs_own, nb + 16);
  if (rc == SIGAX_OK) rc = ensure(&b->offs_own, ((size_t)n_reads + 1) * 8);
  if (rc != SIGAX_OK) return rc;
  if (nb) HIP_TRY(hipMemcpyAsync(b->seqs_own.p, seqs, nb, hipMemcpyHostToDevice, st));
  static const u64 zero = 0;
  HIP_TRY(hipMemcpyAsync(b->offs_own.p, n_reads ? (const void*)offs : (const void*)&zero, ((size_t)n_reads + 1) * 8,
                         hipMemcpyHostToDevice, st));
  b->d_seqs = (const unsigned char*)b->seqs_own.p;
  b->d_offs = (const u64*)b->offs_own.p;
  b->n_reads = n_reads;
  b->n_bases = nb;
  b->cur_max_len = mx;
  b->perm_valid = false;
  b->ran = b->finished = false;
  return SIGAX_OK;
}

extern "C" int sigax_batch_set_device_reads(sigax_batch* b, const void* d_seqs, const void* d_offs, uint32_t n_reads,
                                            uint64_t n_bases, uint32_t max_len) {
  if (!b || (n_reads && (!d_seqs || !d_offs))) return sigax_fail(SIGAX_E_ARG, "NULL argument");
  b->d_seqs = (const unsigned char*)d_seqs;
  b->d_offs = (const u64*)d_offs;
  b->n_reads = n_reads;
  b->n_bases = n_bases;
  b->cur_max_len = max_len;
  b->perm_valid = false;
  b->ran = b->finished = false;
  return SIGAX_OK;
}

// Cooperative or per-lane finder for this run?  The cooperative one (lines through LDS, eight lanes per line: one address
// translation) wherever the per-lane finder's 32-bit byte offsets do not reach (2^31 symbols; 64-bit positions); the per-lane
// one below 2^30 symbols.  In between it depends on what the library cannot see -- how local the batch's reads are: one
// rank's view of the 4-GPU job of bench.py, 1.51e9 symbols: file-range shard 117.6 M reads/s per lane against 111.0 M
// cooperative, key-range shard 132-134 M against 138-139 M (profiles/r04_key_sharding.txt) -- so a batch object measures:
// two runs per lane, two cooperative, the second of each timed (its finder launches' own durations, as they ran), then it
// keeps the faster.  SIGAX_FIND_COOP / SIGAX_COOP_MIN_SYMBOLS decide statically as before; SIGAX_COOP_TUNE_MIN moves the
// lower end of the measured range (tests: 0 = every index).
static bool coop_tunable(const sigax_index* ix) {
  const Settings& cfg = settings();
  if (cfg.find_coop.has_value() || cfg.coop_min_symbols.has_value() || ix->wide) return false;
  return ix->n_symbols >= cfg.coop_tune_min && ix->n_symbols < (1ull << 31);
}
static bool want_coop(const sigax_index* ix, const sigax_batch* b) {
  const Settings& cfg = settings();
  if (cfg.find_coop.has_value()) return *cfg.find_coop;
  if (ix->wide || ix->n_symbols >= cfg.coop_min_symbols.value_or(1ull << 31)) return true;
  if (!coop_tunable(ix)) return false;
  return b->coop_tune >= 4 ? b->coop_pick : b->coop_tune >= 2;
}

extern "C" int sigax_batch_set_device_read_ids(sigax_batch* b, const void* d_ids, uint32_t n_reads) {
  if (!b) return sigax_fail(SIGAX_E_ARG, "NULL batch");
  if ((d_ids != nullptr) != (b->d_ids != nullptr)) b->coop_tune = 0;  // another kind of shard: measure the finders again (want_coop)
  b->d_ids = (const uint32_t*)d_ids;
  b->ids_n = d_ids ? n_reads : 0;
  b->ran = b->finished = false;
  return SIGAX_OK;
}

extern "C" int sigax_batch_upload_read_ids(sigax_batch* b, const uint32_t* ids, uint32_t n_reads, void* stream) {
  if (!b || (n_reads && !ids)) return sigax_fail(SIGAX_E_ARG, "NULL argument");
  HIP_TRY(hipSetDevice(b->ix->device));
  for (uint32_t i = 0; i < n_reads; ++i)
    if (ids[i] >= b->ix->n_strings) return sigax_fail(SIGAX_E_ARG, "read id %u (entry %u) is beyond the %llu indexed reads", ids[i], i, (unsigned long long)b->ix->n_strings);
  int rc = ensure(&b->ids_own, ((size_t)n_reads + 1) * 4);
  if (rc != SIGAX_OK) return rc;
  HIP_TRY(hipMemcpyAsync(b->ids_own.p, ids, (size_t)n_reads * 4, hipMemcpyHostToDevice, (hipStream_t)stream));
  return sigax_batch_set_device_read_ids(b, n_reads ? b->ids_own.p : nullptr, n_reads);
}

// ---- the stages of enqueue() ----

// The batch's arenas for this run (they grow, never shrink) and the grid of the fast filter/extract kernel
static int size_arenas(sigax_batch* b, bool edges, unsigned* fast_grid_out) {
  sigax_index* ix = b->ix;
  const Settings& cfg = settings();
  const uint32_t n = b->n_reads;
  b->cap = chain_cap(ix, b->cur_max_len, b->minov, b->cap_floor);
  int rc;
  if ((rc = ensure(&b->arena, (size_t)n * 4 * b->cap * cand_bytes(ix->wide))) != SIGAX_OK) return rc;
  if ((rc = ensure(&b->chain_cnt, (size_t)n * 4 * 4)) != SIGAX_OK) return rc;
  if ((rc = ensure(&b->fin_cnt, (2 * (size_t)n + 2) * 4)) != SIGAX_OK) return rc;
  if ((rc = ensure(&b->occ_side, (2 * (size_t)n + 2) * 4)) != SIGAX_OK) return rc;
  if ((rc = ensure(&b->slow_flag, ((size_t)n + 1) * 4)) != SIGAX_OK) return rc;
  if ((rc = ensure(&b->offs2, (2 * (size_t)n + 4) * 8)) != SIGAX_OK) return rc;
  if ((rc = ensure(&b->substring, (size_t)n + 16)) != SIGAX_OK) return rc;
  if ((rc = ensure(&b->block_offs, ((size_t)n + 2) * 8)) != SIGAX_OK) return rc;
  // fast filter/extract kernel: persistent waves (one read at a time per wave) with a private pool each
  // Three workgroups per CU: all of them are resident beside the finder's two (register file: 2 x 64 + 3 x 128 per
  // SIMD), so no filter/extract workgroup is left waiting to take the slot a finished finder workgroup frees.
  // (round 4: 2.5 per CU beside the per-lane finder's three workgroups -- two fit a CU's LDS beside them, the rest queue --;
  // 3 per CU beside the cooperative finder as before)
  const bool coop_idx = want_coop(ix, b);
  // ... and 3 per CU again for a batch object whose last run waited for filter/extract rather than for the finder (reads
  // with sequencing errors: fx_heavy, see sigax_batch_finish).  tools/sweep_env.sh, BASELINE configs[1] shape, 2.5 against 3
  // per CU: no errors 155.9 / 153.6 M reads/s, 0.03 % substitutions 138.7 / 144.7, 0.1 % 121.7 / 121.9, 0.3 % 93.7 / 98.0,
  // 1 % 66.7 / 76.7 (profiles/r04_error_rates.txt).
  const unsigned grid_max = 3u * (unsigned)ix->n_cu;
  unsigned fast_grid = (unsigned)std::min<u64>(cfg.fx_grid ? (u64)*cfg.fx_grid : ((coop_idx || b->fx_heavy) ? grid_max : 5u * (unsigned)ix->n_cu / 2u), ((u64)n + 3) / 4);  // two items per wave
  if (fast_grid == 0) fast_grid = 1;
  // (the pools are sized for the larger grid: a change of mind costs no allocation)
  if ((rc = ensure(&b->wpool, (size_t)std::max(fast_grid, std::min<unsigned>(grid_max, (unsigned)(((u64)n + 3) / 4))) * 4 * fast_pool_entries_per_wave() * SIGAX_ENT_BYTES)) != SIGAX_OK) return rc;
  if ((rc = ensure(&b->work, ((size_t)n + 1) * 4)) != SIGAX_OK) return rc;
  if ((rc = ensure(&b->work64, (2 * (size_t)n + 2) * 4)) != SIGAX_OK) return rc;
  if ((rc = ensure(&b->work64b, (2 * (size_t)n + 2) * 4)) != SIGAX_OK) return rc;
  if ((rc = ensure(&b->work64c, (2 * (size_t)n + 2) * 4)) != SIGAX_OK) return rc;
  if ((rc = ensure(&b->work64d, (2 * (size_t)n + 2) * 4)) != SIGAX_OK) return rc;
  // general filter/extract kernel (reads the fast kernel queued): persistent lanes with a private pool each
  unsigned want_grid = (unsigned)std::min<u64>(128, ((u64)n + 255) / 256);
  if (want_grid == 0) want_grid = 1;
  // SIGAX_TEST_{POOL,FIN,EDGE}_CAP: tiny first sizes, so that tests reach the grow-and-rerun loop of sigax_batch_finish
  uint32_t want_pool = std::max<uint32_t>(b->pool_cap, cfg.test_pool_cap ? (uint32_t)*cfg.test_pool_cap : 4u * (b->cap + 2u) + 128u);
  b->fx_grid = want_grid;
  b->pool_cap = want_pool;
  if ((rc = ensure(&b->pool, (size_t)want_grid * 256 * want_pool * SIGAX_ENT_BYTES)) != SIGAX_OK) return rc;
  // the unordered arena is handed out in chunks (one atomic per chunk): leave room for every wave's / lane's tail
  u64 chunk_slack = (u64)fast_grid * 4 * fast_fin_chunk() + (u64)want_grid * 256 * 64 + 1024;
  u64 want_fin = ((b->flags & SIGAX_IRREDUCIBLE) ? (u64)n * 8 : (u64)n * 64) + chunk_slack;
  if (cfg.test_fin_cap) want_fin = std::max<u64>(*cfg.test_fin_cap, 1);
  b->fin_cap = std::max<u64>(b->fin_cap, want_fin);
  if ((rc = ensure(&b->fin, b->fin_cap * sizeof(sigax_block))) != SIGAX_OK) return rc;
  if ((rc = ensure(&b->outb, b->fin_cap * sizeof(sigax_block))) != SIGAX_OK) return rc;
  if ((rc = ensure(&b->item_base, (2 * (size_t)n + 2) * 8)) != SIGAX_OK) return rc;
  u64 scan_n = std::max<u64>(2 * (u64)n, b->fin_cap);
  if ((rc = ensure(&b->partial, scan_partials_needed(scan_n) * 8)) != SIGAX_OK) return rc;
  if (edges) {
    if (b->edge_cap == 0) b->edge_cap = cfg.test_edge_cap ? std::max<u64>(*cfg.test_edge_cap, 1) : b->fin_cap * 2 + 1024;
    if ((rc = ensure(&b->edge_cnt, (2 * (size_t)n + 2) * 4)) != SIGAX_OK) return rc;
    if ((rc = ensure(&b->edge_offs, (2 * (size_t)n + 4) * 8)) != SIGAX_OK) return rc;
    if ((rc = ensure(&b->edges, b->edge_cap * sizeof(sigax_edge))) != SIGAX_OK) return rc;
  }
  *fast_grid_out = fast_grid;
  return SIGAX_OK;
}

// bytes per read in the finder's LDS copy of its workgroup's reads under the locality order
static uint32_t perm_stride(const sigax_batch* b) { return (b->cur_max_len + 3u) & ~3u; }

// Locality order of the reads for the per-lane finder (sigax_order_reads): once per set of reads and sub-batch count,
// on the caller's stream behind the upload (no host wait: the pipeline streams start behind EV_START); only where the
// workgroup's reads are staged in LDS by slot (the longest read decides).
// SIGAX_READ_ORDER=0 turns it off.
static int locality_order(sigax_batch* b, hipStream_t st, const uint32_t** d_perm) {
  sigax_index* ix = b->ix;
  const uint32_t n = b->n_reads;
  const unsigned nsub = b->nsub;
  b->last_ordered = false;
  const uint32_t stride = perm_stride(b);
  // Off unless SIGAX_READ_ORDER=1.  Measured with the ordering inside the timed step, as every product batch pays it:
  // BASELINE configs[1] 107-111 M reads/s with it against 119-121 M without (the table is cache-resident there and the
  // order buys the finder 1 to 5 %); the configs[2] shape 87.2 / 89.3 M against 90.9 / 89.6 M (3.75-fold coverage inside a
  // batch: the finder gains 0.4 ms of 26.7, the batch's chain gets 7 ms longer); the configs[4] shape 35.7 against 38.8 M
  // (a batch covers the genome 1.1 times: hardly any read has a neighbour in its batch).  What reads in GENOME order are
  // worth (+14 % / +23 %) needs them sorted by position inside a class too -- round 2's full radix sort got
  // the configs[2] finder from 26.9 to 22.4 ms -- and that costs twenty dependent launches on a GPU the other batches
  // keep full: 17 to 40 ms on the batch's chain.  Kept as an option for callers whose batches are deep.
  const bool coop_would = (ix->st[0].gran2 && ix->st[1].gran2) && want_coop(ix, b) && 32ull * stride + 32 <= 32768;
  if (!settings().read_order || n < 2 || !(coop_would || 128ull * stride + 8 <= find_stage_capacity(b->cur_max_len))) return SIGAX_OK;
  if (!b->perm_valid || b->perm_nsub != nsub) {
    HIP_TRY(hipEventRecord(b->ev[EV_ORD0], st));  // behind the upload of the reads
    HIP_TRY(hipStreamWaitEvent(ix->s_ord, b->ev[EV_ORD0], 0));
    b->last_ordered = true;
    const size_t tb = sigax_order_reads_tmp_bytes(nsub);
    int rc;
    if ((rc = ensure(&b->ord_keys, (size_t)n * 4)) != SIGAX_OK) return rc;
    if ((rc = ensure(&b->perm, (size_t)n * 4)) != SIGAX_OK) return rc;
    if ((rc = ensure(&b->ord_tmp, tb)) != SIGAX_OK) return rc;
    uint32_t bounds[SIGAX_MAX_SUB + 1];
    for (unsigned i = 0; i <= nsub; ++i) bounds[i] = (uint32_t)((u64)n * i / nsub);
    rc = sigax_order_reads(b->d_seqs, b->d_offs, n, b->cur_max_len, bounds, nsub, (uint32_t*)b->ord_keys.p, (uint32_t*)b->perm.p, b->ord_tmp.p, tb,
                           &b->perm_cur, ix->s_ord);
    if (rc != SIGAX_OK) return rc;
    HIP_TRY(hipEventRecord(b->ev[EV_ORD1], ix->s_ord));
    HIP_TRY(hipStreamWaitEvent(st, b->ev[EV_ORD1], 0));
    b->perm_valid = true;
    b->perm_nsub = nsub;
  }
  *d_perm = b->perm_cur;
  return SIGAX_OK;
}

// Sub-batch i (reads [rb, re)): the finder's launch, or one per strand, on the index's find stream
static int find_sub(sigax_batch* b, unsigned i, uint32_t rb, uint32_t re, const uint32_t* d_perm) {
  sigax_index* ix = b->ix;
  const Settings& cfg = settings();
  const uint32_t stride = perm_stride(b);
  FindArgs fa;
  fa.fwd = ix->st[0];
  fa.rev = ix->st[1];
  fa.seqs = b->d_seqs;
  fa.offs = b->d_offs;
  fa.n_reads = b->n_reads;
  fa.minov = b->minov;
  fa.max_len = b->cur_max_len;
  fa.chain_mask = (b->flags & SIGAX_DUPLICATE) ? 0x9u : (b->flags & SIGAX_RC) ? 0xFu : 0x5u;
  fa.cap = b->cap;
  fa.max_seen = ix->cap_seen->load();
  fa.start_ok = (ix->st[0].start && ix->st[1].start && b->minov >= (uint32_t)SIGAX_START_K) ? 1u : 0u;
  fa.deep_k = (!cfg.find_deep_use_off && ix->st[0].deep && ix->st[1].deep && ix->st[0].deep_k == ix->st[1].deep_k && ix->st[0].deep_k <= b->minov) ? ix->st[0].deep_k : 0u;
  b->last_deep_k = fa.deep_k;
  fa.read_begin = rb;
  fa.read_end = re;
  fa.stage_bytes = 0;  // set by launch_find
  fa.two_step = (ix->st[0].gran2 && ix->st[1].gran2) ? 1u : 0u;
  fa.mask_upper = cfg.find_mask_upper_off ? 0u : 1u;  // A/B aid: 0 = ten loads for every lane
  {
    // From 2^30 symbols the cooperative finder is the faster one (round 3, one rank's view of the 2- / 4- / 8-GPU jobs of
    // bench.py: 7.6e8 symbols 93.6 M reads/s per lane vs 92.3 M cooperative; 1.5e9 symbols 76.7 vs 90.4 M; round 2, before
    // the cooperative finder's LDS diet, had 80 vs 66 M at 1.2e9); from 2^31 the per-lane finder's 32-bit byte offsets
    // no longer reach the table at all.
    // Round 4: with the deep start table and three workgroups per CU the per-lane finder leads again wherever it can reach
    // (same box, one rank's view of the 4-GPU job, 1.51e9 symbols: 117.6 M reads/s per lane vs 111.0 M cooperative; 2-GPU
    // job, 7.6e8: 128.6 vs 120.0 M), so the switch sits at its reach: 2^31 symbols.
    // the workgroup's 64 reads, staged as 4-bit ranks: one byte range, or by slot under the locality order
    const u64 need = d_perm ? 32ull * stride + 32 : (64ull * b->cur_max_len + 16) / 2 + 16;
    const bool can = fa.two_step && need <= 32768;
    const bool want = want_coop(ix, b);
    fa.coop = (can && want) ? 1u : 0u;
    fa.coop_stage_bytes = (uint32_t)((need + 15) & ~15ull);
    // measurement aid: cap the grid at this many workgroups per CU (they then walk the tiles).  Not a way to set the
    // residency: the dispatcher packs a CU before it moves on, so a grid of 4 per CU fills two CUs in three with 6 each
    // (finder 10.3 ms per 1 M reads at C2 against 7.7 uncapped, tools/coop_c2.sh)
    fa.coop_grid = (uint32_t)ix->n_cu * cfg.find_coop_wgs;
    // per-lane gathers use 32-bit byte offsets into the two-step table: beyond 2^31 symbols only the cooperative form works
    if (fa.two_step && !fa.coop && ix->n_symbols >= (1ull << 31)) fa.two_step = 0;
  }
  fa.arena = b->arena.p;
  fa.chain_cnt = (uint32_t*)b->chain_cnt.p;
  fa.dstat = (u64*)b->dstat.p;
  fa.perm = (fa.coop || 128ull * stride + 8 <= find_stage_capacity(b->cur_max_len)) ? d_perm : nullptr;
  fa.stage_stride = stride;
  b->last_two_step = fa.two_step != 0;
  b->last_coop = fa.coop != 0;
  b->last_perm = fa.perm != nullptr;
  HIP_TRY(hipEventRecord(b->sev[i][SV_F0], ix->s_find));
  fa.chain_base = 0;
  fa.chains_per_wg = 4;
  // (only while the 128 reads of such a workgroup still fit the LDS staging buffer: the double step needs them there)
  // Without the two-step tables (indexes of 1.6 G symbols and more) the same split keeps one launch's gathers inside one
  // strand's granule table once the two tables together pass the translation reach (profiles/r01_gather_probe.txt).
  const bool big_one_step = !fa.two_step && ix->n_symbols >= (1ull << 30);
  const bool split = fa.coop || (cfg.split_strands.value_or((fa.two_step && ix->split_strands) || big_one_step) &&
                                 128ull * b->cur_max_len + 8 <= find_stage_capacity(b->cur_max_len));
  b->find_per_sub = split ? 2u : 1u;
  if (split) {
    // one launch per strand's two-step table (chains 0,1 gather from the forward index, 2,3 from the reverse one)
    fa.chains_per_wg = 2;
    launch_find(fa, ix->wide, ix->s_find);
    fa.chain_base = 2;
  }
  launch_find(fa, ix->wide, ix->s_find);
  HIP_TRY(hipEventRecord(b->sev[i][SV_F1], ix->s_find));
  HIP_TRY(hipStreamWaitEvent(ix->s_fx, b->sev[i][SV_F1], 0));
  return SIGAX_OK;
}

// Sub-batch i (reads [rb, re)): the fast filter/extract launch chain on the index's filter/extract stream, then the general
// kernel on the tail stream
static int fx_sub(sigax_batch* b, unsigned i, uint32_t rb, uint32_t re, unsigned fast_grid) {
  sigax_index* ix = b->ix;
  const Settings& cfg = settings();
  u64* dstat = (u64*)b->dstat.p;
  FxArgs xa{};  // no input / output queues (set per launch by launch_filter_extract_fast), no work list
  xa.fwd = ix->st[0];
  xa.rev = ix->st[1];
  xa.offs = b->d_offs;
  if (cfg.fx_one_step) xa.fwd.gran2 = xa.rev.gran2 = nullptr;  // A/B aid: extractor without the two-step table
  xa.n_reads = b->n_reads;
  xa.cap = b->cap;
  xa.irreducible = (b->flags & SIGAX_IRREDUCIBLE) ? 1u : 0u;
  xa.no_lean = (b->lean_off || cfg.fx_skip_strict) ? 1u : 0u;  // (SIGAX_FX_SKIP_STRICT: A/B aid)
  xa.arena = b->arena.p;
  xa.chain_cnt = (const uint32_t*)b->chain_cnt.p;
  xa.n_map = ix->n_strings;
  xa.pool = (Ent*)b->pool.p;
  xa.pool_cap = b->pool_cap;
  xa.wpool = (Ent*)b->wpool.p;
  xa.work_out = (uint32_t*)b->work.p + rb;
  xa.slow_counter = dstat + DS_SLOW_BASE + i;
  xa.work64 = (uint32_t*)b->work64.p + 2 * (size_t)rb;
  xa.w64_counter = dstat + DS_W64_BASE + i;
  xa.work64b = (uint32_t*)b->work64b.p + 2 * (size_t)rb;
  xa.w64b_counter = dstat + DS_W64B_BASE + i;
  xa.work64c = (uint32_t*)b->work64c.p + 2 * (size_t)rb;
  xa.w64c_counter = dstat + DS_W64C_BASE + i;
  xa.work64d = (uint32_t*)b->work64d.p + 2 * (size_t)rb;
  xa.w64d_counter = dstat + DS_W64D_BASE + i;
  xa.read_begin = rb;
  xa.read_end = re;
  xa.item_base = (u64*)b->item_base.p;
  xa.fin = (sigax_block*)b->fin.p;
  xa.fin_cap = b->fin_cap;
  xa.fin_cnt = (uint32_t*)b->fin_cnt.p;
  xa.occ_side = (uint32_t*)b->occ_side.p;
  xa.slow_flag = (uint32_t*)b->slow_flag.p;
  xa.substring = (uint8_t*)b->substring.p;
  xa.dstat = dstat;
  HIP_TRY(hipEventRecord(b->sev[i][SV_X0], ix->s_fx));
  if (!cfg.general_only) {  // (SIGAX_GENERAL_ONLY: debugging aid, skips the fast kernel)
    // grid of the 64-lane launches: SIGAX_FX_GRID64 (they size themselves down by their queues)
    launch_filter_extract_fast(xa, ix->wide, fast_grid, std::min(fast_grid, cfg.fx_grid64), b->qhint_lean_off == b->lean_off ? b->qhint : nullptr, ix->s_fx);
    xa.work = (const uint32_t*)b->work.p + rb;  // the general kernel redoes what the fast one queued
    xa.n_work_ptr = dstat + DS_SLOW_BASE + i;
  } else {
    // every read of the sub-batch through the general kernel
    std::vector<uint32_t> ids(re - rb);
    for (uint32_t k = rb; k < re; ++k) ids[k - rb] = k;
    HIP_TRY(hipMemcpyAsync((uint32_t*)b->work.p + rb, ids.data(), ids.size() * 4, hipMemcpyHostToDevice, ix->s_fx));
    HIP_TRY(hipStreamSynchronize(ix->s_fx));
    xa.work = (const uint32_t*)b->work.p + rb;
    xa.n_work = re - rb;
  }
  HIP_TRY(hipEventRecord(b->sev[i][SV_X1], ix->s_fx));
  // The general kernel (what the lane-group launches queued: usually nothing) goes to the high-priority tail stream: on
  // the low-priority one its 170-register workgroups found no room beside the finder's, whose own new workgroups took
  // every slot that came free first -- at the BASELINE configs[4] shape an EMPTY launch sat there for 3 to 6 ms per run
  // and held up the next batch's filter/extract chain behind it.
  HIP_TRY(hipStreamWaitEvent(ix->s_tail, b->sev[i][SV_X1], 0));
  launch_filter_extract(xa, ix->wide, b->fx_grid, ix->s_tail);
  HIP_TRY(hipEventRecord(b->sev[i][SV_G1], ix->s_tail));
  return SIGAX_OK;
}

static OrderArgs order_args(sigax_batch* b) {
  sigax_index* ix = b->ix;
  OrderArgs oa;
  oa.fin = (const sigax_block*)b->fin.p;
  oa.item_base = (const u64*)b->item_base.p;
  oa.fin_cnt = (const uint32_t*)b->fin_cnt.p;
  oa.n_items = 2 * (u64)b->n_reads;
  oa.fin_cap = b->fin_cap;
  oa.offs2 = (const u64*)b->offs2.p;
  oa.out = (sigax_block*)b->outb.p;
  oa.out_cap = b->fin_cap;
  oa.arena = b->arena.p;
  oa.cap = b->cap;
  oa.wide = ix->wide ? 1u : 0u;
  oa.read_ids = b->d_ids;
  oa.n_index_reads = (uint32_t)std::min<u64>(ix->n_strings, 0xFFFFFFFFull);
  oa.bad_ids = nullptr;
  return oa;
}

// The short tail (scans, ordered scatter or edge records) runs on its own high-priority stream: queued behind the
// long kernels of the next batch on an ordinary stream it took ten times its own duration and held up the
// batch's completion, i.e. the moment the caller can submit this batch object again.
//   without SIGAX_EDGES: scan of fin_cnt (which also writes block_offs), ordered copy of the blocks: three launches
//   with SIGAX_EDGES:    scan of fin_cnt, stage, scan of edge_cnt, emit: six launches.  No consumer of the edge records
//     reads the ordered blocks, so they are not made here: order_blocks() makes them when they are asked for.  The staged
//     records live in outb's allocation (fin_cap records of 16 bytes in room for fin_cap blocks of 80).
static int tail(sigax_batch* b, bool edges, hipStream_t st) {
  sigax_index* ix = b->ix;
  const uint32_t n = b->n_reads;
  u64* dstat = (u64*)b->dstat.p;
  HIP_TRY(hipEventRecord(b->ev[EV_FX_DONE], ix->s_fx));
  hipStream_t ts = ix->s_tail;
  HIP_TRY(hipStreamWaitEvent(ts, b->ev[EV_FX_DONE], 0));

  launch_scan((const uint32_t*)b->fin_cnt.p, 2 * (u64)n, (u64*)b->partial.p, (u64*)b->offs2.p, dstat + DS_TOTAL_BLOCKS, ts, (u64*)b->block_offs.p);
  EdgeArgs ea;
  if (!edges) {
    OrderArgs oa = order_args(b);
    oa.bad_ids = dstat + DS_BAD_IDS;
    launch_order_scatter(oa, ts);
  } else {
    ea.fin = (const sigax_block*)b->fin.p;
    ea.item_base = (const u64*)b->item_base.p;
    ea.fin_cap = b->fin_cap;
    ea.arena = b->arena.p;
    ea.cap = b->cap;
    ea.wide = ix->wide ? 1u : 0u;
    ea.offs2 = (const u64*)b->offs2.p;
    ea.fin_cnt = (const uint32_t*)b->fin_cnt.p;
    ea.n_items = 2 * (u64)n;
    ea.stage = b->outb.p;
    ea.stage_cap = b->fin_cap;
    ea.item_edges = (uint32_t*)b->edge_cnt.p;
    ea.read_base = b->read_base;
    ea.read_ids = b->d_ids;
    ea.n_index_reads = (uint32_t)std::min<u64>(ix->n_strings, 0xFFFFFFFFull);
    ea.bad_ids = dstat + DS_BAD_IDS;
    ea.sai = ix->d_sai[0];
    ea.rsai = ix->d_sai[1];
    ea.n_sai = ix->n_sai;
    ea.read_len = ix->d_read_len;
    ea.name_rank = ix->d_name_rank;
    ea.edge_offs = (const u64*)b->edge_offs.p;
    ea.edges = (sigax_edge*)b->edges.p;
    ea.edge_cap = b->edge_cap;
    launch_edges_stage(ea, ts);
  }
  b->blocks_ordered = !edges;
  HIP_TRY(hipEventRecord(b->ev[EV_ORDER], ts));

  if (edges) {
    launch_scan((const uint32_t*)b->edge_cnt.p, 2 * (u64)n, (u64*)b->partial.p, (u64*)b->edge_offs.p, dstat + DS_TOTAL_EDGES, ts);
    launch_edges_emit(ea, ts);
  }
  HIP_TRY(hipEventRecord(b->ev[EV_EDGES], ts));
  HIP_TRY(hipStreamWaitEvent(st, b->ev[EV_EDGES], 0));
  HIP_TRY(hipGetLastError());
  return SIGAX_OK;
}

// The ordered blocks of a finished run with SIGAX_EDGES, made when they are first asked for: fin, item_base, offs2 and the
// candidate arena stay as the run left them until the batch's next run.  The copy goes to the tail stream under the index's
// enqueue mutex, like every launch sequence on the shared streams, and is waited for.
static int order_blocks(sigax_batch* b) {
  if (b->blocks_ordered) return SIGAX_OK;
  sigax_index* ix = b->ix;
  HIP_TRY(hipSetDevice(ix->device));
  {
    std::lock_guard<std::mutex> lock(*ix->enqueue_mu);
    launch_order_scatter(order_args(b), ix->s_tail);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(b->ev[EV_BLOCKS], ix->s_tail));
  }
  HIP_TRY(hipEventSynchronize(b->ev[EV_BLOCKS]));
  b->blocks_ordered = true;
  return SIGAX_OK;
}

static int enqueue(sigax_batch* b, hipStream_t st) {
  sigax_index* ix = b->ix;
  if (ix->fwd_only) return sigax_fail(SIGAX_E_STATE, "the index was opened without its reverse strand: overlap runs need <prefix>.rbwt too");
  std::lock_guard<std::mutex> lock(*ix->enqueue_mu);  // one batch's launch sequence at a time on the shared streams
  b->blocks_ordered = false;  // outb is about to be rewritten (tail)
  publish_tables(ix);
  publish_deep(ix);
  // a whole pass over the indexed reads has been asked for before this run: the index is being reused
  if (ix->reads_asked >= std::max<u64>(ix->n_strings, 1)) {
    start_row_tables(ix, false);
    if (!(b->flags & SIGAX_DUPLICATE)) start_deep_tables(ix, b->minov);
  }
  ix->reads_asked += b->n_reads;
  const uint32_t n = b->n_reads;
  const bool edges = (b->flags & SIGAX_EDGES) != 0;
  if (edges && (!ix->d_sai[0] || !ix->d_read_len))
    return sigax_fail(SIGAX_E_STATE, "SIGAX_EDGES needs the .sai tables and sigax_index_set_reads()");
  if (b->d_ids != nullptr && b->ids_n != n)
    return sigax_fail(SIGAX_E_STATE, "the batch holds read ids for %u reads and %u reads (sigax_batch_set_device_read_ids(NULL) forgets them)", b->ids_n, n);
  if (edges && b->d_ids == nullptr && (u64)b->read_base + n > ix->n_strings)
    return sigax_fail(SIGAX_E_ARG, "read_base + n_reads exceeds the indexed read set");
  unsigned fast_grid = 0;
  int rc = size_arenas(b, edges, &fast_grid);
  if (rc != SIGAX_OK) return rc;
  HIP_TRY(hipMemsetAsync(b->dstat.p, 0, DS_COUNT * 8, st));
  HIP_TRY(hipMemsetAsync(b->occ_side.p, 0, (2 * (size_t)n + 2) * 4, st));
  HIP_TRY(hipMemsetAsync(b->slow_flag.p, 0, ((size_t)n + 1) * 4, st));
  // Sub-batches: the finder is bound by the memory system's request rate, filter/extract by VALU issue; running
  // sub-batch i's filter/extract while sub-batch i+1's finder runs overlaps the two.
  const std::optional<int>& env_sub = settings().subbatches;
  unsigned nsub = b->nsub_req ? b->nsub_req : env_sub ? (unsigned)*env_sub : (n >= 4 * 131072u ? 4u : n >= 2 * 131072u ? 2u : 1u);
  if (nsub < 1) nsub = 1;
  if (nsub > SIGAX_MAX_SUB) nsub = SIGAX_MAX_SUB;
  b->nsub = nsub;
  const uint32_t* d_perm = nullptr;
  if ((rc = locality_order(b, st, &d_perm)) != SIGAX_OK) return rc;
  HIP_TRY(hipEventRecord(b->ev[EV_START], st));

  HIP_TRY(hipStreamWaitEvent(ix->s_find, b->ev[EV_START], 0));
  HIP_TRY(hipStreamWaitEvent(ix->s_fx, b->ev[EV_START], 0));
  for (unsigned i = 0; i < nsub; ++i) {
    const uint32_t rb = (uint32_t)((u64)n * i / nsub), re = (uint32_t)((u64)n * (i + 1) / nsub);
    if ((rc = find_sub(b, i, rb, re, d_perm)) != SIGAX_OK || (rc = fx_sub(b, i, rb, re, fast_grid)) != SIGAX_OK) return rc;
  }
  return tail(b, edges, st);
}

extern "C" int sigax_batch_run(sigax_batch* b, uint32_t read_base, uint32_t min_overlap, uint32_t flags, void* stream) {
  if (!b) return sigax_fail(SIGAX_E_ARG, "NULL batch");
  if (b->n_reads && !b->d_seqs) return sigax_fail(SIGAX_E_STATE, "no reads set on this batch");
  HIP_TRY(hipSetDevice(b->ix->device));
  b->read_base = read_base;
  b->minov = min_overlap;
  b->flags = flags;
  if (flags & SIGAX_DUPLICATE) {  // duplicate(): minOverlap = seq.length() so no proper-overlap block is ever pushed;
    b->minov = 0xFFFFFFFFu;       // the exhaustive plumbing then returns exactly {containment of find 0, of find 3}
    b->flags = (flags & SIGAX_EDGES) | SIGAX_DUPLICATE;
  }
  b->finished = false;
  int rc = enqueue(b, (hipStream_t)stream);
  b->ran = rc == SIGAX_OK;
  return rc;
}

extern "C" int sigax_batch_finish(sigax_batch* b, void* stream, sigax_stats* stats) {
  if (!b) return sigax_fail(SIGAX_E_ARG, "NULL batch");
  if (!b->ran) return sigax_fail(SIGAX_E_STATE, "sigax_batch_run was not called");
  HIP_TRY(hipSetDevice(b->ix->device));
  hipStream_t st = (hipStream_t)stream;
  for (int attempt = 0; attempt < 8; ++attempt) {
    u64 ds[DS_COUNT];
    HIP_TRY(hipMemcpyAsync(ds, b->dstat.p, sizeof(ds), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    bool again = false;
    {
      // what the longest chain needed becomes the index's knowledge (later runs and other batch objects size by it)
      uint32_t seen = b->ix->cap_seen->load();
      const uint32_t got = (uint32_t)std::min<u64>(ds[DS_MAX_CHAIN], 0x0FFFFFFFull);
      while (got > seen && !b->ix->cap_seen->compare_exchange_weak(seen, got)) {}
    }
    if (ds[DS_BAD_IDS])
      return sigax_fail(SIGAX_E_ARG, "%llu (read, side) items carry a read id beyond the %llu indexed reads (sigax_batch_set_device_read_ids)",
                  (unsigned long long)ds[DS_BAD_IDS], (unsigned long long)b->ix->n_strings);
    if (ds[DS_FIND_OVERFLOW]) {
      if (b->cap >= worst_cap(b->cur_max_len, b->minov))
        return sigax_fail(SIGAX_E_CAPACITY, "candidate arena overflow (max read length given too small?)");
      b->cap_floor = (uint32_t)std::min<u64>(ds[DS_MAX_CHAIN], 0x0FFFFFFFull);  // the chains ran out of slots: once more with what they need
      again = true;
    }
    if (ds[DS_POOL_OVERFLOW]) {
      if (b->pool_cap > (1u << 22)) return sigax_fail(SIGAX_E_CAPACITY, "%llu reads overflow the filter/extract pool", ds[DS_POOL_OVERFLOW]);
      b->pool_cap *= 4;
      again = true;
    }
    if (ds[DS_FIN_TOP] > b->fin_cap) {
      b->fin_cap = ds[DS_FIN_TOP] + ds[DS_FIN_TOP] / 4 + 1024;
      b->fin_grown = true;
      if (b->edge_cap) b->edge_cap = std::max<u64>(b->edge_cap, b->fin_cap * 2);
      again = true;
    }
    if (!again && (b->flags & SIGAX_EDGES) && ds[DS_TOTAL_EDGES] > b->edge_cap) {
      b->edge_cap = ds[DS_TOTAL_EDGES] + ds[DS_TOTAL_EDGES] / 4 + 1024;
      again = true;
    }
    if (again) {
      ++b->n_reruns;
      int rc = enqueue(b, st);
      if (rc != SIGAX_OK) return rc;
      continue;
    }
    memset(&b->last, 0, sizeof(b->last));
    b->last.n_reads = b->n_reads;
    b->last.n_candidate_blocks = ds[DS_CAND_BLOCKS];
    b->last.n_blocks = ds[DS_TOTAL_BLOCKS];
    b->last.n_edges = (b->flags & SIGAX_EDGES) ? ds[DS_TOTAL_EDGES] : 0;
    b->last.n_occ_find = ds[DS_OCC_FIND];
    b->last.n_occ_extract = ds[DS_OCC_EXTRACT];
    b->last.n_substring = ds[DS_SUBSTRING];
    b->last.n_slow_reads = 0;
    for (int i = 0; i < SIGAX_MAX_SUB; ++i) b->last.n_slow_reads += ds[DS_SLOW_BASE + i];
    {
      // Reads with sequencing errors make the extraction branch; the strict lean launch hands such items on after wasted
      // work.  If more than a tenth of the (read, side) items went on, this batch object starts its next 32 runs with the
      // branching lean launch (9 % slower on items that do not branch, no wasted work on those that do: measured equal
      // at 8 % handed on, 12 % ahead at 23 %, tools/ab_skip_strict.sh), then tries the strict one again.
      u64 q64 = 0;
      for (int i = 0; i < SIGAX_MAX_SUB; ++i) q64 += ds[DS_W64_BASE + i];
      for (int k = 0; k < 4; ++k) {
        const int base = k == 0 ? DS_W64_BASE : k == 1 ? DS_W64B_BASE : k == 2 ? DS_W64C_BASE : DS_W64D_BASE;
        u64 m = 0;
        for (int i = 0; i < SIGAX_MAX_SUB; ++i) m = std::max<u64>(m, ds[base + i]);
        b->qhint[k] = m;
      }
      b->qhint_lean_off = b->lean_off;
      const u64 items = 2ull * b->n_reads;
      if (!b->lean_off) {
        if (q64 * 10 > items) {
          b->lean_off = true;
          b->lean_off_runs = 32;
        }
      } else if (--b->lean_off_runs == 0) {
        b->lean_off = false;
      }
    }
    {
      // Which kernel did the step wait for?  The launches' own durations (beside each other, as they ran) decide the
      // residency split of this batch object's next run: the finder's three workgroups per CU leave two and a half
      // filter/extract workgroups room, which is the better split while the two kernels take about the same time; reads with
      // sequencing errors make filter/extract the longer one by up to 2x, and it then gets three per CU (enqueue).  With
      // hysteresis: the ratio itself moves by 0.1 with the split.
      float tf = 0.f, tx = 0.f, t = 0.f;
      bool ok = true;
      for (unsigned i = 0; i < b->nsub && ok; ++i) {
        ok = hipEventElapsedTime(&t, b->sev[i][SV_F0], b->sev[i][SV_F1]) == hipSuccess;
        tf += t;
        ok = ok && hipEventElapsedTime(&t, b->sev[i][SV_X0], b->sev[i][SV_X1]) == hipSuccess;
        tx += t;
      }
      if (!ok) (void)hipGetLastError();
      else if (tf > 0.f) {
        if (!b->fx_heavy && tx > 1.12f * tf) b->fx_heavy = true;
        else if (b->fx_heavy && tx < 0.95f * tf) b->fx_heavy = false;
      }
      if (b->coop_tune < 4 && coop_tunable(b->ix)) {  // want_coop: this run was per lane (0, 1) or cooperative (2, 3)
        if (!ok || tf <= 0.f) {
          b->coop_tune = 4;  // no times, no tuning: per lane
          b->coop_pick = false;
        } else {
          if (b->coop_tune == 1) b->coop_t_lane = tf;
          if (b->coop_tune == 3) b->coop_pick = b->last_coop && tf < b->coop_t_lane;
          ++b->coop_tune;
        }
      }
    }
    b->last.n_extract_errors = ds[DS_EXTRACT_ERRORS];
    b->last.n_sectors_find = ds[DS_SEC_FIND];
    b->last.n_sectors_extract = ds[DS_SEC_EXTRACT];
    b->last_total_blocks = ds[DS_TOTAL_BLOCKS];
    b->last_total_edges = b->last.n_edges;
    b->finished = true;
    if (stats) *stats = b->last;
    return SIGAX_OK;
  }
  return sigax_fail(SIGAX_E_CAPACITY, "arenas still overflowing after 8 attempts");
}

extern "C" int sigax_batch_device_outputs(sigax_batch* b, const sigax_block** d_blocks, const uint64_t** d_block_offs,
                                          const uint8_t** d_substring, const sigax_edge** d_edges) {
  if (!b || !b->finished) return sigax_fail(SIGAX_E_STATE, "batch not finished");
  if (d_blocks) {
    int rc = order_blocks(b);
    if (rc != SIGAX_OK) return rc;
    *d_blocks = (const sigax_block*)b->outb.p;
  }
  if (d_block_offs) *d_block_offs = (const uint64_t*)b->block_offs.p;
  if (d_substring) *d_substring = (const uint8_t*)b->substring.p;
  if (d_edges) *d_edges = (const sigax_edge*)b->edges.p;
  return SIGAX_OK;
}

extern "C" void sigax_result_free(sigax_result* r) {
  if (!r) return;
  free(r->block_offs);
  free(r->blocks);
  free(r->substring);
  free(r->edges);
  memset(r, 0, sizeof(*r));
}

extern "C" int sigax_batch_download(sigax_batch* b, sigax_result* out) {
  if (!b || !out) return sigax_fail(SIGAX_E_ARG, "NULL argument");
  if (!b->finished) return sigax_fail(SIGAX_E_STATE, "batch not finished");
  HIP_TRY(hipSetDevice(b->ix->device));
  memset(out, 0, sizeof(*out));
  int rc = order_blocks(b);
  if (rc != SIGAX_OK) return rc;
  uint32_t n = b->n_reads;
  out->n_reads = n;
  out->stats = b->last;
  out->block_offs = (uint64_t*)malloc(((size_t)n + 1) * 8);
  out->blocks = (sigax_block*)malloc(std::max<size_t>(1, b->last_total_blocks) * sizeof(sigax_block));
  out->substring = (uint8_t*)malloc(std::max<size_t>(1, n));
  out->n_edges = b->last_total_edges;
  out->edges = (sigax_edge*)malloc(std::max<size_t>(1, b->last_total_edges) * sizeof(sigax_edge));
  if (!out->block_offs || !out->blocks || !out->substring || !out->edges) {
    sigax_result_free(out);
    return sigax_fail(SIGAX_E_ARG, "host allocation failed");
  }
  HIP_TRY(hipMemcpy(out->block_offs, b->block_offs.p, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost));
  if (b->last_total_blocks)
    HIP_TRY(hipMemcpy(out->blocks, b->outb.p, b->last_total_blocks * sizeof(sigax_block), hipMemcpyDeviceToHost));
  if (n) HIP_TRY(hipMemcpy(out->substring, b->substring.p, n, hipMemcpyDeviceToHost));
  if (b->last_total_edges)
    HIP_TRY(hipMemcpy(out->edges, b->edges.p, b->last_total_edges * sizeof(sigax_edge), hipMemcpyDeviceToHost));
  return SIGAX_OK;
}

// Diagnostic builds (-DSIGAX_FX_PROFILE): which path the extension rounds of the last finished run took.  Not in the header.
extern "C" int sigax_debug_counters(sigax_batch* b, uint64_t out[32]) {
  if (!b || !out) return sigax_fail(SIGAX_E_ARG, "NULL argument");
  HIP_TRY(hipSetDevice(b->ix->device));
  HIP_TRY(hipMemcpy(out, (u64*)b->dstat.p + DS_PROF_BASE, 32 * 8, hipMemcpyDeviceToHost));
  return SIGAX_OK;
}

// What the ASQG writer needs from a finished batch: substring flags and edge records (not the 80-byte blocks).
extern "C" int sigax_batch_download_edges(sigax_batch* b, uint8_t* substring, sigax_edge** edges, uint64_t* n_edges) {
  if (!b || !edges || !n_edges) return sigax_fail(SIGAX_E_ARG, "NULL argument");
  if (!b->finished) return sigax_fail(SIGAX_E_STATE, "batch not finished");
  HIP_TRY(hipSetDevice(b->ix->device));
  *edges = nullptr;
  *n_edges = b->last_total_edges;
  if (substring && b->n_reads) HIP_TRY(hipMemcpy(substring, b->substring.p, b->n_reads, hipMemcpyDeviceToHost));
  sigax_edge* e = (sigax_edge*)malloc(std::max<size_t>(1, b->last_total_edges) * sizeof(sigax_edge));
  if (!e) return sigax_fail(SIGAX_E_ARG, "host allocation failed");
  if (b->last_total_edges) {
    hipError_t err = hipMemcpy(e, b->edges.p, b->last_total_edges * sizeof(sigax_edge), hipMemcpyDeviceToHost);
    if (err != hipSuccess) {
      free(e);
      return sigax_fail(SIGAX_E_DEVICE, "copying edge records: %s", hipGetErrorString(err));
    }
  }
  *edges = e;
  return SIGAX_OK;
}

// How many reads of up to max_read_len bases one batch object may hold when `in_flight` of them share the device's
// free memory (the candidate arena is sized for the worst case: 4 chains x (L - m + 1) records per read).
extern "C" int sigax_batch_size_hint(sigax_index* ix, uint32_t max_read_len, uint32_t min_overlap, uint32_t flags, uint32_t in_flight,
                                     uint32_t* max_reads) {
  if (!ix || !max_reads) return sigax_fail(SIGAX_E_ARG, "NULL argument");
  HIP_TRY(hipSetDevice(ix->device));
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  free_b = free_b > ix->tab_plan ? free_b - ix->tab_plan : 0;  // the row tables are allocated later (build_rowend)
  // Slots per chain: the WORST case (one per overlap length).  A run sizes its arena by the longest chain seen so far and
  // repeats itself with more when a chain outgrows that (sigax_batch_finish) -- up to the worst case, so that is what a
  // batch of this many reads must be able to get: a hint from the typical size let a rerun's arena grow fail with
  // SIGAX_E_DEVICE in the middle of a job on a memory-tight index (BASELINE configs[4]: 190 GB of tables).  The price is
  // nil where memory is plentiful (the callers cap their batches at 2^20 reads) and 1 M -> 0.7 M reads per batch at configs[4].
  const uint32_t mo = (flags & SIGAX_DUPLICATE) ? max_read_len : min_overlap;
  const u64 cap = worst_cap(max_read_len, mo);
  if (!ix->ptab_tried) free_b = free_b > prefix_table_bytes(ix->wide, 13) ? free_b - prefix_table_bytes(ix->wide, 13) : 0;  // `siga correct`'s table, built at its first call
  // + the locality order's keys, values and sort space (40 bytes per read), the per-read queues and counters (~70)
  const u64 per_read = 4 * cap * cand_bytes(ix->wide) + max_read_len + ((flags & SIGAX_IRREDUCIBLE) ? 8 : 64) * (2 * 80 + 2 * 16 + 12) + 256;
  const u64 fixed = (2ull << 30) + (u64)32768 * (4 * (cap + 2) + 128) * SIGAX_ENT_BYTES;  // pools of the lane-group and general kernels
  const u64 share = (u64)(free_b * 0.85) / std::max<uint32_t>(in_flight, 1u);
  u64 n = share > fixed ? (share - fixed) / per_read : 0;
  n = std::min<u64>(n, 1u << 22);
  if (n < 1024) return sigax_fail(SIGAX_E_CAPACITY, "not enough free device memory for a batch of reads of %u bases (%zu bytes free)", max_read_len, free_b);
  *max_reads = (uint32_t)n;
  return SIGAX_OK;
}

extern "C" int sigax_batch_set_subbatches(sigax_batch* b, uint32_t n) {
  if (!b) return sigax_fail(SIGAX_E_ARG, "NULL batch");
  if (n > SIGAX_MAX_SUB) return sigax_fail(SIGAX_E_ARG, "at most %d sub-batches", SIGAX_MAX_SUB);
  b->nsub_req = n;
  return SIGAX_OK;
}

extern "C" int sigax_batch_kernel_ms(sigax_batch* b, float ms[5], uint32_t* n_sub) {
  if (!b || !ms) return sigax_fail(SIGAX_E_ARG, "NULL argument");
  if (!b->finished) return sigax_fail(SIGAX_E_STATE, "batch not finished");
  if (n_sub) *n_sub = b->nsub * b->find_per_sub;
  for (int i = 0; i < 5; ++i) ms[i] = 0.f;
  for (unsigned i = 0; i < b->nsub; ++i) {  // sums over the sub-batch launches (which overlap across the two streams)
    float t = 0.f;
    HIP_TRY(hipEventElapsedTime(&t, b->sev[i][SV_F0], b->sev[i][SV_F1]));
    ms[0] += t;
    HIP_TRY(hipEventElapsedTime(&t, b->sev[i][SV_X0], b->sev[i][SV_X1]));
    ms[1] += t;
    HIP_TRY(hipEventElapsedTime(&t, b->sev[i][SV_X1], b->sev[i][SV_G1]));
    ms[2] += t;
  }
  HIP_TRY(hipEventElapsedTime(&ms[3], b->ev[EV_FX_DONE], b->ev[EV_ORDER]));
  HIP_TRY(hipEventElapsedTime(&ms[4], b->ev[EV_ORDER], b->ev[EV_EDGES]));
  return SIGAX_OK;
}

extern "C" int sigax_batch_run_info(sigax_batch* b, sigax_run_info* out) {
  if (!b || !out) return sigax_fail(SIGAX_E_ARG, "NULL argument");
  if (!b->finished) return sigax_fail(SIGAX_E_STATE, "batch not finished");
  HIP_TRY(hipSetDevice(b->ix->device));
  memset(out, 0, sizeof(*out));
  out->n_sub = b->nsub;
  out->find_per_sub = b->find_per_sub;
  out->two_step = b->last_two_step ? 1u : 0u;
  out->coop = b->last_coop ? 1u : 0u;
  out->read_order = b->last_perm ? 1u : 0u;
  out->cap = b->cap;
  out->worst_cap = worst_cap(b->cur_max_len, b->minov);
  const FmStrand& f = b->ix->st[0];
  out->row_bits = f.sa ? f.sa_bits : 0u;
  out->row_syms = f.sa ? (f.sa_bits - f.ld_bits - f.t_bits) / 2u : 0u;
  out->row_text = f.text ? 1u : 0u;
  out->row_direct = f.xmap ? 1u : 0u;
  out->deep_k = b->last_deep_k;
  out->arena_bytes = b->arena.bytes;
  each_buffer(b, [&](DevBuf* d) { out->workspace_bytes += d->bytes; });
  out->reruns = b->n_reruns;
  if (b->last_ordered) HIP_TRY(hipEventElapsedTime(&out->order_ms, b->ev[EV_ORD0], b->ev[EV_ORD1]));
  return SIGAX_OK;
}

// One call = OverlapBuilder::overlap for any number of reads: what does not fit one device workspace beside the index goes
// through it in pieces (sized by sigax_batch_size_hint) and the pieces' results are joined in read order.
extern "C" int sigax_overlap_batch(sigax_index* ix, const char* seqs, const uint64_t* offs, uint32_t n_reads,
                                   uint32_t read_base, uint32_t min_overlap, uint32_t flags, sigax_result* out) {
  if (!ix || !out || (n_reads && (!seqs || !offs))) return sigax_fail(SIGAX_E_ARG, "NULL argument");
  memset(out, 0, sizeof(*out));
  uint32_t max_len = 0;
  for (uint32_t i = 0; i < n_reads; ++i) {
    if (offs[i + 1] < offs[i] || offs[i + 1] - offs[i] > 0x0FFFFFFFull) return sigax_fail(SIGAX_E_ARG, "bad offsets at read %u", i);
    max_len = std::max<uint32_t>(max_len, (uint32_t)(offs[i + 1] - offs[i]));
  }
  uint32_t piece = n_reads;
  const std::optional<int>& test_piece = settings().test_piece;  // tests: force several pieces on small inputs
  if (n_reads > 65536) {
    uint32_t hint = 0;
    int rc = sigax_batch_size_hint(ix, max_len, min_overlap, flags, 1, &hint);
    if (rc != SIGAX_OK) return rc;
    if (test_piece) hint = std::max<uint32_t>(1u, (uint32_t)*test_piece);
    piece = std::min(n_reads, hint);
  } else if (test_piece) {
    piece = std::min<uint32_t>(n_reads, std::max<uint32_t>(1u, (uint32_t)*test_piece));
  }
  sigax_batch* b = nullptr;
  int rc = sigax_batch_create(ix, piece, 0, max_len, &b);
  if (rc != SIGAX_OK) return rc;
  if (piece == n_reads) {
    rc = sigax_batch_upload(b, seqs, offs, n_reads, nullptr);
    if (rc == SIGAX_OK) rc = sigax_batch_run(b, read_base, min_overlap, flags, nullptr);
    if (rc == SIGAX_OK) rc = sigax_batch_finish(b, nullptr, nullptr);
    if (rc == SIGAX_OK) rc = sigax_batch_download(b, out);
    sigax_batch_destroy(b);
    return rc;
  }
  out->n_reads = n_reads;
  out->block_offs = (uint64_t*)malloc(((size_t)n_reads + 1) * 8);
  out->substring = (uint8_t*)malloc(std::max<size_t>(1, n_reads));
  size_t blk_cap = 0, edge_cap = 0;
  u64 nblk = 0, nedge = 0;
  if (!out->block_offs || !out->substring) rc = sigax_fail(SIGAX_E_ARG, "host allocation failed");
  std::vector<uint64_t> po;
  for (uint32_t lo = 0; rc == SIGAX_OK && lo < n_reads; lo += piece) {
    const uint32_t n = std::min(piece, n_reads - lo);
    po.resize((size_t)n + 1);
    for (uint32_t i = 0; i <= n; ++i) po[i] = offs[lo + i] - offs[lo];
    sigax_result part;
    memset(&part, 0, sizeof(part));
    rc = sigax_batch_upload(b, seqs + offs[lo], po.data(), n, nullptr);
    if (rc == SIGAX_OK) rc = sigax_batch_run(b, read_base + lo, min_overlap, flags, nullptr);
    if (rc == SIGAX_OK) rc = sigax_batch_finish(b, nullptr, nullptr);
    if (rc == SIGAX_OK) rc = sigax_batch_download(b, &part);
    if (rc != SIGAX_OK) break;
    const u64 pb = part.block_offs[n], pe = part.n_edges;
    if (nblk + pb > blk_cap) {
      blk_cap = std::max<size_t>((size_t)(nblk + pb), blk_cap + blk_cap / 2);
      void* q = realloc(out->blocks, std::max<size_t>(1, blk_cap) * sizeof(sigax_block));
      if (!q) rc = sigax_fail(SIGAX_E_ARG, "host allocation failed");
      else out->blocks = (sigax_block*)q;
    }
    if (rc == SIGAX_OK && nedge + pe > edge_cap) {
      edge_cap = std::max<size_t>((size_t)(nedge + pe), edge_cap + edge_cap / 2);
      void* q = realloc(out->edges, std::max<size_t>(1, edge_cap) * sizeof(sigax_edge));
      if (!q) rc = sigax_fail(SIGAX_E_ARG, "host allocation failed");
      else out->edges = (sigax_edge*)q;
    }
    if (rc == SIGAX_OK) {
      for (uint32_t i = 0; i < n; ++i) out->block_offs[lo + i] = nblk + part.block_offs[i];
      if (pb) memcpy(out->blocks + nblk, part.blocks, pb * sizeof(sigax_block));
      if (pe) memcpy(out->edges + nedge, part.edges, pe * sizeof(sigax_edge));
      memcpy(out->substring + lo, part.substring, n);
      nblk += pb;
      nedge += pe;
      uint64_t* acc = (uint64_t*)&out->stats;
      const uint64_t* add = (const uint64_t*)&part.stats;
      for (size_t k = 0; k < sizeof(sigax_stats) / 8; ++k) acc[k] += add[k];
    }
    sigax_result_free(&part);
  }
  sigax_batch_destroy(b);
  if (rc != SIGAX_OK) {
    sigax_result_free(out);
    return rc;
  }
  out->block_offs[n_reads] = nblk;
  out->n_edges = nedge;
  if (!out->blocks) out->blocks = (sigax_block*)malloc(sizeof(sigax_block));
  if (!out->edges) out->edges = (sigax_edge*)malloc(sizeof(sigax_edge));
  return SIGAX_OK;
}
