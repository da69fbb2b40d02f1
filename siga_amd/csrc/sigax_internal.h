// siga_amd/csrc/sigax_internal.h -- what the host side of libsigax.so shares between its files: the error setter, the
// switches read from the environment, the index object and the entry points of its optional tables.  Host code only.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <mutex>
#include <optional>
#include <thread>
#include <vector>

#include "sigax_kernels.h"

typedef unsigned long long u64;
typedef unsigned int u32;

// the library's one error setter: the thread-local text of sigax_last_error(), returns `code` (sigax_index.cpp)
int sigax_fail(int code, const char* fmt, ...);

// RL units (src/rlstring.h:10-63) -> 64-byte rank granules (fm_layout.h), decoded on the device (sigax_index_build.hip)
int sigax_decode_strand(const uint8_t* runs, u64 n_runs, u64 nsym, bool wide, void** d_gran, u64* gran_bytes, void** d_super,
                        u64* super_bytes, u64 C[5], u64 total[5]);

#define HIP_TRY(expr)                                                                                  \
  do {                                                                                                 \
    hipError_t e_ = (expr);                                                                            \
    if (e_ != hipSuccess) return sigax_fail(SIGAX_E_DEVICE, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

// frees device buffers on every exit path of the one-shot calls
struct DevGuard {
  std::vector<void*> ptrs;
  ~DevGuard() {
    for (void* p : ptrs)
      if (p) hipFree(p);
  }
  hipError_t alloc(void** out, size_t bytes) {
    *out = nullptr;
    hipError_t e = hipMalloc(out, bytes ? bytes : 16);
    if (e == hipSuccess) ptrs.push_back(*out);
    return e;
  }
};

// owns the host arrays a call hands to its caller (who returns them with sigax_free) until the call has succeeded
struct HostGuard {
  std::vector<void*> ptrs;
  bool ok = true;
  ~HostGuard() {
    for (void* p : ptrs) free(p);
  }
  template <typename T>
  T* alloc(size_t bytes) {
    void* p = malloc(bytes ? bytes : 1);
    ok = ok && p != nullptr;
    ptrs.push_back(p);
    return (T*)p;
  }
  void release() { ptrs.clear(); }
};

// Measurement aid of tools/unitig_bench.py, exported but not part of include/sigax.h and not stable: the bases pass of
// sigax_unitigs_device alone, over the scratch a call with the same reads and records left in d_work.  It cannot tell whether
// such a call was made; the pass bounds every access all the same.  Same argument checks as sigax_unitigs_device.
extern "C" int sigax_unitigs_bases_device(int device, const void* d_seqs, const void* d_offs, uint64_t n_reads, uint64_t n_edges, void* d_useqs,
                                          void* d_work, uint64_t work_bytes, void* stream);

// Measurement aid of tools/scaffold_bench.py, exported but not part of include/sigax.h and not stable: the bases pass of
// sigax_scaffold_device alone, over the scratch a call with the same arguments left in d_work.  Same argument checks.
extern "C" int sigax_scaffold_bases_device(int device, const void* d_n_unitigs, uint64_t max_unitigs, const void* d_seq_offs, const void* d_uflags,
                                           const void* d_useqs, uint64_t useqs_bytes, const sigax_pair_link* d_links, const void* d_n_links,
                                           uint64_t max_links, const void* d_status24, const sigax_scaffold_opts* opts, void* d_sc_offs,
                                           void* d_sc_lay_offs, void* d_sc_flags, sigax_placement* d_sc_layout, void* d_sseqs,
                                           uint64_t sseqs_capacity, void* d_status16, void* d_work, uint64_t work_bytes, void* stream);

#pragma GCC visibility push(hidden)

// ------------------------------------------------------------------------------------------------------
// The SIGAX_* switches of the host code, read once, at the first settings() call: nothing sets one in-process after the
// library has loaded.  Read elsewhere: SIGAX_BUILD_GROUP (sigax_index_build.hip, per call: a test changes it between
// calls) and the launch switches of sigax_kernels.hip (finder and filter/extract; sigax_tables.hip and sigax_tail.hip have
// none).  INTEGRATION.md lists them all.
// ------------------------------------------------------------------------------------------------------
struct Settings {
  static bool set(const char* v) { return v != nullptr; }     // present, whatever its value
  static bool zero(const char* v) { return v && v[0] == '0'; }  // "=0"
  static char first(const char* v) { return v ? v[0] : '\0'; }
  static std::optional<bool> on_off(const char* v) { return v ? std::optional<bool>(v[0] != '0') : std::nullopt; }
  static std::optional<int> num(const char* v) { return v ? std::optional<int>(atoi(v)) : std::nullopt; }
  static std::optional<u64> unum(const char* v) { return v ? std::optional<u64>(strtoull(v, nullptr, 10)) : std::nullopt; }

  bool verbose = set(getenv("SIGAX_VERBOSE"));                                   // diagnostics: which tables, open times
  bool no_sai_cache = set(getenv("SIGAX_NO_SAI_CACHE"));                         // option: no <file>.sai.bin images
  bool force_wide = set(getenv("SIGAX_FORCE_WIDE"));                             // test hook: 64-bit positions on a small index
  bool two_step_off = zero(getenv("SIGAX_TWO_STEP"));                            // A/B aid: no two-step tables
  u64 two_step_max_symbols = unum(getenv("SIGAX_TWO_STEP_MAX_SYMBOLS")).value_or(~0ull);  // test hook: two-step tables below n
  std::optional<bool> find_start = on_off(getenv("SIGAX_FIND_START"));           // test hook: finder start tables off / forced
  int cu_split = num(getenv("SIGAX_CU_SPLIT")).value_or(0);                      // experiment: CUs of the non-finder streams
  bool rowend_off = zero(getenv("SIGAX_ROWEND"));                                // A/B aid: no row tables, the extractor walks
  bool lookahead_off = zero(getenv("SIGAX_LOOKAHEAD"));                          // A/B aid: row tables without the text
  char xmap = first(getenv("SIGAX_XMAP"));                                       // test hook: '1' forces direct maps, '0' forbids
  u32 row_syms = (u32)num(getenv("SIGAX_ROW_SYMS")).value_or(14);                // test hook: symbols a row-table entry carries
  bool tables_sync = set(getenv("SIGAX_TABLES_SYNC"));                           // option: row tables built at open
  bool find_deep_off = zero(getenv("SIGAX_FIND_DEEP"));                          // A/B aid: no deep start tables
  std::optional<int> deep_k = num(getenv("SIGAX_DEEP_K"));                       // test hook: K of the deep start tables
  std::optional<int> deep_load = num(getenv("SIGAX_DEEP_LOAD"));                 // test hook: their load factor in per cent
  bool find_deep_use_off = zero(getenv("SIGAX_FIND_DEEP_USE"));                  // A/B aid: deep tables built, not used
  u32 kmer_prefix = (u32)num(getenv("SIGAX_KMER_PREFIX")).value_or(13);          // product default 13: `siga correct`'s prefix table
  bool kmer_table_off = zero(getenv("SIGAX_KMER_TABLE"));                        // A/B aid: `siga correct` without its k-mer table
  bool cand_cap_worst = first(getenv("SIGAX_CAND_CAP")) == 'w';                  // A/B aid: "worst", round 2's candidate slots ...
  std::optional<int> cand_cap = num(getenv("SIGAX_CAND_CAP"));                   // test hook: ... or a number: slots of the first try
  std::optional<bool> find_coop = on_off(getenv("SIGAX_FIND_COOP"));             // A/B aid: cooperative finder off / on, untimed
  std::optional<u64> coop_min_symbols = unum(getenv("SIGAX_COOP_MIN_SYMBOLS"));  // A/B aid: cooperative finder from n symbols
  u64 coop_tune_min = unum(getenv("SIGAX_COOP_TUNE_MIN")).value_or(1ull << 30);  // test hook: lower end of the timed finder choice
  u32 find_coop_wgs = (u32)num(getenv("SIGAX_FIND_COOP_WGS")).value_or(0);       // measurement aid: cooperative grid per CU
  bool find_mask_upper_off = zero(getenv("SIGAX_FIND_MASK_UPPER"));              // A/B aid: every lane loads its upper line
  std::optional<bool> split_strands = on_off(getenv("SIGAX_SPLIT_STRANDS"));     // A/B aid: finder launches split by strand or not
  bool read_order = on_off(getenv("SIGAX_READ_ORDER")).value_or(false);          // experiment: locality order of a batch's reads
  std::optional<int> subbatches = num(getenv("SIGAX_SUBBATCHES"));               // A/B aid: sub-batches per run
  std::optional<int> fx_grid = num(getenv("SIGAX_FX_GRID"));                     // A/B aid: filter/extract workgroups
  unsigned fx_grid64 = (unsigned)std::max(1, num(getenv("SIGAX_FX_GRID64")).value_or(512));  // A/B aid: grid of the 64-lane launches
  bool general_only = set(getenv("SIGAX_GENERAL_ONLY"));                         // debugging aid: no fast filter/extract kernel
  bool fx_one_step = set(getenv("SIGAX_FX_ONE_STEP"));                           // A/B aid: extractor without the two-step table
  bool fx_skip_strict = set(getenv("SIGAX_FX_SKIP_STRICT"));                     // A/B aid: no strict lean launch
  std::optional<int> test_pool_cap = num(getenv("SIGAX_TEST_POOL_CAP"));         // test hook: first filter/extract pool size
  std::optional<u64> test_fin_cap = unum(getenv("SIGAX_TEST_FIN_CAP"));          // test hook: first block arena size
  std::optional<u64> test_edge_cap = unum(getenv("SIGAX_TEST_EDGE_CAP"));        // test hook: first edge arena size
  std::optional<int> test_piece = num(getenv("SIGAX_TEST_PIECE"));               // test hook: sigax_overlap_batch in pieces of n
  bool pool_poison = set(getenv("SIGAX_POOL_POISON"));                           // test hook: builders' reused blocks set to 0xA5
  bool build_timing = set(getenv("SIGAX_BUILD_TIMING"));                         // diagnostics: index builder phase times
  int order_bits = num(getenv("SIGAX_ORDER_BITS")).value_or(20);                 // experiment: class bits of the locality order
};
const Settings& settings();  // sigax_index.cpp

// ------------------------------------------------------------------------------------------------------
// index
// ------------------------------------------------------------------------------------------------------
struct sigax_index {
  int device;
  bool wide;
  FmStrand st[2];  // 0 forward (.bwt), 1 reverse (.rbwt); pointers are device pointers
  void* d_gran[2];
  void* d_gran2[2];  // two-step tables (fm_layout.h) or NULL
  void* d_super2[2]; // ... their superblock bases (64-bit positions) or NULL
  void* d_sa[2];     // row tables (fm_layout.h) or NULL
  void* d_text[2];   // stretch texts (fm_layout.h) or NULL
  void* d_xmap[2];   // direct maps (fm_layout.h) or NULL
  u64 sa_alloc[2], text_alloc[2];  // bytes allocated for them
  // The row tables of an index of 2^26 symbols and more are built by a side thread while the caller goes on (at BASELINE
  // configs[1] 0.1 s: more than the whole one-batch `siga overlap` spends on the GPU); runs enqueued before they are ready
  // use the forms without them -- same bytes out.  0 none / published, 1 being built, 2 built: tab_st waits for publishing.
  // Nor are they started before the index has been asked for as many reads as it holds (build_rowend): one pass of the
  // CLI would pay for tables that cost it more than they save.  tab_plan = bytes of the tables still to be allocated (sigax_batch_size_hint leaves them free).
  std::thread* tab_thread;
  std::atomic<int>* tab_state;
  FmStrand tab_st[2];
  u64 tab_bytes, tab_plan, reads_asked;
  bool tab_tried;  // the build has been started once (it is not tried again when memory was short)
  bool tab_text;
  bool tab_direct;   // direct maps instead of row tables (.sai tables present, ACGT-only reads)
  u32 tab_syms;      // symbols a row-table entry carries (plan)
  u32 max_read_len;  // longest read of sigax_index_set_reads (0: not told yet), an upper bound of the longest stretch
  void* d_super[2];
  void* d_start[2];  // start tables of the block finder (fm_layout.h) or NULL
  // Deep start tables (fm_layout.h): built by sigax_index_prepare_overlap, or on a side thread once the index is being
  // reused, for the min-overlap of the run at hand; deep_state 0 none / published, 1 being built, 2 built (deep_new waits
  // for publishing under enqueue_mu).  d_slen = the stretches' lengths by '$' rank (kept from the row tables' build).
  void* d_deep[2];
  u64 deep_slots[2], deep_bytes;
  uint32_t deep_k;
  uint32_t* d_slen[2];
  std::thread* deep_thread;
  std::atomic<int>* deep_state;
  void* deep_new[2];
  u64 deep_new_slots[2], deep_new_bytes;
  uint32_t deep_new_k;
  bool deep_tried;
  uint32_t ptab_k;
  void* d_ptab;      // intervals of all 12-mers of the forward index: `siga correct`'s k-mer lookups start there (built by the
  bool ptab_tried;   // first correction call; SIGAX_KMER_PREFIX=0: never)
  hipEvent_t ptab_ev;  // recorded behind the table's build on the first call's stream
  // `siga correct`'s k-mer table: the deep start table of the forward strand for K = the corrector's k (fm_layout.h) -- every
  // distinct k-mer of the reads with its number of occurrences, so FMIndex::Interval::occurrences (src/fmindex.h:80-86) of a
  // k-mer is ONE lookup, and a k-mer that is not in the table does not occur.  Built by the first correction call with that k
  // (ensure_kmer_table), from a forward row table + text of its own when the index has none.
  void* d_ktab;
  u64 ktab_slots, ktab_bytes;
  uint32_t ktab_k, ktab_tried_k;
  uint32_t csa_bits, cld_bits, ct_bits, ctext_stride;
  void *d_csa, *d_ctext;  // forward row table + stretch text built for it (fwd_only indexes, or before the extractor's exist)
  uint32_t* d_cslen;
  uint32_t* d_sai[2];
  u64 n_sai;
  uint32_t* d_read_len;
  uint32_t* d_name_rank;
  u64 n_meta;
  u64 n_symbols, n_strings, device_bytes;
  // The internal pipeline streams belong to the index, not to a batch: every batch on this index queues its finder
  // launches on s_find and its filter/extract launches on s_fx, so with two batches in flight batch B's first finder
  // launch runs beside batch A's last filter/extract launch and finder launches never run beside each other.
  hipStream_t s_find, s_fx, s_tail;
  hipStream_t s_ord;  // the locality ordering of a batch (a key kernel + some twenty launches of the radix sort, 1 ms of work
                      // per 2.5 M reads): high priority -- queued on the caller's stream beside the long kernels of the
                      // batches in flight it took 17 ms at the BASELINE configs[2] shape, all of it on the batch's own chain
  std::mutex* enqueue_mu;
  int n_cu;  // compute units of the device
  // The longest chain of candidate blocks any run on this index has produced so far.  The candidate arena gives every chain
  // that many slots plus headroom instead of the worst case (one per overlap length): BASELINE configs[1] 11 records per
  // chain on average, 30-odd at most, 106 in the worst case.  A run whose chains outgrow their slots is repeated with what
  // it reported (sigax_batch_finish).
  std::atomic<uint32_t>* cap_seen;
  bool split_strands;  // two-step tables too large to gather from both at once: one finder launch per strand
  bool fwd_only;       // opened without the reverse strand (what `siga correct` needs: src/correct.cpp loads <prefix>.bwt alone)
};

// The corrector's prefix table for a launch on `st`, if a correction call has built it (none is ever allocated for a match,
// spectrum or locate call): *ptab = NULL, *pk = 0 without one.  Its build may still be running on that call's stream, so `st`
// waits for it.
inline int ptab_for_stream(sigax_index* ix, hipStream_t st, const void** ptab, uint32_t* pk) {
  *ptab = nullptr;
  *pk = 0;
  std::lock_guard<std::mutex> lock(*ix->enqueue_mu);
  if (ix->d_ptab && ix->ptab_k) {
    if (ix->ptab_ev) HIP_TRY(hipStreamWaitEvent(st, ix->ptab_ev, 0));
    *ptab = ix->d_ptab;
    *pk = ix->ptab_k;
  }
  return SIGAX_OK;
}

// The strings of a _batch call (n >= 1 of them, `noun` each in the error text) to the device on `st`: offsets checked -- none
// descending, no item longer than max_item -- then *d_seqs (the bytes, 16 of slack behind them) and *d_offs allocated in `g`
// and copied.  offs[0] need not be 0 (a window of a longer table): the device gets the window's bytes and offsets from 0.
inline int stage_strings(DevGuard& g, const char* seqs, const uint64_t* offs, u64 n, u64 max_item, const char* noun, hipStream_t st,
                         unsigned char** d_seqs, u64** d_offs) {
  for (u64 i = 0; i < n; ++i)
    if (offs[i + 1] < offs[i] || offs[i + 1] - offs[i] > max_item) return sigax_fail(SIGAX_E_ARG, "%s %llu: bad offsets", noun, i);
  const u64 b0 = offs[0], nb = offs[n] - b0;
  std::vector<uint64_t> rebased;
  if (b0) {
    rebased.resize((size_t)n + 1);
    for (u64 i = 0; i <= n; ++i) rebased[i] = offs[i] - b0;
    offs = rebased.data();
  }
  HIP_TRY(g.alloc((void**)d_seqs, nb + 16));
  HIP_TRY(g.alloc((void**)d_offs, ((size_t)n + 1) * 8));
  HIP_TRY(hipMemcpyAsync(*d_seqs, seqs + b0, nb, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(*d_offs, offs, ((size_t)n + 1) * 8, hipMemcpyHostToDevice, st));
  if (b0) HIP_TRY(hipStreamSynchronize(st));  // `rebased` is about to go
  return SIGAX_OK;
}

// ---- sigax_tables.cpp: row tables, direct maps, stretch texts, deep start tables ----
struct RowTabGeom {
  u32 sa_bits, ld_bits, t_bits, text_stride;
  u64 sa_bytes, text_bytes;  // per strand
};
RowTabGeom row_tab_geom(const sigax_index* ix, u32 maxlen, u32 syms);
void plan_row_tables(sigax_index* ix);
void start_row_tables(sigax_index* ix, bool sync);
void publish_tables(sigax_index* ix);
void build_rowend(sigax_index* ix);
void row_tables_now(sigax_index* ix);
void publish_deep(sigax_index* ix);
void start_deep_tables(sigax_index* ix, uint32_t min_overlap);

#pragma GCC visibility pop
