// siga_amd/csrc/sigax_kernels.h -- argument blocks and launch wrappers that the kernel files (sigax_kernels.hip: finder,
// filter/extract, corrector; sigax_tables.hip: index tables; sigax_tail.hip: scan, ordered copy, edge records; and the files of
// the later commands) share with the host code that launches them
#ifndef SIGA_AMD_SIGAX_KERNELS_H_
#define SIGA_AMD_SIGAX_KERNELS_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sigax.h"
#include "fm_layout.h"

static_assert(sizeof(sigax_block) == 80, "sigax_block must be 5 x 16 bytes");
static_assert(sizeof(sigax_edge) == 16, "sigax_edge must be 16 bytes");

// slots of the per-batch device statistics / allocator block (u64 each, zeroed before every run)
enum {
  DS_OCC_FIND = 0,
  DS_CAND_BLOCKS,
  DS_FIND_OVERFLOW,
  DS_OCC_EXTRACT,
  DS_EXTRACT_ERRORS,
  DS_POOL_OVERFLOW,
  DS_SUBSTRING,
  DS_FIN_TOP,      // bump allocator of the unordered final-block arena (may run past fin_cap: needed size)
  DS_TOTAL_BLOCKS, // written by the scan: sum of per-read block counts
  DS_TOTAL_EDGES,  // written by the edge scan
  DS_SLOW_BASE,    // [DS_SLOW_BASE + i]: reads sub-batch i queued for the general kernel (i < SIGAX_MAX_SUB)
  DS_W64_BASE = DS_SLOW_BASE + 8,  // [DS_W64_BASE + i]: (read, side) items sub-batch i queued for the 64-lane launch
  DS_SEC_FIND = DS_W64_BASE + 8,   // distinct 64-byte sectors of the rank tables the finder asked for, step by step
  DS_SEC_EXTRACT,                  // ... filter/extract, round by round
  DS_MAX_CHAIN,                    // most candidate blocks any chain of the run pushed (also when its slots ran out)
  DS_BAD_IDS,                      // (read, side) items whose read id (sigax_batch_set_read_ids) is beyond the indexed read set
  DS_PROF_BASE = 32,               // 32 diagnostic counters (builds with -DSIGAX_FX_PROFILE only)
  DS_W64B_BASE = 64,               // [DS_W64B_BASE + i], [DS_W64C_BASE + i]: items in the second and third queue between
  DS_W64C_BASE = 72,               // sub-batch i's filter/extract launches
  DS_W64D_BASE = 80,               // ... in the fourth (what the 16-lane launch hands to the 32-lane one)
  DS_COUNT = 88
};
#define SIGAX_MAX_SUB 8

struct Ent;  // defined in sigax_kernels.hip, with filter/extract (48 bytes)
#define SIGAX_ENT_BYTES 48

struct FindArgs {
  FmStrand fwd, rev;
  const unsigned char* seqs;
  const unsigned long long* offs;
  uint32_t n_reads, minov, chain_mask, cap;  // chain_mask bit o = find o runs; cap = slots per chain, last = containment
  uint32_t max_seen;                 // chains no longer than this need not report their length (DS_MAX_CHAIN)
  uint32_t start_ok;                 // both strands carry the start table and min-overlap >= 12: chains may start twelve symbols in
  uint32_t deep_k;                   // both strands carry the deep start table with this K <= min-overlap (fm_layout.h), or 0
  uint32_t max_len;                  // the batch's longest read (sizes the per-lane finder's LDS budget)
  uint32_t read_begin, read_end;     // this launch's sub-batch
  uint32_t stage_bytes;              // dynamic LDS per workgroup that may hold the workgroup's reads (set by launch_find)
  uint32_t two_step;                 // both strands carry the two-step table (u32 positions only)
  uint32_t mask_upper;               // per-lane two-step finder: lanes whose upper position lies in the lower one's line do not load it again
  uint32_t coop, coop_stage_bytes;   // cooperative two-step finder (k_find_c2): lines staged through LDS; bytes for 64 reads
  uint32_t coop_grid;                // ... its grid cap (persistent workgroups walk the tiles), 0 = one workgroup per tile
  const uint32_t* perm;              // locality order of the batch: slot -> read (a permutation inside every sub-batch), or NULL
  uint32_t stage_stride;             // with perm: bytes per read in the LDS copy (>= the longest read, a multiple of 4)
  uint32_t chain_base, chains_per_wg; // a workgroup walks chains [chain_base, chain_base + chains_per_wg) (4, or 2: one strand's
                                     // table per launch) of 256 / chains_per_wg reads; chains outside are another launch's
  void* arena;                       // [n_reads][4][cap] candidate records of cand_bytes(wide) each
  uint32_t* chain_cnt;               // [n_reads][4]
  unsigned long long* dstat;
};

struct FxArgs {
  FmStrand fwd, rev;
  const unsigned long long* offs;
  uint32_t n_reads, cap, irreducible;
  uint32_t no_lean;   // skip the lean (single-group only) launches: the previous run of this batch object sent most items on
  const void* arena;
  const uint32_t* chain_cnt;
  unsigned long long n_map;  // entries of the strands' direct maps (= reads of the index)
  Ent* pool;          // [lanes][pool_cap]
  uint32_t pool_cap;
  const uint32_t* work;  // optional list of read ids; NULL = all reads
  unsigned long long n_work;
  const unsigned long long* n_work_ptr;  // if set, the list length is read from device memory
  Ent* wpool;         // fast kernel: [waves][fast_pool_entries_per_wave()]
  uint32_t* work_out; // fast kernel: reads queued for the general kernel, counted in *slow_counter
  unsigned long long* slow_counter;
  // fast kernels: three queues of (read, side) items between the launches of launch_filter_extract_fast, each counted
  // in its *counter; the first launch's count also tells the caller how many items needed more than the strict lean form
  uint32_t* work64;
  unsigned long long* w64_counter;
  uint32_t* work64b;
  unsigned long long* w64b_counter;
  uint32_t* work64c;
  unsigned long long* w64c_counter;
  uint32_t* work64d;
  unsigned long long* w64d_counter;
  // set per launch by launch_filter_extract_fast: input queue (NULL: the sub-batch's read range) and output queue (NULL:
  // the last launch, which queues reads for the general kernel)
  const uint32_t* q_in;
  const unsigned long long* q_in_n;
  uint32_t* q_out;
  unsigned long long* q_out_n;
  uint32_t* q_wide;  // optional: items with more blocks than the launch's lane group has lanes skip the next launch
  unsigned long long* q_wide_n;
  uint32_t read_begin, read_end;  // fast kernel: this launch's sub-batch
  sigax_block* fin;   // unordered final blocks, allocated in per-wave / per-lane chunks
  unsigned long long* item_base;  // [n_reads][2]: where a (read, side) item's blocks start in `fin`
  unsigned long long fin_cap;
  uint32_t* fin_cnt;  // [n_reads][2]: blocks of the suffix side (+ containments) and of the prefix side
  uint32_t* occ_side; // [n_reads][2]: what a completed fast side added to the statistics (taken back on redo)
  uint32_t* slow_flag;// [n_reads]: read queued for the general kernel
  uint8_t* substring; // [n_reads]
  unsigned long long* dstat;
};

struct OrderArgs {
  const sigax_block* fin;
  const unsigned long long* item_base;  // [n_items]
  const uint32_t* fin_cnt;              // [n_items]
  unsigned long long n_items;           // 2 * n_reads
  unsigned long long fin_cap;
  const unsigned long long* offs2;      // [n_items+1] per-(read, side) offsets in the ordered output
  sigax_block* out;
  unsigned long long out_cap;
  const void* arena;   // candidate records: a block whose `reserved` has bit 63 set carries (chain, slot) there instead
  uint32_t cap, wide;  // of its raw intervals, length and flags, which the scatter then takes from the candidate record
  // the batch's reads in the index's read table, when they carry ids (see EdgeArgs): an id >= n_index_reads is counted in
  // *bad_ids unless that is NULL (a run with edge records counts them in its stage pass)
  const uint32_t* read_ids;
  uint32_t n_index_reads;
  unsigned long long* bad_ids;
};

// the two edge passes (k_edges_stage, k_edges_emit) with the scan of item_edges into edge_offs between them
struct EdgeArgs {
  const sigax_block* fin;                // unordered final blocks, as the filter/extract kernels left them
  const unsigned long long* item_base;   // [n_items] where an item's blocks start in `fin`
  unsigned long long fin_cap;
  const void* arena;                     // candidate records (length and flags of the lane-group kernels' blocks)
  uint32_t cap, wide;
  const unsigned long long* offs2;       // [n_items+1] ordered index of each (read, side) item's first block
  const uint32_t* fin_cnt;               // [n_items] its blocks
  unsigned long long n_items;
  void* stage;                           // [stage_cap] 16-byte records by ordered block index
  unsigned long long stage_cap;
  uint32_t* item_edges;                  // [n_items] records per item (written by the stage pass)
  uint32_t read_base;
  // the batch's reads in the index's read table: read_base + i, or read_ids[i] (a rank's share of a key-range sharding:
  // any subset in any order); an id >= n_index_reads makes no edge and is counted in *bad_ids
  const uint32_t* read_ids;
  uint32_t n_index_reads;
  unsigned long long* bad_ids;
  const uint32_t* sai;
  const uint32_t* rsai;
  unsigned long long n_sai;
  const uint32_t* read_len;
  const uint32_t* name_rank;
  const unsigned long long* edge_offs;   // [n_items+1] scan of item_edges
  sigax_edge* edges;
  unsigned long long edge_cap;
};

#define CORRECT_NEVER 0xFFFFFFFFu
struct CorrectArgs {
  FmStrand fwd;
  const unsigned char* seqs;
  const unsigned char* quals;  // NULL: every base scores Quality::Phred::DEFAULT_SCORE (15)
  const unsigned long long* offs;
  unsigned long long n_reads;
  // CorrectThreshold: required support low / high (phred >= cutoff).  CORRECT_NEVER = a support no count reaches (what a
  // negative threshold is in the reference): kmer_occ's counts saturate one below it
  uint32_t k, low, high, cutoff, rounds, offset;
  unsigned char* out;    // corrected sequences, same layout as seqs
  unsigned char* valid;  // CorrectResult::validQC; 2 = read longer than the kernel supports
  unsigned long long* dstat;  // [0] reads too long, [1] rank-table sectors asked for, [2] k-mer lookups (4 x u64)
  const void* ktab;           // hash of the reads' distinct k-mers with their counts (fm_layout.h: deep start table, K = k), or NULL
  unsigned long long ktab_slots;
  const void* ptab;           // intervals of all pk-mers (launch_prefix_build), or NULL
  uint32_t pk;
  uint32_t max_len;           // upper bound of the batch's read lengths, 0 = unknown (launch_correct picks the kernel form)
  uint32_t only_deferred;     // set by launch_correct: this launch takes the reads the small form marked (valid = 3)
};
void launch_correct(const CorrectArgs& a, bool wide, hipStream_t st);
// table of the intervals of all pk-mers on strand s: prefix_table_bytes(wide, pk) bytes
unsigned long long prefix_table_bytes(bool wide, uint32_t pk);
void launch_prefix_build(const FmStrand& s, bool wide, void* tab, uint32_t pk, hipStream_t st);

// `siga match` (sigax_match.hip): occurrences of whole reads, or of their first and last max_length bases, on the forward strand
struct MatchArgs {
  FmStrand fwd;
  const unsigned char* seqs;
  const unsigned long long* offs;        // [n_reads + 1]
  unsigned long long n_reads;
  unsigned long long max_length;         // ~0: no read is split
  uint32_t rc;                           // also count the reverse complement
  uint32_t pk;                           // symbols of an entry of ptab
  const void* ptab;                      // the corrector's prefix table when it is resident (launch_prefix_build), or NULL
  unsigned long long* counts;            // [2 n_reads]: sigax_match_device
  unsigned long long* dstat;             // 4 u64, zeroed: chains run, symbols consumed, rank-table sectors asked for, the chain counter
};
void launch_match(const MatchArgs& a, bool wide, int n_cu, hipStream_t st);

// `siga preqc` (sigax_spectrum.hip).  Rows of strand s back to text: out == NULL is the lengths pass (lens, and unless NULL
// stretch), else the write pass (offs, out).  status (zeroed by the caller): rows out of range, walks cut, slots of the wrong size.
struct WalkArgs {
  FmStrand s;
  const unsigned long long* rows;        // [n]
  unsigned long long n;
  uint32_t max_len;
  uint32_t* lens;                        // [n]
  unsigned long long* stretch;           // [n] or NULL: Occ('$', end row - 1), ~0 for a walk that was cut or never started
  const unsigned long long* offs;        // [n + 1]
  unsigned char* out;
  unsigned long long* status;
};
void launch_walk(const WalkArgs& a, bool wide, hipStream_t st);
// k-mer count distribution of a batch of strings on the forward strand, both strands of every window
struct SpectrumArgs {
  FmStrand fwd;
  const unsigned char* seqs;
  const unsigned long long* offs;        // [n_reads + 1]
  unsigned long long n_reads;
  unsigned long long n_bins;
  uint32_t k;
  uint32_t pk;                           // symbols of an entry of ptab
  const void* ptab;                      // the corrector's prefix table when it is resident (launch_prefix_build), or NULL
  unsigned long long* hist;              // [n_bins], added to
  unsigned long long* dstat;             // 4 u64, zeroed: strings with len >= k, their bases, windows counted, rank-table sectors asked for
  unsigned long long* counter;           // 1 u64, zeroed: the kernel's string counter
};
void launch_spectrum(const SpectrumArgs& a, bool wide, int n_cu, hipStream_t st);

// `siga locate` (sigax_locate.hip).  Search: the two chains of every query -> chains[2q + strand] = {lower row, width}
// (zeroed by the caller: a chain that dies, or is not run, leaves its zeros).  Finish: totals, per-query flags and the widths
// that are listed (cnt), which launch_scan turns into hit_offs.  Walk: one LF walk per listed row -> its hit record.
struct LocateArgs {
  FmStrand fwd;
  const unsigned char* seqs;
  const unsigned long long* offs;        // [n_queries + 1]
  unsigned long long n_queries;
  uint32_t rc;                           // also the reverse complement's chain
  uint32_t pk;                           // symbols of an entry of ptab
  const void* ptab;                      // the corrector's prefix table when it is resident (launch_prefix_build), or NULL
  uint32_t max_hits, max_len;
  ulonglong2* chains;                    // [2 n_queries]
  unsigned long long* totals;            // [n_queries]
  uint32_t* qflags;                      // [n_queries]
  uint32_t* cnt;                         // [n_queries]: hits listed per query
  const unsigned long long* hit_offs;    // [n_queries + 1] (walk)
  sigax_hit* hits;                       // [hits_cap]
  unsigned long long* rows;              // [hits_cap] or NULL
  unsigned long long hits_cap;
  const uint32_t* sai;                   // [n_sai]
  unsigned long long n_sai;
  unsigned long long* status;            // 4 u64: [0] written by the scan; [1] walks cut and [2] sectors are added to (zeroed by the caller)
  unsigned long long* counters;          // 2 u64, zeroed: the search's chain counter, one reserved
};
void launch_locate_search(const LocateArgs& a, bool wide, int n_cu, hipStream_t st);
void launch_locate_finish(const LocateArgs& a, hipStream_t st);
void launch_locate_walk(const LocateArgs& a, bool wide, hipStream_t st);
// the slots the walk launches a lane for, min(hits_cap, n_queries * max_hits), and the most a grid of 256-lane workgroups holds
unsigned long long locate_walk_slots(unsigned long long n_queries, uint32_t max_hits, unsigned long long hits_cap);
static const unsigned long long LOCATE_MAX_SLOTS = 0x7FFFFFFFull * 256ull;

// `siga unitig` (sigax_unitig.hip): unbranched chains of overlaps compacted.  State 2r + e = read r left through end e (0 = B,
// prefix; 1 = E, suffix).  Everything below `status` is the caller's scratch (sigax_unitig.cpp lays it out).
enum { UNI_C_BAD = 0, UNI_C_LOW = 1, UNI_C_SIMPLE = 2, UNI_C_CYCLES = 3 };
struct UnitigArgs {
  const sigax_edge* edges;
  unsigned long long n_edges, n_reads;
  const uint32_t* lengths;               // [n_reads]
  const unsigned char* seqs;
  const unsigned long long* offs;        // [n_reads + 1]
  uint32_t min_overlap;
  unsigned long long* seq_offs;          // [n_reads + 1]
  unsigned long long* lay_offs;          // [n_reads + 1]
  uint32_t* uflags;                      // [n_reads]
  sigax_placement* layout;               // [n_reads]
  unsigned char* useqs;                  // offs[n_reads] - offs[0] bytes, or NULL: layout only
  unsigned long long* status;            // 6 u64, written
  uint32_t* deg;                         // [2 n_reads], zeroed: kept records per read end
  uint2* link;                           // [2 n_reads], 0xFF-filled: {end touched on the other read, overlap} of an end's simple record
  void* rank[2];                         // 2 x uint4[2 n_reads]: the ranking's ping-pong buffers ...
  unsigned long long* dist[2];           // 2 x [2 n_reads] ... and their base distances
  uint32_t* closing;                     // [n_reads], zeroed: a cut cycle's unitig flags, at its smallest read
  uint32_t* cnt;                         // 4 x [n_reads + 1]: per read {is a head, its unitig's reads, bases low, bases high}
  unsigned long long* scan;              // 4 x [n_reads + 1]: their prefix sums
  unsigned long long* partial;           // scan_partials_needed(n_reads) u64
  unsigned long long* scan_total;        // 1 u64
  unsigned long long* dst;               // [n_reads + 1]: where in useqs the bases placement i adds begin; [n_reads] = all bases
  unsigned long long* src;               // [n_reads]: the byte of seqs that goes there; bit 63: descending and complemented
  unsigned long long* counts;            // 4 u64, zeroed: UNI_C_*
};
// tip trimming and the lifted records (sigax_unitigs_trim_*): the unitig call's block and what the rounds and the lift need.  A
// block of its own, so that the kernels of sigax_unitigs_device keep the argument block they had.
struct UnitigTrimArgs : UnitigArgs {
  uint32_t* removed;                     // [n_reads], zeroed before round 1: the round in which a read went, 0 = alive
  uint32_t* verdict;                     // [n_reads]: a round's decision, under the unitig's head
  uint32_t* umap;                        // [n_reads]: (unitig << 1) | placed reversed, 0xFFFFFFFF for a removed read
  unsigned long long* trim;              // TRIM_WORDS u64, zeroed before round 1: the TRIM_C_* counters (counter_slot), the lifted records at
                                         // TRIM_LIFTED, and at TRIM_ROUND0 + r whether round r removed something
  uint32_t round;                        // 1 .. max_rounds: a trim round; 0: the pass that writes the result
  uint32_t min_branch_length, min_branch_coverage;
  sigax_edge* uedges;                    // [n_edges], or NULL: no lifted records
  uint32_t* eflag;                       // [n_edges]: the record is lifted
  unsigned long long* escan;             // [n_edges + 1]: where
  unsigned long long* epartial;          // scan_partials_needed(n_edges) u64
};
// A trim counter is TRIM_SLOTS partial sums 256 bytes apart, a wave adding to the slot of its number: where most unitigs go
// in a round nearly every wave adds, and adds to one address serialise.  Every counter block of the unitig, pairs
// and scaffold calls is laid out so: counter_words(n) words of n counters (counter_slot and counter_total of sigax_device.h), then
// the block's own tail; a step of the rounds keeps one flag per round there, at X_ROUND0 + r.
enum { TRIM_SLOTS = 32, TRIM_STRIDE = 32, TRIM_MAX_ROUNDS = 64 };
constexpr int counter_words(int n) { return n * TRIM_SLOTS * TRIM_STRIDE; }
enum { TRIM_C_ISLANDS = 0, TRIM_C_DEAD_ENDS = 1, TRIM_C_READS = 2, TRIM_C_DROPPED = 3, TRIM_COUNTERS = 4,
       TRIM_LIFTED = counter_words(TRIM_COUNTERS), TRIM_ROUND0 = TRIM_LIFTED + 8, TRIM_WORDS = TRIM_ROUND0 + TRIM_MAX_ROUNDS + 8 };
static const uint32_t TRIM_NO_COVERAGE = 0xFFFFFFFFu;
// non-maximal overlap cutting (sigax_unitigs_prune_*): the trim block and what a round's cut step needs.  Again a block of its
// own: the kernels of the two older entry points keep theirs.
struct UnitigPruneArgs : UnitigTrimArgs {
  uint32_t* cut;                         // [n_edges], zeroed before round 1: the round in which a record was cut, 0 = not cut
  uint32_t* maxlen;                      // [2 n_reads], cleared by the cut step: the longest participant at a read end; NULL in every
                                         // other pass (the degree kernel then takes no maximum)
  uint32_t* maxself;                     // [2 n_reads], cleared (careful): the longest participant at a read end with both ends in one unitig
  uint32_t* uniq;                        // [n_reads]: the unitig counts as unique, under its head
  unsigned long long* keys;              // key_cap u64, all ones when empty (careful): (read end << 32) | head of the unitig at the other end, of
                                         // every participant within delta of that read end's maximum; open addressing
  unsigned long long key_cap;            // a power of two >= 4 n_edges: at most 2 n_edges keys go in
  unsigned long long* prune;             // PRUNE_WORDS u64, zeroed before round 1: the PRUNE_C_* counters, slotted as the trim counters
                                         // are, and at PRUNE_ROUND0 + r whether round r cut something
  uint32_t delta, careful;
  unsigned long long num_reads, genome_size;
  double uniq_threshold;
};
enum { PRUNE_C_CUT = 0, PRUNE_C_UNIQUE = 1, PRUNE_COUNTERS = 2, PRUNE_ROUND0 = counter_words(PRUNE_COUNTERS),
       PRUNE_WORDS = PRUNE_ROUND0 + TRIM_MAX_ROUNDS + 8 };
unsigned unitig_rounds(unsigned long long n_reads);  // ceil(log2 n_reads) + 1: the pointer-jumping launches of one ranking
void launch_unitigs(const UnitigArgs& a, hipStream_t st);
void launch_unitig_bases(const UnitigArgs& a, hipStream_t st);  // the last phase alone, over what launch_unitigs left (sigax_unitigs_bases_device)
// one trim round (a.round >= 1): the graph of the alive reads, the verdict per unitig, removed[] marked.  Its launches leave at
// once when the round before it removed nothing.  The caller resets deg, closing, counts and link before each round and
// before the launch_unitigs_trim (a.round = 0) that writes the result; launch_unitig_lift then writes uedges and status[6 .. 11].
void launch_trim_round(const UnitigTrimArgs& a, hipStream_t st);
void launch_unitigs_trim(const UnitigTrimArgs& a, hipStream_t st);
void launch_unitig_lift(const UnitigTrimArgs& a, hipStream_t st);
// one round's cut step (a.round >= 1, a.maxlen set): the graph of the live records, the longest participant per read end, the
// verdict per unitig, cut[] marked.  Then launch_prune_trim_round (a.maxlen = NULL): launch_trim_round over the records that are
// not cut.  Both leave at once when the round before changed nothing.  The caller resets as for launch_trim_round; the cut step
// clears maxlen, maxself and keys itself.  launch_unitigs_prune / launch_unitig_prune_lift: the result, and status[6 .. 15].
void launch_prune_cut_round(const UnitigPruneArgs& a, hipStream_t st);
void launch_prune_trim_round(const UnitigPruneArgs& a, hipStream_t st);
void launch_unitigs_prune(const UnitigPruneArgs& a, hipStream_t st);
void launch_unitig_prune_lift(const UnitigPruneArgs& a, hipStream_t st);
// chimeric unitig removal (sigax_unitigs_chimeric_*): the prune block and what a round's chimeric step needs.  The existing
// kernels take the prune block out of it (by value); only the kernels of the chimeric step see the rest.
struct UnitigChimericArgs : UnitigPruneArgs {
  uint32_t* nbr;                         // [2 n_reads], cleared by the step (all ones): at a read end of degree 1 whose record is a
                                         // participant, the read end at that record's other side
  unsigned long long* minb[2];           // 2 x [2 n_reads], cleared (all ones): per read end of degree >= 2 the smallest
                                         // (min(bases(U(b)), 2^32 - 1) << 32 | head(b)) over its participants' other ends b; [1]: the
                                         // smallest among those whose head is not [0]'s
  unsigned long long* mink[2];           // the same over (K(U(b)) << 32 | head(b))
  unsigned long long* chim;              // CHIM_WORDS u64, zeroed before round 1: the CHIM_C_* counters, slotted as the trim counters are,
                                         // and at CHIM_ROUND0 + r whether round r's chimeric step removed something
  unsigned long long* prune_aside;       // PRUNE_WORDS u64: where the scoring pass of a chimeric step counts (status[14] is the cut step's)
  uint32_t min_chimeric_length, min_chimeric_coverage, chimeric_delta;
  double chimeric_threshold;
};
enum { CHIM_C_UNITIGS = 0, CHIM_C_READS = 1, CHIM_COUNTERS = 2, CHIM_ROUND0 = counter_words(CHIM_COUNTERS),
       CHIM_WORDS = CHIM_ROUND0 + TRIM_MAX_ROUNDS + 8 };
static const uint32_t REMOVED_CHIMERIC = 0x80000000u;
// one round's chimeric step (a.round >= 1, a.maxlen = NULL), after launch_prune_trim_round: the graph of the live records, every
// unitig scored under chimeric_threshold, the neighbours and the two minima per read end, the verdict per unitig, removed[] marked
// with REMOVED_CHIMERIC.  Leaves at once when the round before changed nothing.  The caller resets as for launch_trim_round; the
// step clears nbr, minb and mink itself.  launch_chimeric_status: status[16 .. 19], after launch_unitig_prune_lift.
void launch_chimeric_round(const UnitigChimericArgs& a, hipStream_t st);
void launch_chimeric_status(const UnitigChimericArgs& a, hipStream_t st);
// bubble popping (sigax_unitigs_bubble_*): the chimeric block and what a round's bubble step needs.  The existing kernels take the
// block they know out of it (by value); only the kernels of the bubble step see the rest.
struct UnitigBubbleArgs : UnitigChimericArgs {
  uint32_t* bnbr;                        // [2 n_reads], cleared by the step (all ones): at a read end of degree 1 whose record is a
                                         // participant, the read end at that record's other side ...
  uint32_t* blen;                        // [2 n_reads] ... and that record's length
  uint4* arm;                            // [n_reads], under a head: {lo, hi, span, o_lo} of an arm that takes part
  uint32_t* aside;                       // [n_reads], under a head: 1 = the unitig's left end is the one joined to lo
  uint32_t* gslot;                       // [n_reads], under a head: the table slot of the arm's group, all ones = takes no part
  uint32_t* table;                       // group_cap u32, cleared (all ones): the head of the arm that opened the group; open
                                         // addressing over a hash of (lo, hi, span)
  unsigned long long* best;              // group_cap u64, cleared (0): the largest (K << 32) | ~head over the group's arms
  unsigned long long group_cap;          // a power of two >= 2 n_reads: at most n_reads groups go in
  uint32_t* losers;                      // [n_reads]: the heads of the arms that wait for the bases test, as appended
  uint4* where;                          // [n_reads]: the step's own layout, per placement {read | placed reversed << 31, its overlap with the
                                         // read before it, low and high half of where in its unitig the bases it adds begin}
  unsigned long long* bub;               // BUB_WORDS u64, zeroed before round 1: the BUB_C_* counters, slotted as the trim counters are;
                                         // the appended losers at BUB_APPENDED; at BUB_ROUND0 + r whether round r's step removed something
  uint32_t max_bubble_span, max_divergence_permille;
};
enum { BUB_C_POPPED = 0, BUB_C_READS = 1, BUB_C_KEPT = 2, BUB_COUNTERS = 3, BUB_APPENDED = counter_words(BUB_COUNTERS),
       BUB_ROUND0 = BUB_APPENDED + 8, BUB_WORDS = BUB_ROUND0 + TRIM_MAX_ROUNDS + 8, BUB_COMPARE_WAVES = 8192 };
static const uint32_t REMOVED_BUBBLE = 0x40000000u;
static const uint32_t BUBBLE_NO_BASES = 0xFFFFFFFFu;
// one round's bubble step (a.round >= 1, a.maxlen = NULL), after launch_prune_trim_round and before launch_chimeric_round: the graph of
// the live records, the arms and their groups, a group's winner, the bases test of every other arm, removed[] marked with
// REMOVED_BUBBLE.  Its kernels leave at once when the round before changed nothing.  The caller resets as for launch_trim_round; the
// step clears its own scratch.  launch_bubble_status: status[20 .. 23], after launch_chimeric_status.
void launch_bubble_round(const UnitigBubbleArgs& a, hipStream_t st);
void launch_bubble_status(const UnitigBubbleArgs& a, hipStream_t st);
// indel bubble popping (sigax_unitigs_indel_*): the bubble block and what a round's indel step needs.  The step runs after the bubble
// step over the same scratch (neighbours, arms, placements, group table, verdicts); only its own kernels see the fields below.
struct UnitigIndelArgs : UnitigBubbleArgs {
  uint32_t* pairs;                       // [n_reads]: the heads of the losers that wait for the edit distance, as appended
  unsigned long long* ind;               // IND_WORDS u64, zeroed before round 1: the IND_C_* counters, slotted as the trim counters are;
                                         // the appended pairs at IND_APPENDED; at IND_ROUND0 + r whether round r's step removed something
  uint32_t max_edits, max_edit_permille;
};
enum { IND_C_POPPED = 0, IND_C_READS = 1, IND_C_KEPT = 2, IND_C_SKIPPED = 3, IND_COUNTERS = 4,
       IND_APPENDED = counter_words(IND_COUNTERS), IND_ROUND0 = IND_APPENDED + 8, IND_WORDS = IND_ROUND0 + TRIM_MAX_ROUNDS + 8,
       IND_MAX_SPAN = 4096, IND_MAX_EDITS = 31 };
static const uint32_t REMOVED_INDEL = 0x20000000u;
// one round's indel step (a.round >= 1, a.maxlen = NULL, 0 < a.max_bubble_span <= IND_MAX_SPAN, 0 < a.max_edits <= IND_MAX_EDITS), after
// launch_bubble_round and before launch_chimeric_round: the graph of the live records, the arms as the bubble step finds them, their
// groups by (lo, hi) alone, a group's winner, the bounded edit distance of every other arm whose span is within max_edits of the
// winner's and not equal to it, removed[] marked with REMOVED_INDEL.  Its kernels leave at once when the round before changed nothing.
// The caller resets as for launch_trim_round; the step clears its own scratch.  launch_indel_status: status[24 .. 31], after
// launch_bubble_status.
void launch_indel_round(const UnitigIndelArgs& a, hipStream_t st);
void launch_indel_status(const UnitigIndelArgs& a, hipStream_t st);
// transitive reduction (sigax_unitigs_reduce_*): the indel block and what a reduction pass needs.  A pass flags records in cut[]
// (CUT_TRANSITIVE); every older kernel already takes a record with cut[i] != 0 as not there.  Only the pass's kernels see the fields below.
struct UnitigReduceArgs : UnitigIndelArgs {
  unsigned long long* red;               // RED_WORDS u64, zeroed before the first pass: the RED_C_* counters of the pass that ran last,
                                         // slotted as the trim counters are, and the call's counts at RED_FIRST .. RED_PASSES
  uint32_t* rcnt;                        // [2 n_reads + 1]: participants per state
  uint32_t* rfill;                       // [2 n_reads]: how many entries of a state's segment are written
  unsigned long long* roff;              // [2 n_reads + 1]: where a state's segment of the adjacency begins
  unsigned long long* rpartial;          // scan_partials_needed(2 n_reads) u64
  unsigned long long* rtotal;            // 1 u64
  uint2* radj;                           // [2 n_edges]: {the state at the other side, the extension towards it}, by state
  uint32_t* rtable;                      // [red_cap]: open addressing over (state, state, overlap); an entry names a participant record
  unsigned long long red_cap;            // a power of two, at least 4 n_edges
  uint32_t red_prev;                     // the round before this pass (0: none); the pass is idle when that round changed nothing
};
enum { RED_C_FLAGGED = 0, RED_C_PART = 1, RED_COUNTERS = 2, RED_FIRST = counter_words(RED_COUNTERS), RED_LAST = RED_FIRST + 1,
       RED_PASSES = RED_FIRST + 2, RED_LAST_PART = RED_FIRST + 3, RED_WORDS = RED_FIRST + 8 };
static const uint32_t CUT_TRANSITIVE = 0x80000000u;
// One reduction pass over the records as removed[] and the low bits of cut[] stand (a.maxlen = NULL, n_edges < 2^32): bit 31 of every
// cut[i] cleared, the participants counted per state, launch_scan, the adjacency and the table filled, then one lane per participant
// walks the segments of its two states and probes the table; bit 31 set where a third read explains the record.  a.red_prev names the
// round whose flag decides whether the pass is idle; an idle pass writes nothing.  launch_reduce_status: status[32 .. 39], after
// launch_indel_status.
void launch_reduce_pass(const UnitigReduceArgs& a, hipStream_t st);
void launch_reduce_status(const UnitigReduceArgs& a, hipStream_t st);

// `siga unitig --pairs` (sigax_pairs.hip): mate-pair statistics and links over the layout a unitig call left.  Everything below
// `status` is the caller's scratch (sigax_pairs.cpp lays it out).
struct PairArgs {
  const uint32_t* mate;                  // [n_reads]
  const uint32_t* lengths;               // [n_reads]
  unsigned long long n_reads;
  const unsigned long long* n_unitigs;   // 1 u64 on the device: the unitig call's status[0]
  const unsigned long long* seq_offs;    // [n_reads + 1]
  const unsigned long long* lay_offs;    // [n_reads + 1]
  const uint32_t* uflags;                // [n_reads]
  const sigax_placement* layout;         // [n_reads]
  uint32_t flags, hist_bins, hist_shift;
  unsigned long long max_span;
  unsigned long long* hist;              // [hist_bins], zeroed
  sigax_pair_link* links;                // [cap]
  unsigned long long* status;            // 24 u64, written
  unsigned long long* where;             // [n_reads], zeroed: (unitig << 32) | (placement + 1) of a read, 0 = not placed
  unsigned long long* cnt;               // PAIR_WORDS u64, zeroed: counter c = status entry c, slotted as the trim counters are; the
                                         // appended link entries at PAIR_APPENDED
  unsigned long long cap;                // n_reads / 2: the most pairs there can be
  unsigned long long* keys[2];           // 2 x [cap]: [0] the appended link keys (a << 32) | b, all ones where empty; [1] sorted
  unsigned long long* vals[2];           // 2 x [cap]: their s, as appended and as sorted
  uint32_t* head;                        // [cap]: a sorted entry begins a run of equal keys
  unsigned long long* scan;              // [cap + 1]: the heads before it
  unsigned long long* partial;           // scan_partials_needed(cap) u64
  unsigned long long* scan_total;        // 1 u64, zeroed: the records
  void* sort_tmp;                        // pairs_sort_bytes(cap) bytes
  unsigned long long sort_tmp_bytes;
};
enum { PAIR_COUNTERS = 22, PAIR_APPENDED = counter_words(PAIR_COUNTERS), PAIR_WORDS = PAIR_APPENDED + 8, PAIR_HIST_MAX = 8192,
       PAIR_READS_PER_BLOCK = 1024 };
// bytes of scratch the device sort of `cap` (key, value) entries asks for: a size query, launches nothing
hipError_t pairs_sort_bytes(unsigned long long cap, unsigned long long* bytes);
hipError_t launch_pairs(const PairArgs& a, hipStream_t st);

// `siga unitig --scaffold` (sigax_scaffold.hip): unitigs joined through the link records of the pairs call.  Everything below
// `status` is the caller's scratch (sigax_scaffold.cpp lays it out).  nu = min(*n_unitigs, max_unitigs), nl likewise.
struct ScaffoldArgs {
  const unsigned long long* n_unitigs;   // on the device
  const unsigned long long* n_links;     // on the device
  unsigned long long max_unitigs, max_links;
  const unsigned long long* seq_offs;    // [max_unitigs + 1]
  const uint32_t* uflags;                // [max_unitigs]
  const unsigned char* useqs;            // useqs_bytes bytes: nothing at or beyond them is read
  unsigned long long useqs_bytes;
  const sigax_pair_link* links;          // [max_links]
  const unsigned long long* status24;    // of the pairs call
  uint32_t flags, min_pairs, link_ratio, min_unitig_bases, min_gap, max_gap;
  unsigned long long insert_size;
  unsigned long long* sc_offs;           // [max_unitigs + 1]
  unsigned long long* sc_lay_offs;       // [max_unitigs + 1]
  uint32_t* sc_flags;                    // [max_unitigs]
  sigax_placement* sc_layout;            // [max_unitigs]
  unsigned char* sseqs;                  // sseqs_capacity bytes or NULL
  unsigned long long sseqs_capacity;
  unsigned long long* status;            // 16 u64, written
  unsigned long long* cnt;               // SCAF_WORDS u64: counter c = status entry c, slotted as the trim counters are
  uint32_t* best;                        // [2 max_unitigs]: the largest count among the candidates of a unitig end
  uint32_t* deg;                         // [2 max_unitigs]: its strong candidates
  uint2* link;                           // [2 max_unitigs]: {the unitig end its join leads to or NIL, the join's gap}
  uint32_t* closing;                     // [max_unitigs]: a cycle's flag word under its smallest unitig
  unsigned long long* rank[2];           // 2 x [2 max_unitigs] uint4
  unsigned long long* dist[2];           // 2 x [2 max_unitigs]
  uint32_t* hcnt;                        // 4 x [max_unitigs + 1]: per unitig {is a head, its scaffold's unitigs, bases low, high}
  unsigned long long* scan;              // 4 x [max_unitigs + 1]: their prefix sums
  unsigned long long* partial;           // scan_partials_needed(max_unitigs) u64
  unsigned long long* scan_total;        // 1 u64
  unsigned long long* pdst;              // [max_unitigs + 1]: where in sseqs placement i's unitig begins; [placements] = all bases
  unsigned long long* psrc;              // [max_unitigs]: where in useqs it lies | reversed << 63
  unsigned long long* plen;              // [max_unitigs]: its bases
};
// counters 2-14 are status entries; SCAF_C_CLOSING_GAPS sums the gaps of the joins that close cycles
enum { SCAF_C_CLOSING_GAPS = 0, SCAF_COUNTERS = 16, SCAF_ANY_CUT = counter_words(SCAF_COUNTERS), SCAF_WORDS = SCAF_ANY_CUT + 8 };
hipError_t launch_scaffold(const ScaffoldArgs& a, hipStream_t st);
void launch_scaffold_bases(const ScaffoldArgs& a, hipStream_t st);  // the last phase alone, over what launch_scaffold left

// `siga unitig --scaffold --gapfill` (sigax_gapfill.hip): scaffold gaps closed by k-mer walks on the forward strand.  Everything
// below `status` is the caller's scratch (sigax_gapfill.cpp lays it out).  n = max_unitigs; nu, S and P are clamped to it.
struct GapfillArgs {
  FmStrand fwd;
  const unsigned long long* n_unitigs;   // on the device
  const unsigned long long* n_scaffolds; // on the device
  unsigned long long max_unitigs;
  const unsigned long long* seq_offs;    // [n + 1]
  const unsigned char* useqs;            // useqs_bytes bytes: nothing at or beyond them is read
  unsigned long long useqs_bytes;
  const unsigned long long* sc_lay_offs; // [n + 1]
  const sigax_placement* sc_layout;      // [n]
  uint32_t k, min_count, slack, max_fill;
  unsigned long long* sc_offs;           // [n + 1], written
  sigax_placement* sc_layout_out;        // [n], written
  unsigned char* sseqs;                  // sseqs_capacity bytes or NULL
  unsigned long long sseqs_capacity;
  sigax_gap* gaps;                       // [n], written
  unsigned long long* status;            // 24 u64, written
  unsigned long long* cnt;               // GAP_WORDS u64, zeroed: the GAP_C_* counters and the walk kernel's chain counter
  uint32_t* sof;                         // [n]: the scaffold of a placement
  uint32_t* isgap;                       // [n]: placement p and p + 1 are a gap ...
  uint32_t* need;                        // [n]: ... the bytes of walk scratch it needs (0: it is not walked)
  uint32_t* fillc;                       // [n]: its fill when filled, else 0 ...
  uint32_t* remc;                        // [n]: ... and the N that the fill replaces
  uint32_t* lenlo;                       // [n]: the new bases of scaffold s, low and ...
  uint32_t* lenhi;                       // [n]: ... high half
  unsigned long long* gnum;              // [n + 1]: scans of the six, in that order
  unsigned long long* soff;
  unsigned long long* fsum;
  unsigned long long* rsum;
  unsigned long long* slo;
  unsigned long long* shi;
  unsigned long long* partial;           // scan_partials_needed(n) u64
  unsigned long long* scan_total;        // 1 u64
  uint2* gres;                           // [n]: {class | fwd << 8 | rev << 16 | dir << 24, fill}; class GAP_WALK before the walks
  unsigned long long* gap_g;             // [n]: G
  unsigned long long* win;               // [16 n]: per placement four windows of four words, 2 bits a base, base i at bit 2 i:
                                         // the forward walk's start and goal, the reverse walk's start and goal
  unsigned long long* pdst;              // [n + 1]: where in sseqs placement p's unitig begins; [P] = all bases
  unsigned long long* psrc;              // [n]: where in useqs it lies | reversed << 63
  unsigned long long* plen;              // [n]: its bases (0 for a bad placement)
  unsigned char* walk;                   // max_walk_bases bytes: the bases a walk appends, as appended
  unsigned long long max_walk_bases;
};
// counters 0 .. 10 are the classes; GAP_CHAIN is the persistent kernel's chain counter
enum { GAP_C_FWD = 11, GAP_C_REV = 12, GAP_C_FILL = 13, GAP_C_NLEFT = 14, GAP_C_STEPS = 15, GAP_C_SECTORS = 16, GAP_C_GAPS = 17, GAP_CHAIN = 24,
       GAP_WORDS = 32 };
static const uint32_t GAP_WALK = 0xFFu, GAP_NONE = 0xFEu;  // gres classes before the walks: to be walked, no gap here
hipError_t launch_gapfill(const GapfillArgs& a, bool wide, int n_cu, hipStream_t st);
void launch_gapfill_bases(const GapfillArgs& a, hipStream_t st);  // the last phase alone, over what launch_gapfill left

// `siga unitig --scaffold --join-overlaps` (sigax_join.hip): scaffold neighbours that overlap written as one sequence.  Everything
// below `status` is the caller's scratch (sigax_join.cpp lays it out).  n = max_unitigs; nu, S and P are clamped to it.
struct JoinArgs {
  FmStrand fwd;
  const unsigned long long* n_unitigs;   // on the device
  const unsigned long long* n_scaffolds; // on the device
  unsigned long long max_unitigs;
  const unsigned long long* seq_offs;    // [n + 1]
  const unsigned long long* sc_offs_in;  // [n + 1]
  const unsigned long long* sc_lay_offs; // [n + 1]
  const sigax_placement* sc_layout;      // [n]
  const unsigned char* sseqs_in;         // sseqs_bytes bytes: nothing at or beyond them is read
  unsigned long long sseqs_bytes;
  uint32_t min_overlap, max_overlap, slack, k, min_count;
  unsigned long long* sc_offs;           // [n + 1], written
  sigax_placement* sc_layout_out;        // [n], written
  unsigned char* sseqs;                  // sseqs_capacity bytes or NULL
  unsigned long long sseqs_capacity;
  sigax_join* joins;                     // [n], written
  unsigned long long* status;            // 16 u64, written
  unsigned long long* cnt;               // JOIN_WORDS u64, zeroed: the JOIN_C_* counters
  uint32_t* sof;                         // [n]: the scaffold of a placement
  uint32_t* isgap;                       // [n]: placement p and p + 1 are a gap ...
  uint32_t* open;                        // [n]: ... that comes to the match
  uint32_t* rem;                         // [n]: G + v of a joined gap, else 0
  uint32_t* lenlo;                       // [n]: the new bases of scaffold s, low and ...
  uint32_t* lenhi;                       // [n]: ... high half
  unsigned long long* gnum;              // [n + 1]: scans of isgap, open, rem, lenlo, lenhi
  unsigned long long* onum;
  unsigned long long* esum;
  unsigned long long* slo;
  unsigned long long* shi;
  unsigned long long* partial;           // scan_partials_needed(n) u64
  unsigned long long* scan_total;        // 1 u64
  uint32_t* list;                        // [n]: the placements whose gap comes to the match, in order
  uint4* gres;                           // [n]: {class | matches << 8 | windows << 16, v, G saturated, hi}; class JOIN_OPEN before the match,
                                         // JOIN_UNIQUE between the match and the support test
  unsigned long long* plen;              // [n]: bases(p) (0 for a bad placement)
  unsigned long long* psrc;              // [n]: where in sseqs_in X(p) begins
  unsigned long long* pkey;              // [n + 1]: the output byte from which placement p's shift holds; [P] = all bases
  unsigned long long* pshift;            // [n]: output byte x of that stretch is input byte x + pshift[p] (modulo 2^64)
  // `--join-mismatches` (sigax_join_approx_*): all zero and NULL in a sigax_join_* call, which writes 16 status entries
  uint32_t max_mismatches, mismatch_permille;
  uint32_t n_status;                     // 16 or 24
  uint32_t* mm;                          // [n], written per gap: mismatches | taken_right << 8 | approximate << 16; or NULL
  unsigned long long* acnt;              // JOIN_AWORDS u64, zeroed: the JOIN_A_* counters
  uint16_t* cols;                        // [16 n]: the mismatch columns j_0 < j_1 < ... of a gap with one approximate v
  uint32_t* ainfo;                       // [n]: mm of the gap at placement p, 0 where the exact match decided
  uint32_t* amask;                       // [n]: bit i set where column i takes R's base
};
// counters 0 .. 7 are the classes
enum { JOIN_C_GAPS = 8, JOIN_C_OVERLAP = 9, JOIN_C_N = 10, JOIN_C_CAND = 11, JOIN_C_WINDOWS = 12, JOIN_WORDS = 16 };
enum { JOIN_A_JOINED = 0, JOIN_A_COLUMNS = 1, JOIN_A_RIGHT = 2, JOIN_A_CAND = 3, JOIN_A_CHOICE = 4, JOIN_AWORDS = 8 };  // status 16 + c
enum { JOIN_MAX_COLUMNS = 16 };
// JOIN_APPROX: one approximate v, between the match and the support test (the choice in between leaves the class as it is)
static const uint32_t JOIN_OPEN = 0xFFu, JOIN_NO_GAP = 0xFEu, JOIN_UNIQUE = 0xFDu, JOIN_APPROX = 0xFCu;
hipError_t launch_join(const JoinArgs& a, bool wide, int n_cu, hipStream_t st);
void launch_join_bases(const JoinArgs& a, hipStream_t st);  // the last phase alone, over what launch_join left (the patches with it)

void launch_occ_batch(const FmStrand& s, bool wide, const unsigned long long* pos, unsigned long long n,
                      unsigned long long* out, hipStream_t st);
void launch_kmer_count(const FmStrand& s, bool wide, const unsigned char* kmers, uint32_t k, unsigned long long n,
                       unsigned long long* out, hipStream_t st);
void launch_find(const FindArgs& a, bool wide, hipStream_t st);
// rows of strand s in suffix order?  bad3 (device, zeroed except [1] = ~0): pairs out of order, first such row, undecided pairs
void launch_suffix_order_check(const FmStrand& s, const uint32_t* sai, uint32_t* isai_tmp, const uint32_t* read_len,
                               unsigned long long n_strings, unsigned long long* bad3, hipStream_t st);
// start table of the finder for chains whose primary index is `prim` (fm_layout.h): start_table_bytes(wide) bytes
unsigned long long start_table_bytes(bool wide);
void launch_start_build(const FmStrand& prim, const FmStrand& other, bool wide, void* tab, hipStream_t st);
// deep start table of strand `prim` as primary index (fm_layout.h).  launch_deep_scan: *count (zeroed by the caller) += the
// distinct K-mers of s's text = the runs of rows with equal K-symbol prefixes; with list != NULL each run's first row goes
// to list[] (any order, at most list_cap).  launch_deep_fill: their states into tab (nslots entries of deep_entry_bytes(),
// zeroed by the caller); *err (zeroed) counts K-mers whose walk did not come out at their own rows.  slen = the stretches'
// lengths by '$' rank (launch_rows_fill).
unsigned long long deep_entry_bytes();
void launch_deep_scan(const FmStrand& s, const uint32_t* slen, unsigned long long n_stretch, uint32_t K, unsigned long long* count,
                      unsigned long long* list, unsigned long long list_cap, hipStream_t st);
void launch_deep_fill(const FmStrand& prim, const FmStrand& other, bool wide, const uint32_t* slen, unsigned long long n_stretch, uint32_t K,
                      const unsigned long long* list, unsigned long long n_list, void* tab, unsigned long long nslots, unsigned long long* err,
                      hipStream_t st);
unsigned long long find_stage_capacity(unsigned max_len);  // bytes of reads a finder workgroup can stage in LDS (batch's longest read given)
void launch_filter_extract(const FxArgs& a, bool wide, unsigned grid, hipStream_t st);
// qhint: items the four queues held last time (per sub-batch; ~0 = unknown), or NULL
void launch_filter_extract_fast(const FxArgs& a, bool wide, unsigned grid32, unsigned grid64, const unsigned long long* qhint, hipStream_t st);
unsigned long long fast_pool_entries_per_wave();
// offs[0..n] = exclusive scan of cnt[0..n), *total_out = offs[n]; partial: scan_partials_needed(n) u64 of scratch.
// even_out (n even), or NULL: even_out[i] = offs[2i] for i <= n / 2
void launch_scan(const uint32_t* cnt, unsigned long long n, unsigned long long* partial, unsigned long long* offs,
                 unsigned long long* total_out, hipStream_t st, unsigned long long* even_out = nullptr);
unsigned long long scan_partials_needed(unsigned long long n);
// Two-step table of one strand (fm_layout.h): gran2 = (n/64+1) x 32 u32; cnt = 20 x (n/64+1) u32, offs = (n/64+2) u64,
// partial = scan_partials_needed(n/64+1) u64, total = 1 u64 of scratch.
void launch_build2(const FmStrand& s, bool wide, uint32_t* gran2, unsigned long long* super2, uint32_t* cnt, unsigned long long* offs, unsigned long long* partial,
                   unsigned long long* total, hipStream_t st);
// Row table + stretch text of one strand (fm_layout.h), two walks over every stretch (n_stretch = C['A'] of them):
// launch_stretch_scan fills info[n_stretch] and *maxlen (zeroed by the caller) = the longest stretch, from which the caller
// sizes the entries; launch_rows_fill writes the table (zeroed by the caller, n * sa_bits bits + 16 bytes; or sa = NULL), unless
// NULL the text rows, and unless NULL the stretches' lengths by their rank among the '$' rows.
void launch_stretch_scan(const FmStrand& s, bool wide, unsigned long long n_stretch, unsigned long long* info, uint32_t* maxlen, hipStream_t st);
void launch_rows_fill(const FmStrand& s, bool wide, unsigned long long n_stretch, const unsigned long long* info, unsigned char* sa,
                      uint32_t sa_bits, uint32_t ld_bits, uint32_t t_bits, unsigned char* text, uint32_t text_stride, uint32_t* slen,
                      hipStream_t st);
// direct map of strand X as extension index (fm_layout.h) from the other strand's .sai ids (sai_y), X's own (sai_x; isai_tmp =
// n u32 of scratch for its inverse) and X's stretch lengths by '$' rank (slen_x, written by launch_rows_fill)
void launch_xmap(const uint32_t* sai_y, const uint32_t* sai_x, uint32_t* isai_tmp, const uint32_t* slen_x, unsigned long long n,
                 unsigned long long* xmap, hipStream_t st);
void launch_order_scatter(const OrderArgs& a, hipStream_t st);
unsigned long long fast_fin_chunk();
unsigned long long cand_bytes(bool wide);
void launch_edges_stage(const EdgeArgs& a, hipStream_t st);
void launch_edges_emit(const EdgeArgs& a, hipStream_t st);
// sigax_index_build.hip: locality order of a batch's reads (a permutation inside each of the nsub slot ranges bounds[0..nsub]),
// queued on `st` without a host wait.  keys = n u32 of scratch, vals = n u32 = the order once the stream gets there
// (*result = vals), tmp = sigax_order_reads_tmp_bytes(nsub) bytes for the class counters.
size_t sigax_order_reads_tmp_bytes(uint32_t nsub);
int sigax_order_reads(const unsigned char* d_seqs, const unsigned long long* d_offs, uint32_t n, uint32_t max_len, const uint32_t* bounds, uint32_t nsub,
                      uint32_t* keys, uint32_t* vals, void* tmp, size_t tmp_bytes, const uint32_t** result, hipStream_t st);

#endif
