/* include/sigax.h -- C-ABI of the MI355X-native `siga overlap` hot path.
 *
 * The reference (chungongyu/siga) has no FFI layer: the seam this library replaces is the C++ class
 * OverlapBuilder (src/overlap_builder.h:19-45) as used by Overlapping::run (src/overlap.cpp:41-47) and the
 * per-read call OverlapBuilder::overlap() that parallel::foreach drives (src/overlap_builder.cpp:269-280,
 * 453-457; src/parallel_framework.h:16-59).  The batch entry points below are "overlap() for a batch of
 * reads"; index lifetime replaces FMIndex::load (src/fmindex.cpp:353-366) + SuffixArray::load
 * (src/suffix_array.cpp:104-118).  Plain pointers and sizes only; nothing throws across this boundary;
 * every function returns SIGAX_OK (0) or a negative error code and sigax_last_error() gives the text.
 *
 * All compute runs in hand-written HIP kernels for gfx950.  There is no CPU fallback: if no GPU is
 * visible the calls fail with SIGAX_E_DEVICE.
 */
#ifndef SIGAX_H_
#define SIGAX_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SIGAX_OK           0
#define SIGAX_E_ARG       -1  /* bad argument */
#define SIGAX_E_IO        -2  /* file missing / malformed (.bwt magic, .sai header) */
#define SIGAX_E_DEVICE    -3  /* HIP error (no device, out of memory, launch failure) */
#define SIGAX_E_CAPACITY  -4  /* a device arena overflowed and could not be grown */
#define SIGAX_E_SUBSTRING -5  /* reserved */
#define SIGAX_E_STATE     -6  /* call order (e.g. edges requested before read metadata was set) */

/* flags of the overlap calls: OverlapBuilder ctor arguments (src/overlap_builder.h:21-24) */
#define SIGAX_IRREDUCIBLE  1u  /* irreducible=true  (CLI: absence of -x/--exhaustive, src/overlap.cpp:43) */
#define SIGAX_RC           2u  /* rc=true           (CLI: absence of --no-opposite-strand) */
#define SIGAX_EDGES        4u  /* also materialise edge records (Hit2OverlapConverter, src/overlap_builder.cpp:345-375) */
#define SIGAX_DUPLICATE    8u  /* OverlapBuilder::duplicate instead of overlap (src/overlap_builder.cpp:1184-1195): only the
                                  seq/fmi and complement(seq)/rfmi finds, minOverlap = read length, blocks = the containment
                                  blocks; min_overlap and the other mode flags are ignored.  Used by `siga rmdup`. */

typedef struct sigax_index sigax_index; /* both FM-indexes + both .sai tables, resident on one GPU */
typedef struct sigax_batch sigax_batch; /* device workspace for batches of reads */

/* One OverlapBlock in the order it is serialised to the hits text (src/overlap_builder.cpp:138-141,198-201):
 * capped pair, raw pair, length, AlignFlags (bit0 QUERYREV, bit1 TARGETREV, bit2 QUERYCOMP; :42-44). */
typedef struct sigax_block {
  uint64_t capped0_lo, capped0_hi, capped1_lo, capped1_hi;
  uint64_t raw0_lo, raw0_hi, raw1_lo, raw1_hi;
  uint32_t length;
  uint32_t af;
  uint64_t reserved;  /* pads the record to 80 bytes = 5 x 16 so device vector accesses stay aligned */
} sigax_block;

/* One kept overlap of Hit2OverlapConverter::convert (src/overlap_builder.cpp:345-375): read indices are
 * positions in the indexed read set; coordinates follow from (length, af, read lengths) exactly as
 * OverlapBlock::overlap computes them (src/overlap_builder.cpp:158-175). */
typedef struct sigax_edge {
  uint32_t query, target;
  uint32_t length;
  uint32_t af;
} sigax_edge;

typedef struct sigax_stats {
  uint64_t n_reads;
  uint64_t n_candidate_blocks; /* blocks pushed by OverlapBlockFinder::find, containments included */
  uint64_t n_blocks;           /* blocks returned */
  uint64_t n_edges;
  uint64_t n_occ_find;         /* Occ(i) evaluations made by the block finder (N_occ_min share) */
  uint64_t n_occ_extract;      /* ... by sub-maximal filter + irreducible extraction */
  uint64_t n_substring;        /* reads flagged substring (SS:i:1) */
  uint64_t n_slow_reads;       /* reads that needed the general (serial) filter/extract kernel */
  uint64_t n_extract_errors;   /* reads where extract() hit "substring read found" (src/overlap_builder.cpp:754-757) */
  uint64_t n_sectors_find;     /* distinct 64-byte sectors of the rank tables the finder's formulation touches: per step one
                                  or two granules (one-step) or both halves of one or two 128-byte lines (two-step table) */
  uint64_t n_sectors_extract;  /* the same for sub-maximal filter + irreducible extraction, per round and block */
} sigax_stats;

typedef struct sigax_result {
  uint32_t     n_reads;
  uint64_t*    block_offs;  /* n_reads+1; blocks of read r are blocks[block_offs[r] .. block_offs[r+1]) in the
                               reference's list order */
  sigax_block* blocks;
  uint8_t*     substring;   /* n_reads; OverlapResult::substring (src/overlap_builder.cpp:211-216) */
  uint64_t     n_edges;
  sigax_edge*  edges;       /* only with SIGAX_EDGES; in hits order = the ED order of the reference at -t 1 */
  sigax_stats  stats;
} sigax_result;

typedef struct sigax_index_info {
  uint64_t n_symbols;   /* BWT length (= sum(len+1)) per strand */
  uint64_t n_strings;   /* reads */
  uint64_t device_bytes;
  uint64_t pred[5];     /* C[] of the forward index: FMIndex::getPC (src/fmindex.h:129-131) */
  int      device;
  int      wide;        /* 1 if positions need 64 bits */
} sigax_index_info;

const char* sigax_last_error(void);           /* thread-local text of the last failure */
int  sigax_device_count(int* n);
/* A HIP stream (non-blocking) for callers that do not link HIP themselves, e.g. to keep two batch objects in flight
 * (sigax_batch_run).  The handle is a hipStream_t and may be passed wherever this header takes a `stream`. */
int  sigax_stream_create(int device, void** stream);
void sigax_stream_destroy(int device, void* stream);

/* FMIndex::load x2 + SuffixArray::load x2 (src/overlap.cpp:41-42, src/overlap_builder.cpp:466).  The .sai
 * paths may be NULL when SIGAX_EDGES is never requested.  rbwt_path NULL or "": the forward strand alone -- what
 * `siga index --no-reverse` writes and `siga correct` loads (src/correct.cpp:41-47) -- serving sigax_occ_batch (which = 0),
 * sigax_kmer_count_batch and sigax_correct_*; overlap runs on such an index fail with SIGAX_E_STATE.  With sai_path given
 * beside it, the forward .sai table is loaded too: what sigax_locate_* needs (rsai_path is not read). */
int  sigax_index_open(const char* bwt_path, const char* rbwt_path, const char* sai_path, const char* rsai_path,
                      int device, sigax_index** out);
/* Same from memory: RL units exactly as in the .bwt payload (src/rlstring.h:10-63), read ids of the .sai lines
 * (rruns NULL with n_rruns 0: forward strand only). */
int  sigax_index_open_mem(const uint8_t* runs, uint64_t n_runs, const uint8_t* rruns, uint64_t n_rruns,
                          uint64_t n_symbols, uint64_t n_strings, const uint32_t* sai, const uint32_t* rsai,
                          int device, sigax_index** out);
/* A replica of an open index (tables, .sai rows, read metadata set so far) on another GPU of the node, copied device to
 * device -- over xGMI between peers -- instead of being read, decoded and uploaded again. */
int  sigax_index_clone(const sigax_index* src, int device, sigax_index** out);
void sigax_index_close(sigax_index*);
int  sigax_index_info_get(const sigax_index*, sigax_index_info* out);
/* Per-read metadata Hit2OverlapConverter keeps (ReadInfo{name,length}, src/overlap_builder.cpp:333-343).
 * name_rank[i] = rank of read i's name among all names under std::string operator< (equal names, equal rank):
 * the dedup rule of src/overlap_builder.cpp:358,365 needs only equality and order of names. */
int  sigax_index_set_reads(sigax_index*, const uint32_t* lengths, const uint32_t* name_rank, uint64_t n);

/* `siga index` for one strand on the GPU: SuffixArrayBuilder "sais2" + BWT(sa, reads) + the .sai rows
 * (src/indexer.cpp:80-104, src/suffix_array_builder.cpp:472-674, src/bwt.cpp:7-32, src/suffix_array.cpp:17-44).
 * seqs/offs as in sigax_overlap_batch; reverse != 0 indexes the reversed reads (src/indexer.cpp:60-64: the .rbwt/.rsai
 * pair).  On success *runs holds *n_runs RL units exactly as the .bwt payload stores them (31-cap of src/bwt.cpp:17),
 * *sai the n_reads read ids of the full-read suffixes in suffix order, *n_symbols = sum(len + 1).  Both arrays are
 * malloc'd; release with sigax_free.  SIGAX_E_CAPACITY = input too repetitive for the device sort (the host falls
 * back to its own SA-IS). */
int  sigax_build_strand(const char* seqs, const uint64_t* offs, uint64_t n_reads, int reverse, int device,
                        uint8_t** runs, uint64_t* n_runs, uint32_t** sai, uint64_t* n_symbols);
void sigax_free(void* p);
/* Brackets several builds (the two strands of one `siga index`): between open (1) and close (0) the builders' device
 * workspace is kept and handed from one call to the next instead of going back to the driver -- hipMalloc hands out
 * cleared memory, and clearing the tens of GB a strand's sort works in again for the next strand cost more than its
 * kernels.  Optional; nests; without it every call returns its workspace when it ends. */
void sigax_build_session(int open);

/* The index is here to stay (a service, a benchmark: many more reads than it holds will be asked of it): builds the
 * extractor's row tables now and returns when they are in place.  Without this call they are built in the background once
 * the index has been asked for as many reads as it holds -- one pass of `siga overlap` over the indexed reads
 * (src/overlap.cpp:41-47) never pays their build.  No-op when they are there already or do not fit. */
int  sigax_index_prepare(sigax_index*);
/* The same for an index that will serve overlap runs with this minimum overlap (the CLI's -m, src/overlap.cpp:44): besides
 * the row tables, the block finder's DEEP START TABLE for K = min(min_overlap, 56) -- every distinct K-mer of the indexed
 * reads with the state OverlapBlockFinder::find (src/overlap_builder.cpp:846-871) holds after consuming it, so that a
 * chain starts where its output starts (nothing is pushed below minOverlap, :861) instead of walking there.  Serves every
 * later run whose min_overlap is at least that K; runs with a smaller one, and chains whose K-mer is not in the reads,
 * walk as before -- same bytes out.  Without this call the table is built in the background, for the min_overlap of the
 * run at hand, once the index has been asked for as many reads as it holds.  No-op when it does not fit the free memory
 * (32 bytes x 2 per distinct K-mer and strand) or min_overlap < 16. */
int  sigax_index_prepare_overlap(sigax_index*, uint32_t min_overlap);

/* Self-check of an open index: are the BWT rows of strand `which` (0 forward, 1 reverse) in the suffix order `siga index`
 * produces (SuffixArrayBuilder "sais2": src/suffix_array_builder.cpp:472-674; SURVEY.md App. C: one '$' smaller than
 * ACGT, comparisons continuing past it, end of text smallest)?  Every pair of adjacent rows is compared on the device.
 * *n_bad = pairs out of order (0 = the index is in order), *first_bad = the first such row, *n_undecided = pairs still
 * tied after 4096 reads' worth of symbols.  Needs the .sai tables and sigax_index_set_reads(); SIGAX_E_STATE when the index
 * holds non-ACGT bases or has no row tables. */
int  sigax_index_check_order(sigax_index*, int which, uint64_t* n_bad, uint64_t* first_bad, uint64_t* n_undecided);

/* FMIndex::getOcc(i) for many positions (src/fmindex.cpp:320-323): which = 0 forward, 1 reverse index;
 * counts5[5*k..] = Occ($,A,C,G,T) inclusive of positions[k]; position 2^64-1 gives zeros. Host buffers. */
int  sigax_occ_batch(sigax_index*, int which, const uint64_t* positions, uint64_t n, uint64_t* counts5);
/* FMIndex::Interval::occurrences (src/fmindex.h:80-86) for n k-mers of length k on the forward index. */
int  sigax_kmer_count_batch(sigax_index*, const char* kmers, uint32_t k, uint64_t n, uint64_t* counts);

/* KmerCorrector::process for a batch of reads (src/correct_processor.cpp:72-229, `siga correct -a kmer`).  quals may be
 * NULL (FASTA input: every base scores 15).  out_seqs has the layout of seqs and receives the corrected sequence of
 * reads that became all-solid and the unchanged sequence otherwise; valid[r] = CorrectResult::validQC (only those
 * reads are written by PostCorrector, :242-265).  Parameters as the CLI's -k/-x/-i/-O (defaults 31/3/10/1,
 * src/correct_processor.h:15-20).  Forward index only, as the reference.
 * A negative kmer_threshold means what it means in the reference, whose CorrectThreshold keeps the two supports as ints and
 * hands them out as size_t (src/correct_processor.cpp:29-37): a negative support is one no count reaches.  With -1 a
 * window or base whose phred is below 20 (every one of a FASTA read) is never solid and never corrected, while one at 20 and
 * above needs support 0; with -2 and below nothing is solid, so no read with at least kmer_size bases is valid.
 * k-mer counts are kept in 32 bits and saturate at 2^32 - 2; 2^32 - 1 stands for "out of reach", also as count_offset. */
int  sigax_correct_batch(sigax_index*, const char* seqs, const char* quals, const uint64_t* offs, uint32_t n_reads,
                         uint32_t kmer_size, int32_t kmer_threshold, uint32_t kmer_rounds, uint32_t count_offset,
                         char* out_seqs, uint8_t* valid);

/* The same with every buffer in device memory, asynchronous on `stream` (a hipStream_t or NULL): d_offs u64[n_reads+1],
 * d_quals may be NULL, d_stat4 = 4 u64 of device scratch that receive {reads longer than the kernel supports (their
 * valid[] is 2), rank-table sectors asked for, k-mer lookups made, reserved}.  What a batching runtime and bench.py use.
 * The first correction call on an index allocates the table of all 13-mer intervals (537 MB, 1 GB with 64-bit positions:
 * the one synchronous step; sigax_batch_size_hint leaves room for it) and builds it on `stream`, ahead of the call's own
 * kernel; calls on other streams wait for that build through an event. */
int  sigax_correct_device(sigax_index*, const void* d_seqs, const void* d_quals, const void* d_offs, uint64_t n_reads,
                          uint32_t kmer_size, int32_t kmer_threshold, uint32_t kmer_rounds, uint32_t count_offset,
                          void* d_out_seqs, void* d_valid, void* d_stat4, void* stream);

/* `siga match` for a batch (src/match.cpp:54-62): how often each read occurs in the indexed set, count(w) = occ(w) +
 * occ(revcomp(w)) with occ = FMIndex::Interval::occurrences (src/fmindex.h:80-86) on the forward index; the second term only
 * with SIGAX_RC (CLI: absence of --no-opposite-strand), so a reverse-palindromic w counts twice, as in the reference.  A read of
 * more than max_length bases is split: counts[2r] = count(its first max_length bases), the number of its `VT 0` line, and
 * counts[2r+1] = count(its last max_length bases), the number of its `VT 1` line; any other read has counts[2r] = count(read)
 * and counts[2r+1] = SIGAX_MATCH_NONE.  max_length = UINT64_MAX: never split; 0: every non-empty read is split into two empty
 * patterns, which occur 0 times.  Bytes outside ACGT rank as '$', in w and in its complement.  Reads of any length below 2^32.
 * flags: SIGAX_RC or 0, anything else is SIGAX_E_ARG.  Exact 64-bit counts.  Works on an index opened without the reverse
 * strand; n_reads = 0 is SIGAX_OK. */
#define SIGAX_MATCH_NONE (~0ull)
int  sigax_match_batch(sigax_index*, const char* seqs, const uint64_t* offs, uint64_t n_reads, uint64_t max_length,
                       uint32_t flags, uint64_t* counts);
/* The same with every buffer in device memory, asynchronous on `stream` (a hipStream_t or NULL); allocates nothing.  d_offs
 * u64[n_reads+1], d_counts u64[2 n_reads], d_stat4 = 4 u64 of device scratch that receive {chains run (non-empty patterns
 * searched), symbols consumed (counted no further than where the reference's loop stops), rank-table sectors asked for,
 * reserved (the kernel's work counter)}.  Uses the two-step tables and, when a correction call has left it on the device, the
 * table of 13-mer intervals; allocates neither.  Counts do not depend on which tables exist. */
int  sigax_match_device(sigax_index*, const void* d_seqs, const void* d_offs, uint64_t n_reads, uint64_t max_length,
                        uint32_t flags, void* d_counts, void* d_stat4, void* stream);

/* A stream of batches through sigax_match_device, for a caller that does not link HIP (`siga match`): `slots` sets of device
 * buffers, pinned host buffers and streams, sized once -- max_reads / max_bases per batch, 0 = from the device's free memory.
 * submit copies batch `slot`'s reads up, runs the kernel and copies the counts down, all asynchronous on the slot's stream,
 * so that one slot's copies run beside another's kernel; offs are the n_reads + 1 offsets of the batch's reads in `seqs`
 * (offs[0] need not be 0: a window of a longer table).  wait returns the slot's counts[2 n_reads], valid until its next
 * submit, and unless NULL its stat4 (sigax_match_device).  SIGAX_E_CAPACITY: the batch does not fit the slot. */
typedef struct sigax_matcher sigax_matcher;
int  sigax_matcher_create(sigax_index*, uint32_t slots, uint64_t max_reads, uint64_t max_bases, sigax_matcher** out);
void sigax_matcher_destroy(sigax_matcher*);
int  sigax_matcher_capacity(const sigax_matcher*, uint64_t* max_reads, uint64_t* max_bases);
int  sigax_matcher_submit(sigax_matcher*, uint32_t slot, const char* seqs, const uint64_t* offs, uint64_t n_reads,
                          uint64_t max_length, uint32_t flags);
int  sigax_matcher_wait(sigax_matcher*, uint32_t slot, const uint64_t** counts, uint64_t stat4[4]);

/* ---- `siga preqc`: index rows back to text, and the k-mer count distribution (csrc/sigax_spectrum.hip) ---------------------
 * FMIndex::getString(i) (src/fmindex.cpp:292-313) for many rows of strand `which` (0 forward, 1 reverse: SIGAX_E_STATE on an
 * index opened without it): the walk backwards from BWT row i to the first symbol of rank 0, i.e. the text in front of that
 * row's suffix -- for a row below n_strings a whole read (on the reverse strand, reversed), or its last ACGT piece when it holds
 * other bytes.  Lengths are not known before the walk, hence two passes: the lengths pass, then -- after the caller's prefix
 * sum -- the write pass.  Every walk is bounded by max_len: one that would be longer stops there, keeps the max_len symbols
 * nearest its row, and is counted.  A row >= n_symbols gives length 0 and is counted.  The bytes do not depend on which of
 * the index's optional tables exist.
 *
 * sigax_string_lengths_device: d_rows u64[n] -> d_lens u32[n] and, unless NULL, d_stretch u64[n] = Occ('$') before the row
 * the walk ended at: the index of the string's stretch among all stretches in suffix order, what the .sai table is indexed by
 * (for ACGT-only read sets sai[that] is the read's id); SIGAX_NO_STRETCH for a walk that was cut or never started.
 * d_status2 = 2 u64, written (not added to): {rows out of range, walks cut at max_len}.
 * sigax_get_strings_device: string i's bytes, in text order, to d_seqs[d_offs[i] .. d_offs[i+1]) (d_offs u64[n+1]); a row
 * whose slot is not its length is not written and counted in d_status3[2] (d_status3[0..1] as above).
 * Both are asynchronous on `stream` (a hipStream_t or NULL) and allocate nothing. */
#define SIGAX_NO_STRETCH (~0ull)
int  sigax_string_lengths_device(sigax_index*, int which, const void* d_rows, uint64_t n, uint32_t max_len, void* d_lens,
                                 void* d_stretch, void* d_status2, void* stream);
int  sigax_get_strings_device(sigax_index*, int which, const void* d_rows, uint64_t n, uint32_t max_len, const void* d_offs,
                              void* d_seqs, void* d_status3, void* stream);
/* Host buffers, synchronous: *seqs (the strings back to back, one '\0' after the last) and *offs (u64[n+1]) are malloc'd,
 * release with sigax_free; stretch = NULL or u64[n] of the caller's. */
int  sigax_get_strings(sigax_index*, int which, const uint64_t* rows, uint64_t n, uint32_t max_len, char** seqs,
                       uint64_t** offs, uint64_t* stretch);

/* KmerDistribution::sample's loop (src/kmerdistr.cpp:12-33) for a batch of strings: a string of fewer than k bytes is skipped;
 * otherwise for j = k .. len-1: w = s[j-k, j), count = occ(w) + occ(revcomp(w)) on the forward index (both strands always, as
 * the reference; occ = FMIndex::Interval::occurrences), hist[min(count, n_bins-1)] += 1.  As in the reference j stops BEFORE
 * len: the window that ends at the string's last base is never counted and a string of exactly k bases contributes no window,
 * though its bases count in L = the sum of the lengths of the strings with len >= k.  Bytes outside ACGT rank as '$', in w and in
 * its complement (as sigax_match_*).  Exact 64-bit counts; the bins are u64 and are ADDED to, so a caller accumulates over batches
 * (and zeroes them first).  stat4, written: {strings with len >= k, L, windows counted, rank-table sectors asked for}.
 * k = 0 or n_bins = 0: SIGAX_E_ARG; n_reads = 0: SIGAX_OK.  Works on an index opened without the reverse strand.  Uses the
 * two-step tables and, when a correction call has left it on the device, the table of 13-mer intervals; allocates neither.
 * The device form is asynchronous on `stream` and allocates nothing: d_work = sigax_kmer_spectrum_workspace bytes of scratch. */
int  sigax_kmer_spectrum_workspace(uint64_t n_reads, uint64_t* bytes);
int  sigax_kmer_spectrum_device(sigax_index*, const void* d_seqs, const void* d_offs, uint64_t n_reads, uint32_t k, uint64_t n_bins,
                                void* d_hist, void* d_stat4, void* d_work, uint64_t work_bytes, void* stream);
/* host strings (seqs/offs as in sigax_match_batch), host bins; stat4 may be NULL */
int  sigax_kmer_spectrum_batch(sigax_index*, const char* seqs, const uint64_t* offs, uint64_t n_reads, uint32_t k, uint64_t n_bins,
                               uint64_t* hist, uint64_t stat4[4]);
/* rows of the forward strand -> their strings (walks bounded by max_len) -> spectrum; the strings never leave the device */
int  sigax_kmer_spectrum_rows(sigax_index*, const uint64_t* rows, uint64_t n, uint32_t k, uint32_t max_len, uint64_t n_bins,
                              uint64_t* hist, uint64_t stat4[4]);
/* rows of strings of up to max_len bytes one sigax_kmer_spectrum_rows call can take with the device's free memory now */
int  sigax_kmer_spectrum_rows_hint(sigax_index*, uint32_t max_len, uint64_t n_bins, uint64_t* max_rows);

/* ---- `siga locate`: where every query occurs (csrc/sigax_locate.hip) ----------------------------------------------------------
 * The other half of the FM-index: an occurrence of w is a row p of w's suffix-array interval; the number of LF steps from p back
 * to the first symbol of rank 0 is the occurrence's offset in its read, and sai[Occ('$') before that row] is the read.  Nothing
 * is stored for it beyond the forward strand and its .sai table.  No counterpart in the reference.
 *
 * Needs an index opened with the forward .sai table (also one opened without the reverse strand: sigax_index_open with
 * rbwt_path NULL and sai_path given) whose reads hold ACGT only -- the check of sigax_index_check_order, C['A'] == n_strings:
 * with other bytes a stretch is a piece of a read, and locating would need a table from stretch to (read, piece offset), which
 * the index does not carry.  SIGAX_E_STATE otherwise.
 *
 * Queries as in sigax_match_batch (seqs, offs u64[n_queries + 1], each below 2^32 bytes).  totals[q] = what sigax_match_batch
 * returns as counts[2q] with max_length = UINT64_MAX and the same flags, for every query: bytes outside ACGT rank as '$', an
 * empty query gives 0, a reverse-palindromic one counts twice with SIGAX_RC.  Hits are LISTED for query q iff it is non-empty,
 * all ACGT and totals[q] <= max_hits; otherwise qflags[q] says why not and hit_offs[q+1] == hit_offs[q].  hits[hit_offs[q] ..
 * hit_offs[q+1]) holds the rows of the query's interval in ascending row order, then -- with SIGAX_RC -- the rows of its reverse
 * complement's interval in ascending row order, flagged SIGAX_HIT_REV.  The order depends on the index's bytes alone, not on
 * which of its optional tables exist.  A walk of more than max_len steps, or one that leaves the table (a damaged index), is
 * cut: flagged SIGAX_HIT_CUT, read = offset = 0xFFFFFFFF, and counted.  max_hits is 32 bits: a query lists fewer than 2^32 hits.
 *
 * sigax_locate_device: every buffer in device memory, asynchronous on `stream` (a hipStream_t or NULL), allocates nothing.
 * d_offs u64[n+1], d_totals u64[n], d_qflags u32[n], d_hit_offs u64[n+1], d_hits sigax_hit[hits_cap] (16-byte aligned), d_rows
 * NULL or u64[hits_cap]: the BWT row of each hit, in the same places.  d_status4 = 4 u64, written (not added to): {hits listed =
 * hit_offs[n], walks cut at max_len, rank-table sectors asked for, reserved}.  d_work = sigax_locate_workspace(n) bytes of
 * scratch, 16-byte aligned.  When the hits listed exceed hits_cap, d_totals, d_qflags, d_hit_offs and status[0] are still
 * complete, no hit and no row is written and nothing outside the buffers is touched: a caller reads status[0], sizes its
 * buffers and calls again.  hits_cap may be any value the buffers hold, UINT64_MAX for "room enough" included: the call walks
 * min(hits_cap, n_queries * max_hits) slots, and SIGAX_E_ARG if that is above (2^31 - 1) * 256 or n_queries above 2^32 - 1 (a
 * hit names its query in 32 bits).  flags other than SIGAX_RC or 0 and a NULL where a buffer is required: SIGAX_E_ARG;
 * n_queries = 0: SIGAX_OK.  Uses the two-step tables and, when a correction call has left it on the device, the table of
 * 13-mer intervals; allocates neither. */
typedef struct sigax_hit { uint32_t query, read, offset, flags; } sigax_hit;  /* 16 bytes */
#define SIGAX_HIT_REV       1u   /* read[offset, offset+len) == revcomp(query) */
#define SIGAX_HIT_CUT       2u   /* walk stopped at max_len: read = offset = 0xFFFFFFFF */
/* per-query flags */
#define SIGAX_LOCATE_SKIPPED  1u /* query empty or holds a byte outside ACGT: no hits listed */
#define SIGAX_LOCATE_OVER     2u /* total > max_hits: no hits listed */
int  sigax_locate_workspace(uint64_t n_queries, uint64_t* bytes);  /* host arithmetic only */
int  sigax_locate_device(sigax_index*, const void* d_seqs, const void* d_offs, uint64_t n_queries, uint32_t flags,
                         uint32_t max_hits, uint32_t max_len, void* d_totals, void* d_qflags, void* d_hit_offs, void* d_hits,
                         void* d_rows, uint64_t hits_cap, void* d_status4, void* d_work, uint64_t work_bytes, void* stream);
/* Host buffers, synchronous: searches and scans, reads the number of hits listed, allocates exactly that many and walks.
 * *totals u64[n], *qflags u32[n], *hit_offs u64[n+1] and *hits sigax_hit[(*hit_offs)[n]] are malloc'd; release with sigax_free.
 * offs[0] need not be 0 (a window of a longer table).  Runs on a stream of its own: calls from several host threads overlap. */
int  sigax_locate_batch(sigax_index*, const char* seqs, const uint64_t* offs, uint64_t n_queries, uint32_t flags,
                        uint32_t max_hits, uint32_t max_len, uint64_t** totals, uint32_t** qflags, uint64_t** hit_offs,
                        sigax_hit** hits);

/* ---- `siga correct -a overlap`: pile-up correction of reads (csrc/sigax_pileup.hip) -------------------------------------------
 * A read is lined up, without gaps, against the indexed reads that share a seed with it, and every column is put to the vote.
 * The reference declares the algorithm and leaves it empty (OverlapCorrector::process, src/correct_processor.cpp:231-240); the
 * rules are these.  Integer arithmetic throughout; no result depends on the order of hits, candidates or reads.
 *
 * Parameters (sigax_pile_params; CLI spelling and default in brackets), anything outside the range is SIGAX_E_ARG with the
 * field named in sigax_last_error():
 *   S seed_length 12..64 (--seed-length 24)    T seed_stride 1..S (--seed-stride 12)      H max_seed_hits 1..4096 (--max-seed-hits 256)
 *   M min_overlap >= 1 (-m 45)                 P error_permille 0..250 (-e 40)            C conflict >= 1 (--conflict 5)
 *   D min_depth >= 1 (--min-depth 2)           K max_candidates 1..4096 (--max-candidates 512)
 *   max_read_len 1..SIGAX_PILE_MAX_LEN, 0 = SIGAX_PILE_MAX_LEN: the columns a wave's LDS is sized for (the host form sets it
 *   from the batch's longest read); a longer read is "too long" below.
 *
 * The reference set is the reads of the index by read id, ref[t], ACGT only (locate's condition), each shorter than 2^30
 * bases.  The query q is a read of n bytes.
 *  1. n < S: unchanged, valid = 0.  n > max_read_len: unchanged, valid = 2 (as sigax_correct_device for reads it cannot take).
 *  2. Seeds: the windows q[p, p+S) for p = 0, T, 2T, ... while p + S <= n, and p = n - S if it is not among them.  A seed with a
 *     byte outside ACGT is skipped; every other seed is located on both strands (sigax_locate_device with SIGAX_RC); one whose
 *     total exceeds H is skipped as a repeat.
 *  3. Candidates: a forward hit (t, o) of the seed at p gives (t, +, d = o - p); a reverse hit (t, o) gives (t, -, d = len(t) -
 *     o - S - p), read against revcomp(ref[t]).  The candidates are the DISTINCT triples (t, strand, d): one triple found through
 *     several seeds counts once, one read at two diagonals twice.  The query gets no vote of its own; if it is in the index it
 *     is a candidate like any read.  More than K distinct triples: unchanged, valid = 0, counted in status[2].
 *  4. Acceptance: column x of q faces position x + d of the candidate's text; the overlap is the x for which both exist, l its
 *     length, m its mismatches (a query byte outside ACGT is one).  Accepted iff l >= M and m <= floor(l * P / 1000).
 *  5. Votes: cnt[x][A,C,G,T] over the accepted candidates that cover x.
 *  6. Change: b = q[x], cnt[x][b] = 0 for a byte outside ACGT, c = the base of the unique largest count at x.  q'[x] = c iff
 *     c != b and cnt[x][c] >= C and cnt[x][b] < C; a tie for the largest count changes nothing.  All columns from the same pile.
 *  7. Validity: valid = 1 iff cnt[x][q'[x]] >= D for every x.  The output is q' for a valid read, q otherwise; changed = 1 iff
 *     the output differs from q.
 *  8. Rounds (host form): a further round runs 2-7 on the output; only reads that changed in the round before take part; the
 *     loop ends when none did or after `rounds`.  The pile always comes from the index as it is.  valid comes from the last
 *     round a read took part in, changed says whether any round changed it.
 *
 * Reference text.  sigax_reference_text_device builds ref[] on the device from the index alone, one BYTE per base (ASCII, read
 * t at d_text[d_text_offs[t] .. d_text_offs[t+1])): rows 0 .. n_strings - 1 through the row walk of sigax_string_lengths_device
 * / sigax_get_strings_device, filed under the read id sai[stretch].  Needs what locate needs (forward .sai, ACGT only),
 * SIGAX_E_STATE otherwise.  *text_bytes of the workspace call = n_symbols - n_strings, exactly the bases; d_text_offs
 * u64[n_strings + 1]; d_status4, written: {reads, bases, rows that gave no read (walk cut at 2^30 - 1 bases, stretch without a
 * read id), slots of the wrong size}; the last two are 0 on an index that is in order.  Asynchronous, allocates nothing.
 *
 * sigax_pileup_device: one round, every buffer in device memory, asynchronous on `stream`, allocates nothing.  d_offs
 * u64[n_reads + 1] (n_reads < 2^31), n_bases >= d_offs[n_reads] - d_offs[0] (it sizes the seed table), d_out_seqs in the layout
 * of d_seqs and not overlapping it, d_valid and d_changed u8[n_reads], d_work = sigax_pileup_workspace(n_reads, n_bases,
 * params, hits_cap) bytes, 16-byte aligned; the seeds' hits live in it.  Seeds go through sigax_locate_device.  d_status8,
 * written (not added to): {hits listed, reads too long, reads over K, seeds located, seeds skipped as repeats, candidates tested,
 * candidates accepted, bases changed}.  When the hits listed exceed hits_cap, no read, no valid[] and no changed[] is written,
 * status[0] carries the number and status[1..7] are 0: the caller sizes its workspace from it and calls again.
 *
 * sigax_pile_ref: the reference text of an index, built once (synchronous) and kept on the device until it is destroyed.
 * sigax_pileup_batch: host buffers, synchronous; loops the rounds (rule 8), sizes hits_cap itself and splits a batch that does
 * not fit the device's free memory.  out_seqs has the layout of seqs (offs[0] need not be 0), valid and changed u8[n_reads],
 * status8 (may be NULL) = the rounds' status words added up, *rounds_run (may be NULL) = the rounds that ran. */
#define SIGAX_PILE_MAX_LEN 4096u
typedef struct sigax_pile_params {
  uint32_t seed_length, seed_stride, max_seed_hits, min_overlap, error_permille, conflict, min_depth, max_candidates;
  uint32_t max_read_len, reserved;  /* reserved = 0 */
} sigax_pile_params;
int  sigax_reference_text_workspace(sigax_index*, uint64_t* text_bytes, uint64_t* work_bytes);  /* host arithmetic only */
int  sigax_reference_text_device(sigax_index*, void* d_text, uint64_t text_bytes, void* d_text_offs, void* d_status4, void* d_work,
                                 uint64_t work_bytes, void* stream);
int  sigax_pileup_workspace(uint64_t n_reads, uint64_t n_bases, const sigax_pile_params*, uint64_t hits_cap, uint64_t* bytes);
int  sigax_pileup_device(sigax_index*, const void* d_seqs, const void* d_offs, uint64_t n_reads, uint64_t n_bases,
                         const sigax_pile_params*, const void* d_ref_text, const void* d_ref_offs, void* d_out_seqs, void* d_valid,
                         void* d_changed, void* d_status8, void* d_work, uint64_t work_bytes, uint64_t hits_cap, void* stream);
typedef struct sigax_pile_ref sigax_pile_ref;
int  sigax_pile_ref_create(sigax_index*, sigax_pile_ref** out);
void sigax_pile_ref_destroy(sigax_pile_ref*);
/* the device buffers of the text (for sigax_pileup_device) and its bytes; any of the three may be NULL */
int  sigax_pile_ref_buffers(const sigax_pile_ref*, const void** d_text, const void** d_text_offs, uint64_t* text_bytes);
int  sigax_pileup_batch(sigax_index*, const sigax_pile_ref*, const char* seqs, const uint64_t* offs, uint64_t n_reads,
                        const sigax_pile_params*, uint32_t rounds, char* out_seqs, uint8_t* valid, uint8_t* changed,
                        uint64_t status8[8], uint32_t* rounds_run);

/* ---- `siga overlap -e`: overlaps with mismatches, seed and verify (csrc/sigax_mmoverlap.hip) ------------------------------------
 * Every read of the index is lined up, without gaps, against the indexed reads that share a seed with it; an overlap of at least
 * M columns with at most P mismatches per mille is kept, a dovetail as an edge record with its mismatch count, a containment as
 * a flag.  The reference finds exact overlaps only (OverlapBlockFinder, src/overlap_builder.cpp:838-912), although Match::numDiff
 * is part of its format (src/coord.cpp:67); the rules are these.  Integer arithmetic throughout; no result depends on the order
 * of hits, candidates, reads or batches.
 *
 * The read set is the reads of the index by id, ref[t]: ACGT only with the forward .sai loaded (locate's condition), and
 * sigax_index_set_reads called (lengths, name ranks); SIGAX_E_STATE otherwise.  A query is itself a read of the index, q = ref[i],
 * n = len(q).
 *
 * Parameters (sigax_mmo_params; CLI spelling and default in brackets), range errors as in sigax_pile_params:
 *   S seed_length 12..64 (--seed-length 24)    T seed_stride 1..S (--seed-stride 12)      H max_seed_hits 1..4096 (--max-seed-hits 256)
 *   M min_overlap >= 1 (-m 45)                 P error_permille 0..250 (-e, no default: its presence selects this path)
 *   K max_candidates 1..4096 (--max-candidates 512)                                       max_read_len 1..4096, 0 = 4096
 *
 *  1. n < S or n > max_read_len: the read emits nothing from its side, and status[1] counts it.
 *  2. Seeds and candidates are exactly rules 2-3 of the pile-up block: the windows q[p, p+S) for p = 0, T, 2T, ... and n - S, each
 *     located on both strands, one with more than H occurrences skipped; the candidates are the distinct triples (t, strand, d), a
 *     forward hit (t, o) giving d = o - p, a reverse hit d = len(t) - o - S - p, read against revcomp(ref[t]).  More than K distinct
 *     triples: the read emits nothing from its side and status[2] counts it.
 *  3. A candidate with name_rank[t] == name_rank[i] is skipped: the read itself and reads of the same name, as
 *     src/overlap_builder.cpp:358 does.  It counts towards K but is not "tested".
 *  4. Geometry: text = ref[t] or its reverse complement, L = len(text), x0 = max(0, -d), x1 = min(n, L - d), l = x1 - x0, m = the
 *     columns x in [x0, x1) with q[x] != text[x + d].  Accepted iff l >= M and m <= floor(l * P / 1000).
 *  5. Class of an accepted candidate: l == n == L DUP; else l == n Q_IN_T; else l == L T_IN_Q; else d < 0 SUFFIX (q's suffix on
 *     text's prefix, l = n + d); otherwise PREFIX (q's prefix on text's suffix, l = L - d).
 *  6. Containment flags, contained[], one byte per read of the index: Q_IN_T sets contained[i], T_IN_Q sets contained[t], DUP sets
 *     the flag of the read with the LARGER name rank (`rmdup` keeps the smaller name).  A flag is set from whichever side finds the
 *     alignment.  Containments give no record unless params.flags asks for them (rule 9).
 *  7. Dovetail records: sigax_mm_edge {query, target, length = l, af, num_diff = m, reserved = 0}; af has the meaning it has in
 *     sigax_edge, so the ED coordinates follow from (length, af, read lengths): SUFFIX + 0, SUFFIX - 6 (TARGETREV|QUERYCOMP),
 *     PREFIX + 3 (QUERYREV|TARGETREV), PREFIX - 5 (QUERYREV|QUERYCOMP).  Canonical form: the read with the larger name rank is
 *     `query` (the pair src/overlap_builder.cpp:365 keeps); when i has the smaller rank the record is written swapped, (t, i, l,
 *     af', m) with af' = af if af & 4, else af ^ 3.
 *  8. Both reads of a pair emit what their own seeds find.  The result is the SET of canonical records, each (query, target, af,
 *     length) once, ascending in (query, target, af, length) by read id: a pair is there if either side's seeds find it.  Where
 *     every accepted alignment holds a run of S + T - 1 matching columns -- min over l >= M of ceil((l - m) / (m + 1)) >= S + T - 1
 *     with m = floor(l P / 1000) -- and neither H is reached nor K on both sides, the set equals the one a search over every read,
 *     strand and diagonal gives.
 *
 *  9. flags = SIGAX_MMO_CONTAINMENTS: every accepted candidate of class Q_IN_T, T_IN_Q or DUP also gives one record in the same
 *     stream, counted by status[7] and subject to edges_cap like the others: query = the contained read (the one rule 6 flags),
 *     target = its container, length = len(contained), af = SIGAX_MM_CONTAINMENT | (4 if the contained read lies
 *     reverse-complemented in the container), num_diff = m, reserved = o, the first column of the container's FORWARD text that the
 *     contained read covers: Q_IN_T found from q = contained gives o = d forward and o = L - d - n reverse, T_IN_Q found from q =
 *     container gives o = -d on either strand, DUP gives 0; both sides of a pair thus give the same record.  Every set byte of
 *     contained[] then has at least one record.  flags = 0: no such record, every output as without this rule.  Other values:
 *     SIGAX_E_ARG.  Two containments of one pair on different diagonals are two records.
 *
 * sigax_mmoverlap_device: reads first_read .. first_read + n_reads of the index as queries, every buffer in device memory,
 * asynchronous on `stream`, allocates nothing.  d_ref_text / d_ref_offs: the reference text (sigax_reference_text_device,
 * sigax_pile_ref_buffers); n_bases >= d_ref_offs[first_read + n_reads] - d_ref_offs[first_read] (it sizes the seed table, as in
 * sigax_pileup_device); d_work = sigax_mmoverlap_workspace(n_reads, n_bases, params, hits_cap) bytes, 16-byte aligned; the seeds'
 * hits live in it.  The call APPENDS its raw canonical records to d_edges[edges_cap] at *d_cursor (u64, the records held so far)
 * and moves the cursor, and sets bytes to 1 in d_contained (u8 per read of the index, zeroed once by the caller).  d_status8,
 * written: {hits listed, reads too short or too long, reads over K, seeds located, seeds skipped as repeats, candidates tested
 * (rule 4 reached), candidates accepted, records emitted by this call}.  Hits over hits_cap: locate's protocol as
 * sigax_pileup_device passes it through -- status[0] carries the number, status[1..7] are 0, nothing is written.  Records over
 * edges_cap - *d_cursor: the cursor is left where it was, no record and no flag of this call is written, status[7] carries the
 * number needed and status[0..6] are as counted.  Raw records are in no particular order and a pair may be there twice.
 *
 * sigax_mmoverlap_finish_device: orders n_raw raw records (below 2^32) by (query, target, af, length, reserved), drops repeats,
 * leaves the result at the front of d_edges and its count in *d_n_unique (u64).  reserved is ordered in full width -- a
 * containment's offset is as wide as its container is long, and a read longer than max_read_len can be one -- and length by its
 * low 13 bits: an overlap of this path has at most 4096 columns.  Asynchronous, allocates nothing; d_work =
 * sigax_mmoverlap_finish_workspace(n_raw) bytes, 16-byte aligned.  Run it once over the records of all calls.
 *
 * sigax_mmoverlap_batch: synchronous; every read of the index in pieces, hits_cap and edges_cap sized from the status words, a
 * piece that does not fit half the free device memory halved, finish once.  *edges (malloc'd; release with sigax_free) holds
 * *n_edges records, contained u8[n_strings] is the caller's, status8 (may be NULL) = the pieces' status words added up.
 *
 * Not held: read sets beyond 2^32 bases are untested.  Out of scope: gapped overlaps (indels); transitive reduction or
 * irreducible output inside this path (`siga unitig -e --reduce` reduces these records on the graph side); more than one GPU;
 * quality values; seeds chosen by content. */
typedef struct sigax_mmo_params {
  uint32_t seed_length, seed_stride, max_seed_hits, min_overlap, error_permille, max_candidates;
  uint32_t max_read_len, flags;  /* flags: 0 or SIGAX_MMO_CONTAINMENTS */
} sigax_mmo_params;
#define SIGAX_MMO_CONTAINMENTS 1u  /* sigax_mmo_params.flags: containment records too (rule 9) */
#define SIGAX_MM_CONTAINMENT   8u  /* sigax_mm_edge.af of a containment record; bit 2 (4): reverse-complemented in the container */
typedef struct sigax_mm_edge { uint32_t query, target, length, af, num_diff, reserved; } sigax_mm_edge;  /* 24 bytes */
int  sigax_mmoverlap_workspace(uint64_t n_reads, uint64_t n_bases, const sigax_mmo_params*, uint64_t hits_cap, uint64_t* bytes);
int  sigax_mmoverlap_device(sigax_index*, const void* d_ref_text, const void* d_ref_offs, uint64_t first_read, uint64_t n_reads,
                            uint64_t n_bases, const sigax_mmo_params*, sigax_mm_edge* d_edges, uint64_t edges_cap, void* d_cursor,
                            void* d_contained, void* d_status8, void* d_work, uint64_t work_bytes, uint64_t hits_cap, void* stream);
int  sigax_mmoverlap_finish_workspace(uint64_t n_raw, uint64_t* bytes);
int  sigax_mmoverlap_finish_device(sigax_mm_edge* d_edges, uint64_t n_raw, void* d_n_unique, void* d_work, uint64_t work_bytes,
                                   void* stream);
int  sigax_mmoverlap_batch(sigax_index*, const sigax_pile_ref*, const sigax_mmo_params*, sigax_mm_edge** edges, uint64_t* n_edges,
                           uint8_t* contained, uint64_t status8[8]);

/* ---- `siga unitig`: unbranched chains of overlaps compacted (csrc/sigax_unitig.hip) ----------------------------------------------
 * The fixpoint of Bigraph::simplify (src/bigraph.cpp:341-414, Vertex::merge at :131-202) over the edge records of an overlap
 * run, without an index: every chain of reads joined by SIMPLE records becomes one unitig.
 *
 * Input: n_reads reads (lengths u32[n_reads], bases seqs / offs u64[n_reads + 1] by read id), n_edges sigax_edge records in
 * any order, each overlap once (what Hit2OverlapConverter leaves), and min_overlap.  A read has two ends, B (prefix, the
 * reference's ANTISENSE) and E (suffix, SENSE): a record touches `query` at E if af bit0 is clear, else at B, and `target` at B
 * if af bit1 is clear, else at E.  A record is IGNORED as malformed when a read id is >= n_reads, af is none of 0, 3, 5, 6,
 * length is 0 or above the shorter of its reads; otherwise ignored as low when length < min_overlap (Bigraph::load's filter).
 * A kept record is a containment when length equals the length of one of its reads, a self edge when query == target.  The
 * degree of a read end is the number of kept records that touch it, a containment counting at both ends of both its reads.  A
 * record is simple iff it is kept, no containment, no self edge and both ends it touches have degree 1 (:356-362).
 *
 * A unitig is a connected component of the reads under simple records: a path (a single read included) or a cycle.  A path
 * starts at its terminal with the smaller id and walks to the other; a read entered through B is placed forward, one entered
 * through E reverse-complemented (A<->T, C<->G, other bytes as they are); the first read is forward iff it is left through
 * E, a single read is forward.  offset[0] = 0, offset[i+1] = offset[i] + L[i] - overlap(i, i+1), the unitig has offset[last] +
 * L[last] bases: the first read whole, then of every next read the last L - overlap bases as placed.  A cycle starts at its
 * smallest id, placed forward and left through E, and walks until the next record would enter the start again: that record
 * is not merged, the unitig is flagged SIGAX_UNITIG_CIRCULAR and carries its overlap (the reference cuts such a cycle where
 * its hash map happens to begin: DESIGN.md 9d).  Unitigs are numbered by ascending id of their first read.
 *
 * Output, sized for the worst case so that one call is enough: seq_offs u64[n_reads + 1] and lay_offs u64[n_reads + 1], of
 * which entries 0 .. n_unitigs are written (unitig u has bases useqs[seq_offs[u] .. seq_offs[u+1]) and placements
 * layout[lay_offs[u] .. lay_offs[u+1])); uflags u32[n_reads], entries 0 .. n_unitigs - 1: bit0 SIGAX_UNITIG_CIRCULAR, the upper
 * 31 bits the closing overlap (uflags >> 1; overlaps are below 2^31); layout sigax_placement[n_reads], all written; useqs
 * offs[n_reads] - offs[0] bytes, of which seq_offs[n_unitigs] are written, or NULL for the layout alone.  status6 = 6 u64,
 * written (not added to): {unitigs, unitig bases, records ignored as malformed, records below min_overlap, simple records
 * merged (a cycle's closing record is not), cycles}.
 *
 * sigax_unitigs_device: every buffer in device memory, asynchronous on `stream` (a hipStream_t or NULL), allocates nothing.
 * d_edges, d_layout, d_useqs and d_work are 16-byte aligned, d_offs, d_seq_offs, d_lay_offs and d_status6 8-byte aligned;
 * d_work = sigax_unitigs_workspace bytes of scratch (some 190 bytes per read).  Whatever the records hold, nothing outside the buffers is touched, and every loop has a bound the host knows: list
 * ranking by pointer jumping runs ceil(log2 n_reads) + 1 rounds, twice.  n_reads >= 2^31, n_edges > 2^32, a NULL where a
 * buffer is required, a misaligned buffer and a work_bytes below sigax_unitigs_workspace's: SIGAX_E_ARG.  n_reads = 0:
 * SIGAX_OK, status zeros (when d_status6 is given).  Needs no index. */
typedef struct sigax_placement { uint32_t read, flags; uint64_t offset; } sigax_placement; /* 16 bytes */
#define SIGAX_PLACED_REV      1u   /* the read lies reverse-complemented in its unitig */
#define SIGAX_PLACED_CONTAINED 2u  /* a contained read placed by sigax_contained_place_*: no unitig call sets it */
#define SIGAX_UNITIG_CIRCULAR 1u   /* unitig flag, bit0; the closing overlap is uflags >> 1 */
int  sigax_unitigs_workspace(uint64_t n_reads, uint64_t n_edges, uint64_t* bytes);  /* host arithmetic only */
int  sigax_unitigs_device(int device, const sigax_edge* d_edges, uint64_t n_edges, const void* d_lengths, const void* d_seqs,
                          const void* d_offs, uint64_t n_reads, uint32_t min_overlap, void* d_seq_offs, void* d_lay_offs,
                          void* d_uflags, sigax_placement* d_layout, void* d_useqs, void* d_status6, void* d_work,
                          uint64_t work_bytes, void* stream);
/* Host buffers, synchronous.  offs[0] need not be 0.  *seq_offs u64[n_unitigs + 1], *lay_offs u64[n_unitigs + 1], *uflags
 * u32[n_unitigs], *layout sigax_placement[n_reads] and *useqs (unitig bases; pass useqs = NULL for the layout alone) are
 * malloc'd; release with sigax_free.  The six counts: sigax_unitigs_last_status. */
int  sigax_unitigs_host(int device, const sigax_edge* edges, uint64_t n_edges, const uint32_t* lengths, const char* seqs,
                        const uint64_t* offs, uint64_t n_reads, uint32_t min_overlap, uint64_t* n_unitigs, uint64_t** seq_offs,
                        uint64_t** lay_offs, uint32_t** uflags, sigax_placement** layout, char** useqs);
/* the six counts (status6 above) of this thread's last successful sigax_unitigs_host call, whose signature has no room for them */
int  sigax_unitigs_last_status(uint64_t status6[6]);

/* ---- `siga unitig -x`: tip trimming, and the graph between the unitigs (csrc/sigax_unitig.hip) ------------------------------------
 * What the reference's `assemble` does after its first simplify(): TrimVisitor (src/bigraph_visitors.cpp:1119-1161) and
 * simplify() in turn, --cut-terminal rounds (src/assembler.cpp:138-159), and the records that are left between the vertices
 * (PREFIX-graph.asqg.gz, :238).  Everything not said here is as in the block above: record classification, B/E ends, degrees,
 * simple records, rings, orientation, offsets, numbering.
 *
 * sigax_trim_opts: max_rounds (the reference's -x; at most 64), min_branch_length L (-n), min_branch_coverage C (-C;
 * 0xFFFFFFFF = no coverage test, the reference's default of -1), reserved = 0.
 *
 * Every read starts alive.  One round r = 1, 2, ...: a record is LIVE if it is kept and both its reads are alive; degrees,
 * simple records, links, the ring cut and the unitigs follow the rules above over the alive reads and the live records only.
 * A unitig's left end is the outward end of its first placed read (that read's B end if it is placed forward, its E end if
 * reversed), its right end the outward end of its last placed read; dL and dR are the degrees of those two read ends.  A
 * ring's two ends each carry its closing record, so a ring is never a dead end.  The unitig is removed in this round iff
 *   dL == 0 or dR == 0,  and  its bases <= L,  and, when C is given,  (K - 1) * max(L, 1) <= (max(C, 1) - 1) * bases
 * with K its number of reads, compared in u64.  The last is Point::avg(vertex) <= Point::avg(C, L) (:37-44) cross-multiplied;
 * it agrees with the reference's two double divisions whenever bases * L < 2^52 (two different quotients with denominators
 * bases and L differ by at least 1 / (bases * L), more than the rounding of either).  A removed unitig counts as an ISLAND if dL and dR are both 0,
 * else as a DEAD END.  Every decision of a round uses the state at its start; all reads of a removed unitig get removed[read]
 * = r.  A round that removes nothing ends the loop and is not counted.
 *
 * Result: the unitigs of the alive reads under the live records after the last round, in the shape of the sigax_unitigs_*
 * output, except: layout holds the alive reads only, lay_offs[n_unitigs] is their count (entries of layout beyond it are not
 * written); removed u32[n_reads] is 0 for a kept read, else the round in which it went.  max_rounds = 0 gives exactly the
 * sigax_unitigs_* result with removed all zero.
 *
 * Lifted records: after the last round every live record that was not merged (records at branched ends, containments, self
 * edges, a ring's closing record) becomes one sigax_edge over unitigs, in input record order.  Read end e (B = 0, E = 1) of a
 * read placed with flags & SIGAX_PLACED_REV = v is unitig end e ^ v.  query = the unitig of the record's query, target = that
 * of its target, length unchanged, af bit0 = the query's unitig end is B, bit1 = the target's unitig end is E, bit2 = bit0 ^
 * bit1.  A read in a live containment is a single forward unitig, so that record's af stays.  Coordinates follow from
 * (length, af, unitig lengths) as they do for reads.
 *
 * status12 = 12 u64, written: 0-5 the six counts above for the final graph, 6 rounds that removed something, 7 islands
 * removed, 8 dead ends removed, 9 reads removed, 10 kept records dropped because one of their reads was removed, 11 lifted
 * records written (0 without d_uedges).
 *
 * sigax_unitigs_trim_device: as sigax_unitigs_device -- asynchronous on `stream`, allocates nothing, never waits for the
 * device.  It enqueues max_rounds rounds; the launches of a round after one that removed nothing return at once on a device
 * counter.  d_removed u32[n_reads]; d_uedges NULL (no graph) or room for n_edges records, 16-byte aligned; d_status12 8-byte
 * aligned; d_work = sigax_unitigs_trim_workspace(n_reads, n_edges, d_uedges != NULL) bytes.  Refusals as above, and
 * max_rounds > 64 or reserved != 0: SIGAX_E_ARG.  Whatever the records hold, nothing outside the buffers is touched. */
typedef struct sigax_trim_opts { uint32_t max_rounds, min_branch_length, min_branch_coverage, reserved; } sigax_trim_opts;
#define SIGAX_TRIM_NO_COVERAGE 0xFFFFFFFFu
int  sigax_unitigs_trim_workspace(uint64_t n_reads, uint64_t n_edges, int want_graph, uint64_t* bytes);  /* host arithmetic only */
int  sigax_unitigs_trim_device(int device, const sigax_edge* d_edges, uint64_t n_edges, const void* d_lengths, const void* d_seqs,
                               const void* d_offs, uint64_t n_reads, uint32_t min_overlap, const sigax_trim_opts* opts,
                               void* d_seq_offs, void* d_lay_offs, void* d_uflags, sigax_placement* d_layout, void* d_useqs,
                               void* d_removed, sigax_edge* d_uedges, void* d_status12, void* d_work, uint64_t work_bytes,
                               void* stream);
/* Host buffers, synchronous; as sigax_unitigs_host.  *layout has lay_offs[n_unitigs] entries, *removed u32[n_reads], *uedges
 * status12[11] records (pass uedges = NULL for no graph); all malloc'd, release with sigax_free.  status12 is filled.  It reads each
 * round's outcome and stops after the first round that removed nothing. */
int  sigax_unitigs_trim_host(int device, const sigax_edge* edges, uint64_t n_edges, const uint32_t* lengths, const char* seqs,
                             const uint64_t* offs, uint64_t n_reads, uint32_t min_overlap, const sigax_trim_opts* opts,
                             uint64_t* n_unitigs, uint64_t** seq_offs, uint64_t** lay_offs, uint32_t** uflags,
                             sigax_placement** layout, char** useqs, uint32_t** removed, sigax_edge** uedges,
                             uint64_t status12[12]);
/* ---- `siga unitig -x -d`: non-maximal overlap cutting in the rounds (csrc/sigax_unitig.hip) ---------------------------------------
 * The second visitor of a round of the reference's default `assemble` loop (src/assembler.cpp:166-221): MaximumOverlapVisitor
 * (src/bigraph_visitors.cpp:410-512; -d, --max-overlap-carefully, -N, -G, -T) before TrimVisitor, each followed by simplify().
 * ChimericVisitor is the block after this one; LoopRemoveVisitor and the paired and linked-read visitors are not restated.
 * Everything not said here is as
 * in the `siga unitig -x` block above: record classes, B/E ends, degrees, simple records, rings, orientation, numbering, the
 * trim verdict, lifted records.
 *
 * sigax_prune_opts: max_rounds, min_branch_length, min_branch_coverage as in sigax_trim_opts; delta (-d), careful (0 or 1),
 * reserved = 0, num_reads N (-N; at least n_reads, so that no unitig holds more reads than N), genome_size G (-G; not 0 when
 * delta > 0), uniq_threshold T (-T).
 *
 * State: removed[read] as above, and cut[i] per record: 0, or the round in which record i was cut.  A record is LIVE if it is
 * kept, not cut, and both its reads are alive.  Degrees, links, unitigs, trim verdicts and lifting run over live records only.
 *
 * One round r = 1, 2, ...:
 *   CUT STEP   the unitigs of the current state are built; every cut is decided from that state alone; cut records get
 *              cut[i] = r.
 *   TRIM STEP  exactly the trim round above, over the state the cut step left (the reference's simplify() between the two
 *              visitors: here everything is recomputed from the reads); removed reads get removed[read] = r.
 * A round in which neither step changed anything ends the loop and is not counted.  At most max_rounds (<= 64) rounds run.
 *
 * The cut verdict.  PARTICIPANTS are the live records that are not containments (the reference asserts a graph without
 * containments; here a containment sets no maximum and is never cut).  A record touches the two states (read ends) its
 * classification names.  max[s] = the largest length among the participants that touch state s.  U(s) = the unitig of the
 * read of s.  unique(U) iff score >= T, with
 *   score = (N - K) * (log(G - bases) - log(G - 2 * bases)) - K * log(2.0)
 * in double as :441-450 writes it, K = the reads of U, bases = its bases; for bases < G <= 2 * bases the second logarithm is
 * log(0.001), as there; for bases >= G the reference's unsigned difference wraps and its expression means nothing: such a
 * unitig counts as NOT unique.  The device's log need not round as the host's does: a score within rounding of T may fall on
 * either side.
 * Record i, touching s and t, is a CANDIDATE FROM s iff unique(U(s)) and max[s] - length_i >= delta.
 *   careful = 0: record i is cut iff it is a candidate from s or from t.
 *   careful = 1: a candidate from s is HELD BACK
 *     when U(s) != U(t): if some participant j touches t, has its other end in U(s) (at either end of it: the reference
 *       compares vertices, not edges, :478-483; record i itself and parallel records between the two unitigs count), and has
 *       max[t] - length_j < delta;
 *     when U(s) == U(t) (a self edge of the merged vertex): if some participant of length max[s] at s has both its ends in U(s).
 *     Record i is cut iff it is a candidate from some side and not held back on that side.
 * delta must be >= 1 to cut: delta = 0 means no cut step, and the result is exactly that of sigax_unitigs_trim_* with cut all
 * zero.  (The reference's delta = 0 keeps one record per end, and which one depends on the tie order of std::sort; that is not
 * restated.  The self-edge rule above differs from the reference only where such a tie decides there.)  delta = 1 keeps every
 * longest record of an end and cuts all shorter ones.
 *
 * status16 = 16 u64, written: 0-11 as status12, with 6 = rounds that changed something (cut or removed) and 10 = uncut kept
 * records dropped because one of their reads was removed; 12 records cut, 13 rounds in which something was cut, 14 unique
 * unitigs seen by the first round's cut step, 15 = 0.
 *
 * sigax_unitigs_prune_device: sigax_unitigs_trim_device with these options, d_cut u32[n_edges] (4-byte aligned) and d_status16.
 * Asynchronous on `stream`, allocates nothing, never waits for the device; it enqueues max_rounds rounds, whose launches return
 * at once after a round that changed nothing.  d_work = sigax_unitigs_prune_workspace(n_reads, n_edges, d_uedges != NULL,
 * careful) bytes: the trim call's scratch, and per read 12 bytes (20 with careful), per record nothing without careful and with
 * it 8 bytes per slot of a table of the first power of two >= 4 n_edges slots (32 to 64 bytes per record).  Refusals as for the trim call, and
 * careful > 1, reserved != 0, num_reads < n_reads, genome_size == 0 with delta > 0: SIGAX_E_ARG.  Whatever the records hold,
 * nothing outside the buffers is touched. */
typedef struct sigax_prune_opts {
  uint32_t max_rounds, min_branch_length, min_branch_coverage, delta, careful, reserved;
  uint64_t num_reads, genome_size;
  double uniq_threshold;
} sigax_prune_opts;
int  sigax_unitigs_prune_workspace(uint64_t n_reads, uint64_t n_edges, int want_graph, int careful, uint64_t* bytes);  /* host arithmetic only */
int  sigax_unitigs_prune_device(int device, const sigax_edge* d_edges, uint64_t n_edges, const void* d_lengths, const void* d_seqs,
                                const void* d_offs, uint64_t n_reads, uint32_t min_overlap, const sigax_prune_opts* opts,
                                void* d_seq_offs, void* d_lay_offs, void* d_uflags, sigax_placement* d_layout, void* d_useqs,
                                void* d_removed, void* d_cut, sigax_edge* d_uedges, void* d_status16, void* d_work,
                                uint64_t work_bytes, void* stream);
/* Host buffers, synchronous; as sigax_unitigs_trim_host, plus *cut u32[n_edges] (malloc'd, sigax_free) and status16.  It stops
 * after the first round that changed nothing. */
int  sigax_unitigs_prune_host(int device, const sigax_edge* edges, uint64_t n_edges, const uint32_t* lengths, const char* seqs,
                              const uint64_t* offs, uint64_t n_reads, uint32_t min_overlap, const sigax_prune_opts* opts,
                              uint64_t* n_unitigs, uint64_t** seq_offs, uint64_t** lay_offs, uint32_t** uflags,
                              sigax_placement** layout, char** useqs, uint32_t** removed, uint32_t** cut, sigax_edge** uedges,
                              uint64_t status16[16]);
/* ---- `siga unitig -x -l`: chimeric unitig removal in the rounds (csrc/sigax_unitig.hip) ------------------------------------------
 * The last visitor of a round of the reference's default `assemble` loop: ChimericVisitor (src/bigraph_visitors.cpp:83-198,
 * src/assembler.cpp:207-213; -l, -A, -a, -N, -G, -T), after MaximumOverlapVisitor and TrimVisitor, each followed by simplify().
 * It removes the short, thinly covered vertex that bridges two places of the genome.  Everything not said here is as in the
 * `-x` and `-d` blocks above: record classes, B/E ends, live records, degrees, unitigs, rings, the trim verdict, PARTICIPANTS
 * (live records that are no containments), unique(U), lifted records.
 *
 * sigax_chimeric_opts: prune = the sigax_prune_opts of the block above; min_chimeric_length Lc (-l; 0 = no chimeric step),
 * min_chimeric_coverage Ac (-A; 0xFFFFFFFF = no coverage test), chimeric_delta delta_c (-a), reserved2 = 0,
 * chimeric_threshold Tc (-T as the chimeric visitor takes it).
 *
 * One round r = 1, 2, ...: CUT STEP (when delta > 0), TRIM STEP, CHIMERIC STEP (when Lc > 0).  Each step runs over the state the
 * step before left and takes every decision from the state at its own start.  A round in which no step changed anything ends
 * the loop and is not counted.
 *
 * The chimeric verdict.  For the unitigs of the state at the start of the step, sL and sR are the outward read ends of unitig
 * U and dL, dR their degrees, as the trim block defines them; K(U) its reads, bases(U) its bases.  U is CHIMERIC iff
 *   1. ENDS        dL == 1 and dR == 1, and the one live record at each of sL and sR is a participant.  p = the state at the
 *                  other end of sL's record, q = that of sR's; P = U(p), Q = U(q).  (A ring's ends carry each other: 3 fails.)
 *   2. SIZE        bases(U) <= Lc and, when Ac is given, (K(U) - 1) * max(Lc, 1) <= (max(Ac, 1) - 1) * bases(U) in u64: the
 *                  cross-multiplied Point::avg of the trim verdict.
 *   3. NEIGHBOURS  deg[p] >= 2 and deg[q] >= 2 (degrees as everywhere: containments count).
 *   4. SUPPORT     good(p) or good(q).  good(p) iff unique(P) under Tc (the expression and the bases >= G rule of the -d block)
 *                  and, over the OTHERS of p -- the participants that touch p and have their other end outside U -- either
 *                  every one has min(bases(U(other)), 2^32 - 1) > bases(U) + delta_c (u64), or every one has K(U(other)) >
 *                  K(U) + 3.  With no others both hold, as the reference's loops do.  (A unitig of 2^32 - 1 bases or more counts
 *                  as one of 2^32 - 1: that decides only where bases(U) + delta_c reaches 2^32 - 1.)
 * All reads of a chimeric unitig get removed[read] = r | SIGAX_REMOVED_CHIMERIC.  Only these entry points ever set that bit.
 *
 * Deviations from the reference:
 *   which end of the neighbour  The reference asks prevVert->degrees(ED_SENSE) and nextVert->degrees(ED_ANTISENSE) and walks those
 *       edge lists, whatever end the edge's twin leaves from.  For a neighbour joined on the other strand that is the wrong
 *       end, and for a merged vertex which end is SENSE depends on the order of its hash map.  Here it is always the end the
 *       record touches.  The two agree wherever neighbour and vertex lie on one strand.
 *   coverage option  The reference's -A never reaches the visitor (assembler.cpp:56 reads `max-chimeric-coverage`, the option is
 *       named `min-chimeric-coverage`), so its coverage test always passes.  Here Ac works; not given = no test.
 *   default of -a  The reference's default of -1 makes seq.length() + _delta wrap to length - 1.  Here delta_c is a u32 added in
 *       u64, default 0.
 *   defaults of N and G  The reference's fallbacks for N = 0 and G = 0 are not restated: G is required, N defaults to the reads.
 *   scores near Tc  A score within rounding of Tc may fall on either side: the device's log need not round as libm's does.
 *
 * status20 = 20 u64, written: 0-15 as status16, with 6 = rounds in which any step changed something, 9 = all removed reads, 7
 * and 8 the trim steps' islands and dead ends only; 16 chimeric unitigs removed, 17 reads the chimeric steps removed, 18 rounds
 * in which a chimeric step removed something, 19 = 0.
 *
 * sigax_unitigs_chimeric_device: sigax_unitigs_prune_device with these options and d_status20.  Asynchronous on `stream`,
 * allocates nothing, never waits for the device; it enqueues max_rounds rounds, whose launches return at once after a round that
 * changed nothing.  d_work = sigax_unitigs_chimeric_workspace(n_reads, n_edges, d_uedges != NULL, careful) bytes: the prune
 * call's scratch and 72 bytes per read.  min_chimeric_length = 0 gives exactly the prune call's result, status 16-19 zero and no
 * flag bit.  Refusals as for the prune call, and reserved2 != 0, min_chimeric_length > 0 with genome_size == 0 or with num_reads
 * < n_reads: SIGAX_E_ARG.  Whatever the records hold, nothing outside the buffers is touched. */
#define SIGAX_REMOVED_CHIMERIC 0x80000000u
typedef struct sigax_chimeric_opts {
  sigax_prune_opts prune;
  uint32_t min_chimeric_length;    /* Lc; 0 = no chimeric step */
  uint32_t min_chimeric_coverage;  /* Ac; SIGAX_TRIM_NO_COVERAGE = no test */
  uint32_t chimeric_delta;
  uint32_t reserved2;              /* = 0 */
  double   chimeric_threshold;     /* Tc */
} sigax_chimeric_opts;
int  sigax_unitigs_chimeric_workspace(uint64_t n_reads, uint64_t n_edges, int want_graph, int careful, uint64_t* bytes);  /* host arithmetic only */
int  sigax_unitigs_chimeric_device(int device, const sigax_edge* d_edges, uint64_t n_edges, const void* d_lengths, const void* d_seqs,
                                   const void* d_offs, uint64_t n_reads, uint32_t min_overlap, const sigax_chimeric_opts* opts,
                                   void* d_seq_offs, void* d_lay_offs, void* d_uflags, sigax_placement* d_layout, void* d_useqs,
                                   void* d_removed, void* d_cut, sigax_edge* d_uedges, void* d_status20, void* d_work,
                                   uint64_t work_bytes, void* stream);
/* Host buffers, synchronous; as sigax_unitigs_prune_host, with status20.  It stops after the first round that changed nothing. */
int  sigax_unitigs_chimeric_host(int device, const sigax_edge* edges, uint64_t n_edges, const uint32_t* lengths, const char* seqs,
                                 const uint64_t* offs, uint64_t n_reads, uint32_t min_overlap, const sigax_chimeric_opts* opts,
                                 uint64_t* n_unitigs, uint64_t** seq_offs, uint64_t** lay_offs, uint32_t** uflags,
                                 sigax_placement** layout, char** useqs, uint32_t** removed, uint32_t** cut, sigax_edge** uedges,
                                 uint64_t status20[20]);
/* ---- `siga unitig -x -b`: bubble popping in the rounds (csrc/sigax_unitig.hip) ----------------------------------------------------
 * A bubble is two unitigs that leave the same unitig end and arrive at the same unitig end: a heterozygous SNP, a two-copy
 * near-repeat, a recurring error.  Neither arm is a tip, both carry overlaps of full length, and the chimeric step leaves both or
 * takes both.  The reference declares the step and never wrote it: SmoothingVisitor::visit returns false
 * (src/bigraph_visitors.cpp:1021-1036).  So there is nothing to restate and nothing to deviate from; the rules below are this
 * library's own, and no decision depends on record, read or hash-map order.  Everything not said here is as in the `-x`, `-d` and
 * `-l` blocks above: live records, PARTICIPANTS, sL, sR, dL, dR, K(U), bases(U), and a state = 2 * read + end.  DESIGN.md 9j; the
 * serial restatement the tests hold this against is tests/bubble_cases.py::expected_bubble.
 *
 * sigax_bubble_opts: chimeric = the sigax_chimeric_opts of the block above; max_bubble_span Lb (-b; 0 = no bubble step),
 * max_divergence_permille D (--bubble-divergence; SIGAX_BUBBLE_NO_BASES = no bases test), reserved3 = 0.
 *
 * One round r = 1, 2, ...: CUT STEP (when delta > 0), TRIM STEP, BUBBLE STEP (when Lb > 0), CHIMERIC STEP (when Lc > 0).  The bubble
 * step comes before the chimeric step on purpose: once the losing arm is gone the winner's neighbours are no longer branched, so
 * the chimeric step cannot take the surviving arm in the same round.  Each step runs over the state the step before left and takes
 * every decision from the state at its own start.  A round in which no step changed anything ends the loop and is not counted.
 *
 * The bubble verdict, for the unitigs of the state at the start of the step:
 *   1. ARM    U is an arm iff it is no ring, dL == 1 and dR == 1, the one live record at each of sL and sR is a participant, and,
 *             with p, q the states at the other ends of those records, U(p) != U, U(q) != U and p != q.  U(p) == U(q) is allowed:
 *             the two ends of one unitig may carry a bubble.  key(U) = (lo, hi) = (min(p, q), max(p, q)); o_lo, o_hi are the
 *             lengths of the records at those sides; span(U) = bases(U) - o_lo - o_hi as a signed 64-bit value.  An arm takes
 *             part iff 1 <= span(U) <= Lb.
 *   2. GROUP  The arms that take part and share (lo, hi, span) form a group.  A group of one does nothing.  In a group of two or
 *             more the WINNER is the arm with the largest K, then the smallest id of its first read (the read its layout begins
 *             with); every other arm of the group is a LOSER.
 *   3. BASES  S(U) is the unitig's bases exactly as the final pass would write them for U.  A(U) = S(U) if U's left end is the
 *             one joined to lo, otherwise its reverse complement, bytes complemented as the bases pass complements them (A <-> T,
 *             C <-> G, every other byte itself).  mism(L, W) is the number of t in [0, span) with A(L)[o_lo(L) + t] !=
 *             A(W)[o_lo(W) + t]; outside that window both arms equal the neighbours' bases, because overlaps are exact.  Loser L
 *             is POPPED iff D == SIGAX_BUBBLE_NO_BASES, or mism * 1000 <= D * span in u64.  A loser that fails the test stays
 *             and is counted.
 *   4. MARK   All reads of a popped arm get removed[read] = r | SIGAX_REMOVED_BUBBLE.  Only these entry points ever set that bit.
 *             A winner is never removed by this step.  An arm is in exactly one group.
 * Out of scope: arms of different span (indel bubbles: the `--bubble-edits` block below); bubbles whose arms are themselves branched (paths, not unitigs); a
 * second candidate winner when the first fails the bases test.  Not held: inputs beyond 2^32 bases (nor are the prune and
 * chimeric rounds).
 *
 * status24 = 24 u64, written: 0-19 as status20, with 6 = rounds in which any step changed something and 9 = all removed reads;
 * 20 arms popped, 21 reads the bubble steps removed, 22 rounds in which a bubble step removed something, 23 losers kept because
 * they failed the bases test, summed over the rounds that ran.
 *
 * sigax_unitigs_bubble_device: sigax_unitigs_chimeric_device with these options and d_status24.  Asynchronous on `stream`,
 * allocates nothing, never waits for the device; it enqueues max_rounds rounds, whose kernels return at once after a round that
 * changed nothing (the one prefix sum of a bubble step with a bases test has no such form; nothing reads its result then).  Every
 * index is checked against its buffer; the comparison loop is bounded by Lb, the bisection over a unitig's placements by 32 steps,
 * the group table's probes by its capacity.  d_work = sigax_unitigs_bubble_workspace(n_reads, n_edges, d_uedges != NULL, careful)
 * bytes: the chimeric call's scratch, 60 bytes per read, 12 bytes per slot of the group table (the power of two >= max(16,
 * 2 n_reads)), and 25 216 bytes of counters, each piece rounded up to 16 bytes.  max_bubble_span = 0 gives exactly the chimeric
 * call's result, status 20-23 zero and no new flag bit.  The bubble step needs neither genome_size nor num_reads.  Refusals as
 * for the chimeric call, and reserved3 != 0: SIGAX_E_ARG; d_seqs == NULL is refused with any n_reads > 0, so with a bases test
 * too.  Whatever the records hold, nothing outside the buffers is touched. */
#define SIGAX_REMOVED_BUBBLE 0x40000000u
#define SIGAX_BUBBLE_NO_BASES 0xFFFFFFFFu
typedef struct sigax_bubble_opts {
  sigax_chimeric_opts chimeric;
  uint32_t max_bubble_span;          /* Lb; 0 = no bubble step */
  uint32_t max_divergence_permille;  /* D; SIGAX_BUBBLE_NO_BASES = no bases test */
  uint32_t reserved3[2];             /* = 0 */
} sigax_bubble_opts;
int  sigax_unitigs_bubble_workspace(uint64_t n_reads, uint64_t n_edges, int want_graph, int careful, uint64_t* bytes);  /* host arithmetic only */
int  sigax_unitigs_bubble_device(int device, const sigax_edge* d_edges, uint64_t n_edges, const void* d_lengths, const void* d_seqs,
                                 const void* d_offs, uint64_t n_reads, uint32_t min_overlap, const sigax_bubble_opts* opts,
                                 void* d_seq_offs, void* d_lay_offs, void* d_uflags, sigax_placement* d_layout, void* d_useqs,
                                 void* d_removed, void* d_cut, sigax_edge* d_uedges, void* d_status24, void* d_work,
                                 uint64_t work_bytes, void* stream);
/* Host buffers, synchronous; as sigax_unitigs_chimeric_host, with status24.  It stops after the first round that changed nothing. */
int  sigax_unitigs_bubble_host(int device, const sigax_edge* edges, uint64_t n_edges, const uint32_t* lengths, const char* seqs,
                               const uint64_t* offs, uint64_t n_reads, uint32_t min_overlap, const sigax_bubble_opts* opts,
                               uint64_t* n_unitigs, uint64_t** seq_offs, uint64_t** lay_offs, uint32_t** uflags,
                               sigax_placement** layout, char** useqs, uint32_t** removed, uint32_t** cut, sigax_edge** uedges,
                               uint64_t status24[24]);
/* ---- `siga unitig -x -b --bubble-edits`: indel bubble popping in the rounds (csrc/sigax_unitig.hip) ---------------------------------
 * The bubble step above pops an arm only where it holds as many bases between its two neighbours as the winner: substitutions.  An
 * inserted or deleted base gives two arms of different span, which no other step takes: both carry full-length overlaps at both
 * ends.  The INDEL STEP compares such arms by a bounded edit distance.  Nothing of it is in the reference (SmoothingVisitor::visit
 * returns false); the rules are this library's own, and no decision depends on the order of records, reads, lanes or table slots.
 * Everything not said here is as in the `-b` block above: live records, PARTICIPANTS, ARM, key(U) = (lo, hi), o_lo, o_hi, span,
 * A(U), K, bases(U).  DESIGN.md 9n; the serial restatement the tests hold this against is tests/indel_cases.py::expected_indel.
 *
 * sigax_indel_opts: bubble = the sigax_bubble_opts of the block above (its reserved3 still 0); max_edits E (--bubble-edits; 0 = no
 * indel step; at most 31), max_edit_permille De (--bubble-edit-permille), reserved4 = 0.  With E > 0 the call needs 0 <
 * max_bubble_span <= 4096: Lb bounds the windows, and 4096 bytes per window is what one wave stages.
 *
 * One round r = 1, 2, ...: CUT STEP, TRIM STEP, BUBBLE STEP (when Lb > 0), INDEL STEP (when E > 0), CHIMERIC STEP.  Each step runs over
 * the state the step before left and takes every decision from the state at its own start.  A round in which no step changed
 * anything ends the loop and is not counted.  The indel step comes before the chimeric step for the reason the bubble step does.
 *
 * The indel verdict, for the unitigs of the state at the start of the step:
 *   1. ARM    As in the bubble block, and an arm takes part iff 1 <= span(U) <= Lb.
 *   2. GROUP  The arms that take part and share (lo, hi) form a group, whatever their spans.  A group of one does nothing.  The
 *             WINNER W is the arm with the largest K, then the smallest id of its first read; every other arm is a LOSER.
 *   3. PAIR   For a loser L with a = span(L), b = span(W): a == b: SAME_SPAN, the bubble step's business; it is not compared here
 *             and stays.  |a - b| > E: FAR; it stays.  Otherwise the pair is compared.
 *   4. EDITS  X(U) = A(U)[o_lo(U) .. o_lo(U) + span(U)).  ed = the unit-cost Levenshtein distance between X(L) and X(W), bytes
 *             compared as bytes (N equals N, lower case differs from upper case), computed exactly up to E and "more than E"
 *             beyond.  L is POPPED iff ed <= E and ed * 1000 <= De * min(bases(L), bases(W)) in u64: the divergence is measured
 *             against the shorter arm, not against the window.  A compared loser that fails stays and is counted.
 *   5. MARK   All reads of a popped arm get removed[read] = r | SIGAX_REMOVED_INDEL.  Only these entry points ever set that bit.  A
 *             winner is never removed by this step.
 * Out of scope: arms with span < 1 (the neighbours reach into each other: tandem indels, an indel inside a repeat longer than the
 * window); bubbles whose arms are themselves branched; a second candidate winner when the first fails; inputs beyond 2^32 bases
 * (the bubble rounds do not hold them either).
 *
 * status32 = 32 u64, written: 0-23 as status24, with 6 = rounds in which any step changed something and 9 = all removed reads, both
 * including this step; 24 arms the indel steps popped, 25 their reads, 26 rounds in which an indel step removed something, 27
 * compared losers kept, 28 losers not compared (SAME_SPAN + FAR), 27 and 28 summed over the rounds that ran; 29-31 zero.
 *
 * sigax_unitigs_indel_device: sigax_unitigs_bubble_device with these options and d_status32.  Asynchronous on `stream`, allocates
 * nothing, never waits for the device; it enqueues max_rounds rounds, whose kernels return at once after a round that changed
 * nothing (the prefix sum of an indel step has no such form; nothing reads its result then).  Every index is checked against its
 * buffer; the recurrence runs at most E + 1 turns, a slide at most Lb steps, the bisection over a unitig's placements 32 steps, the
 * group table's probes its capacity.  d_work = sigax_unitigs_indel_workspace(n_reads, n_edges, d_uedges != NULL, careful) bytes: the
 * bubble call's scratch, then 33 408 bytes of counters and 4 bytes per read, each piece rounded up to 16 bytes.  max_edits = 0 gives
 * exactly the bubble call's result, status 24-31 zero and no new flag bit.  Refusals as for the bubble call, and reserved4 != 0,
 * max_edits > 31, max_edits > 0 with max_bubble_span == 0 or > 4096: SIGAX_E_ARG.  Whatever the records hold, nothing outside the
 * buffers is touched. */
#define SIGAX_REMOVED_INDEL 0x20000000u
#define SIGAX_INDEL_MAX_EDITS 31u
#define SIGAX_INDEL_MAX_SPAN 4096u
typedef struct sigax_indel_opts {
  sigax_bubble_opts bubble;
  uint32_t max_edits;          /* E; 0 = no indel step; at most SIGAX_INDEL_MAX_EDITS */
  uint32_t max_edit_permille;  /* De */
  uint32_t reserved4[2];       /* = 0 */
} sigax_indel_opts;
int  sigax_unitigs_indel_workspace(uint64_t n_reads, uint64_t n_edges, int want_graph, int careful, uint64_t* bytes);  /* host arithmetic only */
int  sigax_unitigs_indel_device(int device, const sigax_edge* d_edges, uint64_t n_edges, const void* d_lengths, const void* d_seqs,
                                const void* d_offs, uint64_t n_reads, uint32_t min_overlap, const sigax_indel_opts* opts,
                                void* d_seq_offs, void* d_lay_offs, void* d_uflags, sigax_placement* d_layout, void* d_useqs,
                                void* d_removed, void* d_cut, sigax_edge* d_uedges, void* d_status32, void* d_work,
                                uint64_t work_bytes, void* stream);
/* Host buffers, synchronous; as sigax_unitigs_bubble_host, with status32.  It stops after the first round that changed nothing. */
int  sigax_unitigs_indel_host(int device, const sigax_edge* edges, uint64_t n_edges, const uint32_t* lengths, const char* seqs,
                              const uint64_t* offs, uint64_t n_reads, uint32_t min_overlap, const sigax_indel_opts* opts,
                              uint64_t* n_unitigs, uint64_t** seq_offs, uint64_t** lay_offs, uint32_t** uflags,
                              sigax_placement** layout, char** useqs, uint32_t** removed, uint32_t** cut, sigax_edge** uedges,
                              uint64_t status32[32]);
/* ---- `siga unitig --reduce`: transitive reduction in the rounds (csrc/sigax_unitig.hip) --------------------------------------------
 * An irreducible overlap run decides once, at overlap time, which overlaps a third read explains, and an exhaustive run keeps them
 * all: about 21 records per read instead of 1.1, nearly every read end branched.  A REDUCTION PASS decides it on the graph, over
 * what is alive now: it turns an exhaustive record set back into a string graph, and it lets a record return whose witness a later
 * round removed.  The reference declares this step and leaves it empty (TransitiveReductionVisitor, src/bigraph_visitors.cpp:1084-1093);
 * the rules are this library's own, and on error-free reads without duplicate or contained reads they leave exactly the records
 * the reference's irreducible overlap run writes (tests/test_reduce_cases.py holds that).  No decision depends on the order of
 * records, reads, lanes or table slots.  Everything not said here is as in the blocks above: record classes, B/E ends, states
 * 2 * read + end, degrees, live records, simple records, rings, lifted records.  DESIGN.md 9o; the serial restatement the tests hold
 * this against is tests/reduce_cases.py::expected_reduce.
 *
 * PARTICIPANTS of a pass: the records that are kept, have both reads alive, were not cut in an earlier round
 *             (cut[i] & 0x7FFFFFFF == 0), and are neither a containment nor a self edge.  A participant between states a and b of
 *             reads ra, rb with overlap len has two extensions: ext(a -> b) = L[rb] - len and ext(b -> a) = L[ra] - len.
 * TRANSITIVE  Seen from a, participant i is transitive iff a participant j != i exists between a and a state w of a third read, and
 *             a participant k exists between w ^ 1 (the other end of that read) and b, with
 *             ext(a -> w) + ext((w ^ 1) -> b) == ext(a -> b).  The equality is exact, as the overlaps are; there is no fuzz.  Record i
 *             is transitive in this pass iff it is so seen from a or seen from b.
 * WITNESSES   ignore the flag: j and k may themselves be transitive.  So the verdicts of a pass depend neither on record order nor
 *             on each other; every decision uses the participant set at the start of the pass.
 * NOT TAKING PART  A containment or a self edge is never flagged and never a witness.  Two records between the same two states with
 *             different lengths are judged one by one; the sum rule keeps a record at one offset from being explained through a
 *             witness at another.
 * THE FLAG    Bit 31 of cut[i], SIGAX_CUT_TRANSITIVE: transitive in the latest pass.  Every pass clears it on all records and sets
 *             it anew.  The low 31 bits keep the round of a `-d` cut.  Every step of a round takes a record with cut[i] != 0 as not
 *             there, whichever bits are set; whoever reads cut[] as a round masks bit 31 off.
 * WHEN        With reduce = 1 a pass is the first step of every round: reduce, cut, trim, bubble, indel, chimeric.  One more pass
 *             runs before the final unitigs and the lifted records, so a record whose only witnesses went in the last round is live
 *             again and can be merged.  With max_rounds = 0 that is the only pass: "reduce, then simplify()".
 * IDLE        A pass after a round that changed nothing leaves at once, like every other step; the flags of the pass before still
 *             hold.  A pass does not count as a change for the purpose of ending the loop: it removes nothing that anything else
 *             could have used.  The first pass of a call always runs.
 * Flagged records are not lifted: d_uedges and the `--graph` ASQG leave them out.  status[10] does not count them.
 * Out of scope: any fuzz or inexact reduction; reduction over containments.
 *
 * sigax_reduce_opts: indel = the sigax_indel_opts of the block above (its reserved4 still 0); reduce 0 or 1; reserved5 = 0.
 *
 * status40 = 40 u64, written: 0-31 as status32; 32 records flagged by the first pass of the call, 33 records flagged in the final
 * graph (by the last pass that ran), 34 passes that ran and were not idle, 35 participants of the last pass that ran; 36-39 zero.
 *
 * sigax_unitigs_reduce_device: sigax_unitigs_indel_device with these options and d_status40.  Asynchronous on `stream`, allocates
 * nothing, never waits for the device.  A pass counts the participants per state, takes the exclusive prefix sum, writes {other
 * state, extension} into both states' segments and the record's index into an open-addressing table keyed exactly by (state, state,
 * overlap), and then walks, one lane per record, the segment of each of its ends: trips bounded by the end's degree, probes by the
 * table's capacity.  No cap changes a verdict: a read end of degree 5000 is slow, not wrong.  d_work =
 * sigax_unitigs_reduce_workspace(n_reads, n_edges, d_uedges != NULL, careful) bytes: the indel call's scratch, then 16 448 bytes of
 * counters, (2 n + 1) * 4, 2 n * 4 and (2 n + 1) * 8 bytes of counts and offsets, the prefix sum's partials, 8 bytes, 16 bytes per
 * record of segments and 4 bytes per table slot, the slots the smallest power of two that is at least 16 and at least 4 n_edges, each
 * piece rounded up to 16 bytes.  reduce = 0 gives exactly the indel call's result, bit 31 never set and status 32-39 zero.  Refusals
 * as for the indel call, and reserved5 != 0, reduce > 1, reduce = 1 with 2^32 records: SIGAX_E_ARG.  Whatever the records hold,
 * nothing outside the buffers is touched. */
#define SIGAX_CUT_TRANSITIVE 0x80000000u
typedef struct sigax_reduce_opts {
  sigax_indel_opts indel;
  uint32_t reduce;        /* 0 or 1 */
  uint32_t reserved5[3];  /* = 0 */
} sigax_reduce_opts;
int  sigax_unitigs_reduce_workspace(uint64_t n_reads, uint64_t n_edges, int want_graph, int careful, uint64_t* bytes);  /* host arithmetic only */
int  sigax_unitigs_reduce_device(int device, const sigax_edge* d_edges, uint64_t n_edges, const void* d_lengths, const void* d_seqs,
                                 const void* d_offs, uint64_t n_reads, uint32_t min_overlap, const sigax_reduce_opts* opts,
                                 void* d_seq_offs, void* d_lay_offs, void* d_uflags, sigax_placement* d_layout, void* d_useqs,
                                 void* d_removed, void* d_cut, sigax_edge* d_uedges, void* d_status40, void* d_work,
                                 uint64_t work_bytes, void* stream);
/* Host buffers, synchronous; as sigax_unitigs_indel_host, with status40.  It stops after the first round that changed nothing. */
int  sigax_unitigs_reduce_host(int device, const sigax_edge* edges, uint64_t n_edges, const uint32_t* lengths, const char* seqs,
                               const uint64_t* offs, uint64_t n_reads, uint32_t min_overlap, const sigax_reduce_opts* opts,
                               uint64_t* n_unitigs, uint64_t** seq_offs, uint64_t** lay_offs, uint32_t** uflags,
                               sigax_placement** layout, char** useqs, uint32_t** removed, uint32_t** cut, sigax_edge** uedges,
                               uint64_t status40[40]);
/* ---- `siga unitig -e`: the consensus pass, every unitig column by majority vote (csrc/sigax_consensus.hip) -------------------------
 * A unitig's bases are a copy: the first read whole, then of every next read its last L - overlap bytes.  With exact overlaps
 * every read that covers a column agrees and the copy is the truth; with the mismatch overlaps of `siga overlap -e` a column holds
 * whatever the one copied read holds there, error included.  The layout already says which reads lie over which column; this pass
 * takes the vote.  The reference has nothing like it (Vertex::merge, src/bigraph.cpp:131-202, appends label bytes); the rules are
 * these.  Integer arithmetic throughout; no vote depends on the order of placements, reads or lanes.  DESIGN.md 9r; the serial
 * restatement the tests hold this against is tests/consensus_cases.py::expected_consensus.
 *
 * Input: the outputs of any unitig call -- the number of unitigs, seq_offs, lay_offs, layout, and useqs, which on entry holds what
 * the call wrote (the OWN bases) -- and the reads (lengths, seqs, offs, n_reads).  For unitig u with U = seq_offs[u+1] - seq_offs[u]
 * columns:
 *  1. A placement (r, flags, o) of layout[lay_offs[u] .. lay_offs[u+1]) is valid iff r < n_reads and o + L[r] <= U (no wrap: o <= U
 *     and L[r] <= U - o).  An invalid one is skipped and counted; a valid one covers the columns [o, o + L[r]).
 *  2. The placed byte at column x is seqs[offs[r] + x - o] when the read lies forward, and the complement (A<->T, C<->G, every other
 *     byte as it is) of seqs[offs[r] + L[r] - 1 - (x - o)] when flags & SIGAX_PLACED_REV.
 *  3. c[A], c[C], c[G], c[T] are the numbers of valid placements whose placed byte at x is that letter.  Any other byte -- N, lower
 *     case, anything else -- does not vote.  depth = the sum of the four.
 *  4. The winner w is the letter with the most votes, a tie going to the earliest in the order A, C, G, T.
 *  5. own = the byte of useqs at x on entry, c_own = c[own] if it is one of the four letters, else 0.  The column becomes w iff
 *     c[w] > c_own and c[w] >= min_votes; otherwise it stays.  An own base that ties for first place stays, so with exact overlaps
 *     nothing ever changes.
 *  6. A ring is treated as a line: a placement votes on the columns it covers and on nothing else; the closing overlap of a
 *     SIGAX_UNITIG_CIRCULAR unitig is not wrapped round.
 *
 * Output: useqs rewritten in place (every column is written by one lane, and that lane reads nothing of useqs but its own byte);
 * changed u32 per unitig, the columns replaced; support u8 per column, optional (NULL: not wanted): min(255, votes for the byte the
 * column holds on return), 0 where that byte is no letter.  status8 = 8 u64, written: 0 unitigs seen, 1 columns, 2 columns changed,
 * 3 columns of depth below 2, 4 columns where the own base stayed on a tie with another letter (own is a letter with at least one
 * vote, no letter has more, another has as many), 5 columns held back by min_votes (c[w] > c_own but c[w] < min_votes), 6 the
 * largest depth, 7 placements skipped as invalid.
 *
 * sigax_consensus_opts: min_votes >= 1 (CLI --consensus-min-votes, default 1), reserved = 0.
 *
 * sigax_consensus_device: every buffer in device memory, asynchronous on `stream`, allocates nothing, never waits for the device,
 * so it can be enqueued straight behind a unitig call.  d_n_unitigs points at a u64 ON THE DEVICE -- entry 0 of the unitig call's
 * status block; a value above n_reads or above max_unitigs is taken as that.  d_seq_offs and d_lay_offs u64[max_unitigs + 1],
 * d_layout sigax_placement[n_reads], d_lengths u32[n_reads], d_offs u64[n_reads + 1], d_seqs indexed by d_offs; d_useqs and
 * d_support (or NULL) offs[n_reads] - offs[0] bytes as the unitig call's, d_changed u32[max_unitigs], of which entries 0 ..
 * n_unitigs - 1 are counts and the rest zero; d_work = sigax_consensus_workspace bytes (counters: some 48 KiB whatever the sizes).
 * d_layout, d_useqs, d_support and d_work 16-byte aligned, d_n_unitigs, d_seq_offs, d_lay_offs, d_offs and d_status8 8-byte aligned,
 * d_lengths and d_changed 4-byte aligned.  A NULL where a buffer is required, a misaligned buffer, a short workspace, min_votes =
 * 0, a non-zero reserved word and n_reads >= 2^31: SIGAX_E_ARG.  n_reads = 0 (or max_unitigs = 0): SIGAX_OK, status zeros.
 * Whatever layout, lay_offs and seq_offs hold -- read ids that are too large, offsets beyond the unitig, tables that do not ascend
 * -- nothing outside the buffers is touched, and every loop has a bound the host knows.  The pass finds the placements over a
 * column by bisection: the rules above are met exactly where seq_offs and lay_offs ascend and, within each unitig, the offsets
 * of its placements ascend, as every unitig call writes them (invalid placements among them or not); elsewhere some placements
 * may get no vote or no count.  Needs no index.
 * Not held: read sets beyond 2^32 bases are untested.  Votes of contained reads: a contained read votes once
 * sigax_contained_place_device has given it a placement, and this pass is run over that call's lay_offs2 and layout2.  Out of
 * scope: gapped alignment; quality-weighted votes; wrapping a ring's closing overlap; consensus inside the scaffold, gapfill and join passes. */
typedef struct sigax_consensus_opts { uint32_t min_votes; uint32_t reserved[3]; } sigax_consensus_opts;
int  sigax_consensus_workspace(uint64_t n_reads, uint64_t n_unitigs_max, uint64_t* bytes);  /* host arithmetic only */
int  sigax_consensus_device(int device, const void* d_n_unitigs, uint64_t max_unitigs, const void* d_seq_offs, const void* d_lay_offs,
                            const sigax_placement* d_layout, const void* d_lengths, const void* d_seqs, const void* d_offs,
                            uint64_t n_reads, const sigax_consensus_opts* opts, void* d_useqs, void* d_changed, void* d_support,
                            void* d_status8, void* d_work, uint64_t work_bytes, void* stream);
/* Host buffers, synchronous.  seq_offs and lay_offs u64[n_unitigs + 1], layout sigax_placement[lay_offs[n_unitigs]], useqs
 * seq_offs[n_unitigs] bytes, in and out; offs[0] need not be 0.  n_unitigs or lay_offs[n_unitigs] above n_reads, or more unitig
 * bases than read bases: SIGAX_E_ARG.  *changed u32[n_unitigs] and *support u8[seq_offs[n_unitigs]] (support = NULL: not wanted)
 * are malloc'd; release with sigax_free.  status8 is filled. */
int  sigax_consensus_host(int device, uint64_t n_unitigs, const uint64_t* seq_offs, const uint64_t* lay_offs, const sigax_placement* layout,
                          const uint32_t* lengths, const char* seqs, const uint64_t* offs, uint64_t n_reads,
                          const sigax_consensus_opts* opts, char* useqs, uint32_t** changed, uint8_t** support, uint64_t status8[8]);

/* ---- `siga unitig -e --place-contained`: contained reads placed in the layout (csrc/sigax_contained.hip) ---------------------------
 * `siga unitig -e` sets every contained read aside: it becomes a unitig of its own that is not written, and has no placement in
 * the unitig that holds its bases.  This pass takes the containment records of the mismatch overlap path (SIGAX_MMO_CONTAINMENTS)
 * and gives such a read the placement its container implies, so that it votes in the consensus pass and pairs.  The reference drops
 * contained reads before its graph is built (src/bigraph.cpp); the rules are these.  Integer arithmetic throughout; no result
 * depends on the order of records, reads or lanes.  DESIGN.md 9s; the serial restatement the tests hold this against is
 * tests/contained_cases.py::expected_placement.
 *
 * Input: a unitig call's number of unitigs, seq_offs, lay_offs and layout; lengths and n_reads; contained u8[n_reads]; n_conts
 * containment records in any order.  Unitig u holds the placements lay_offs[u] .. lay_offs[u+1] when lay_offs[u] <= lay_offs[u+1] <=
 * n_reads, none otherwise; placement j belongs to the last u with lay_offs[u] <= j if that unitig holds it, to none otherwise; a
 * read's placement is the first one that belongs to a unitig and names it.
 *  1. A record is VALID iff query and target are below n_reads, query != target, af & SIGAX_MM_CONTAINMENT, contained[query] is
 *     set and reserved + L[query] <= L[target].  Others are skipped and counted.
 *  2. CHOICE(c) is the valid record of c that is smallest in (contained[target] != 0, num_diff, target, af & 4, reserved): a
 *     container that is placed directly first, then the fewest mismatches.
 *  3. ROOT: the choices are followed from c while the current read is contained and has a choice.  c at (o, v) in r, r of length Lr
 *     at (o2, v2) in q: c lies in q at (o2 + o, v) if v2 = 0, at (o2 + Lr - o - Lc, v ^ 1) otherwise.  Records of rule 1 cannot
 *     form a cycle (the length grows or the name rank falls); the chain is resolved by pointer doubling in ceil(log2 n_reads) + 1
 *     rounds, and one that has not reached a read that is not contained by then -- a cycle in foreign tables, or a contained read
 *     without a choice at its end -- is NO_ROOT.  A contained read without a valid record is NO_RECORD.
 *  4. The root's placement (u, flags, offset) composes in the same way with (offset, flags & SIGAX_PLACED_REV) to c's placement
 *     in u; a root without a placement (a trim round took it) gives ROOT_REMOVED, an offset with o + Lc > U (U the bases of u;
 *     foreign tables only) INVALID.
 *  5. lay_offs2 / layout2: per unitig its placements less those whose read is a PLACED contained read -- the hidden unitig of such
 *     a read keeps its number and its bases and has no placement -- plus the placed contained reads with SIGAX_PLACED_CONTAINED
 *     or'ed into flags, ascending in (offset, kind: 0 chain read, 1 contained, read id): what the consensus pass's bisection needs.
 *     The chain placements keep their order among themselves (every unitig call writes them ascending).  A contained read that is
 *     not placed keeps what it had.
 *  6. place_class u8 per read: SIGAX_CP_*.  status8, written: {contained reads, records read, records invalid, placed, no record
 *     or no root, root removed, the longest chain in steps among the reads whose walk reached a root, placements in layout2}.
 *
 * sigax_contained_place_device: every buffer in device memory, asynchronous on `stream`, allocates nothing, never waits for the
 * device.  d_n_unitigs points at a u64 ON THE DEVICE -- entry 0 of the unitig call's status block; a value above n_reads or above
 * max_unitigs is taken as that.  d_seq_offs, d_lay_offs and d_lay_offs2 u64[max_unitigs + 1] (lay_offs2: entries 0 .. min(max_unitigs, n_reads)
 * written, those behind n_unitigs with the total), d_layout and d_layout2 sigax_placement[n_reads] (layout2: 0xFF behind the total), d_lengths
 * u32[n_reads], d_contained and d_place_class u8[n_reads], d_conts sigax_mm_edge[n_conts] (NULL when n_conts = 0), d_work =
 * sigax_contained_place_workspace bytes (some 120 bytes a read and the sort's scratch: the placed contained reads are ordered by
 * two radix passes over one slot a read, because only the device knows how many there are).  d_layout, d_layout2 and d_work
 * 16-byte aligned, d_n_unitigs, d_seq_offs, d_lay_offs, d_lay_offs2, d_conts and d_status8 8-byte aligned, d_lengths 4-byte aligned.
 * A NULL where a buffer is required, a misaligned buffer, a short workspace, a non-zero reserved word, n_reads >= 2^31 and n_conts
 * >= 2^32: SIGAX_E_ARG.  n_reads = 0 (or max_unitigs = 0): SIGAX_OK, status zeros, nothing else written.  Whatever the tables hold
 * -- read ids that are too large, cycles among the choices, offsets beyond the container, tables that do not ascend -- nothing
 * outside the buffers is touched and every loop has a bound the host knows; rules 1-4 and 6 hold for any tables, rule 5 where
 * lay_offs ascends, no read is placed twice and every unitig's offsets ascend.  Needs no index.
 * Not held: read sets beyond 2^32 bases are untested.  Out of scope: gapped containments; placing contained reads into
 * scaffolds; more than one GPU. */
typedef struct sigax_contained_opts { uint32_t reserved[4]; } sigax_contained_opts;  /* all 0 */
#define SIGAX_CP_NOT_CONTAINED 0u
#define SIGAX_CP_PLACED        1u
#define SIGAX_CP_NO_RECORD     2u
#define SIGAX_CP_NO_ROOT       3u
#define SIGAX_CP_ROOT_REMOVED  4u
#define SIGAX_CP_INVALID       5u
int  sigax_contained_place_workspace(uint64_t n_reads, uint64_t max_unitigs, uint64_t n_conts, uint64_t* bytes);
int  sigax_contained_place_device(int device, const void* d_n_unitigs, uint64_t max_unitigs, const void* d_seq_offs, const void* d_lay_offs,
                                  const sigax_placement* d_layout, const void* d_lengths, uint64_t n_reads, const void* d_contained,
                                  const sigax_mm_edge* d_conts, uint64_t n_conts, const sigax_contained_opts* opts, void* d_lay_offs2,
                                  sigax_placement* d_layout2, void* d_place_class, void* d_status8, void* d_work, uint64_t work_bytes,
                                  void* stream);
/* Host buffers, synchronous.  seq_offs and lay_offs u64[n_unitigs + 1], layout sigax_placement[lay_offs[n_unitigs]].  n_unitigs or
 * lay_offs[n_unitigs] above n_reads: SIGAX_E_ARG.  *lay_offs2 u64[n_unitigs + 1], *layout2 sigax_placement[n_reads] (status8[7] of
 * them written) and *place_class u8[n_reads] are malloc'd; release with sigax_free.  status8 is filled. */
int  sigax_contained_place_host(int device, uint64_t n_unitigs, const uint64_t* seq_offs, const uint64_t* lay_offs, const sigax_placement* layout,
                                const uint32_t* lengths, uint64_t n_reads, const uint8_t* contained, const sigax_mm_edge* conts,
                                uint64_t n_conts, const sigax_contained_opts* opts, uint64_t** lay_offs2, sigax_placement** layout2,
                                uint8_t** place_class, uint64_t status8[8]);
/* ---- `siga unitig --pairs`: mate-pair statistics and the links between unitig ends (csrc/sigax_pairs.hip) --------------------------
 * The data-parallel part of the reference's paired-end `assemble` (--pe-mode=1, src/assembler.cpp:75-90): InsertSizeEstimateVisitor
 * (src/bigraph_visitors.cpp:517-663) walks every unbranched chain of the read graph, notes each read's distance along the chain
 * and samples |distance(mate) - distance(read)| of every pair with both mates in one chain.  Those chains are the unitigs and
 * that distance is sigax_placement.offset, so the visitor is one pass over the layout a unitig call left.  PairedReadVisitor
 * (:669-969) searches the graph between mates under a node budget in hash-map order; its result depends on that order and it is
 * not restated.  What a paired-end user still needs -- which unitig ends the pairs join -- is given as link records.
 * DESIGN.md 9h; the serial restatement the tests hold this against is tests/pair_cases.py::expected_pairs.
 *
 * Input: the result of any of the four unitig calls (the number of unitigs, seq_offs, lay_offs, uflags, and layout with
 * lay_offs[n_unitigs] placements: fewer than n_reads after trimming), lengths u32[n_reads], mate u32[n_reads] with
 * SIGAX_NO_MATE = no mate, and sigax_pairs_opts.
 *
 * Pairs.  Read i is PAIRED iff j = mate[i] < n_reads, j != i and mate[j] == i; the pair is handled once, from its smaller id.
 * A read with mate[i] != SIGAX_NO_MATE that is not paired counts as a malformed entry and is otherwise ignored.
 *
 * Placement.  Placement p of the layout belongs to unitig u, the largest u < n_unitigs with lay_offs[u] <= p as a bisection
 * over lay_offs[0 .. n_unitigs] finds it (lo = 0, hi = n_unitigs; while hi - lo > 1: mid = (lo + hi) / 2, lo = mid if
 * lay_offs[mid] <= p, else hi = mid; at most 32 steps).  Its read has left = offset, right = offset + length, rev = flags &
 * SIGAX_PLACED_REV.  bases(u) = seq_offs[u+1] - seq_offs[u].  All arithmetic is modulo 2^64 (layouts of a unitig call never wrap).
 *
 * Every pair falls into exactly one class:
 *   UNPLACED  a mate is not in the layout (a round removed it).
 *   RING      both mates in one unitig flagged SIGAX_UNITIG_CIRCULAR.  Counted, never sampled: a distance on a ring is defined
 *             modulo the ring only (the reference samples it from wherever its hash map enters the ring).
 *   SAME      both mates in one unitig that is not circular.  d = |left(j) - left(i)| (the reference's sample, :604-614), span =
 *             max(right) - min(left).  With a = the mate of smaller left (tie: smaller id) and b the other, the pair is INWARD iff
 *             !rev(a) && rev(b), OUTWARD iff rev(a) && !rev(b), else TANDEM; every SAME pair is in exactly one of the three.  A
 *             SAME pair with span >= 2^32 is also FAR: it is left out of all sums and of the histogram (every square fits 64
 *             bits).  Every other SAME pair adds d to (n, sum d, sum d^2 in 128 bits); if it is of the library's orientation --
 *             INWARD, with SIGAX_PAIRS_OUTWARD instead OUTWARD -- it also adds span to (n, sum span, sum span^2 in 128 bits) and
 *             to hist[min(span >> hist_shift, hist_bins - 1)].
 *   ACROSS    the mates lie in different unitigs.  A read faces the unitig end its mate is expected beyond: for an inward
 *             library a forward read faces end E (1) with g = bases(u) - left and a reversed read end B (0) with g = right; with
 *             SIGAX_PAIRS_OUTWARD a forward read faces B with g = right, a reversed read E with g = bases(u) - left.  s = g_i +
 *             g_j is the span the pair would have if the two ends abutted.  If either unitig is circular the pair counts as a
 *             dropped ring link; else if max_span != 0 && s > max_span it counts as over the span; else it joins the link with
 *             key (a, b), a = 2 u + end of one mate and b that of the other, ordered a <= b (a == b cannot occur).
 *
 * Links: one sigax_pair_link per distinct key, ascending by (a, b); count pairs, min_span = the smallest s saturated at 2^32 - 1,
 * sum_span = the sum of s.  No result depends on the order in which pairs are processed.
 *
 * Options: hist_bins 1 .. 8192 (SIGAX_PAIRS_MAX_BINS), hist_shift 0 .. 31, reserved = 0, flags other than SIGAX_PAIRS_OUTWARD refused.
 *
 * status24 = 24 u64, written (not added to): 0 reads with a mate entry, 1 malformed entries, 2 pairs, 3 UNPLACED, 4 SAME, 5
 * INWARD, 6 OUTWARD, 7 TANDEM, 8 RING, 9 FAR, 10-13 {n, sum d, sum d^2 low, high}, 14-17 {n, sum span, sum span^2 low, high},
 * 18 ACROSS, 19 ring links dropped, 20 over max_span, 21 pairs that went into links, 22 link records written, 23 = 0.
 *
 * Deviations from the reference:
 *   strand flips    After a strand flip the reference's running distance adds the overhang of the read it enters, not of the
 *       one it leaves (:585-592).  With reads of one length both are the left coordinate and d is the reference's sample; with
 *       unequal lengths the reference mixes left-end and right-end coordinates.  Here d is always the difference of left ends.
 *   edge reduction  The reference's edges() (:637-663) drops containment edges and parallel edges of equal label before it asks
 *       for degrees; here the chains are the unitigs, where containments count in every degree.  The two agree on graphs without
 *       containments and duplicate reads, that is after `siga rmdup`.
 *   rings           See RING.
 *   unitig call     The reference estimates on the graph as loaded; here on whichever unitig call the caller ran (max_rounds = 0:
 *       the same graph).
 *   span, the orientation classes, the histogram and the links are not in the reference.
 *
 * sigax_unitigs_pairs_device: every buffer in device memory, asynchronous on `stream`, allocates nothing, never waits for the
 * device.  d_n_unitigs points at a u64 ON THE DEVICE -- entry 0 of the unitig call's status block -- so the call can be enqueued
 * straight behind the unitig call; a value above n_reads is taken as n_reads, and lay_offs[n_unitigs] likewise.  d_seq_offs and
 * d_lay_offs u64[n_reads + 1], d_uflags u32[n_reads], d_layout sigax_placement[n_reads] (the unitig call's buffers); d_hist
 * u64[hist_bins], fully written; d_links room for n_reads / 2 records, of which status24[22] are written; d_work =
 * sigax_unitigs_pairs_workspace bytes (some 38 bytes per read).  d_layout and d_work 16-byte aligned, d_n_unitigs, d_seq_offs,
 * d_lay_offs, d_hist, d_links and d_status24 8-byte aligned, d_mate, d_lengths and d_uflags 4-byte aligned.  A NULL where a
 * buffer is required, a misaligned buffer, a short workspace, bad options and n_reads >= 2^31: SIGAX_E_ARG.  n_reads = 0:
 * SIGAX_OK, status and histogram zeros.  Whatever mate, layout and lay_offs hold -- a placement whose read is >= n_reads,
 * lay_offs that do not ascend -- nothing outside the buffers is touched, and every loop has a bound the host knows.
 * sigax_unitigs_pairs_workspace asks the device sort for the size of its scratch: a size query, it launches nothing. */
#define SIGAX_NO_MATE        0xFFFFFFFFu
#define SIGAX_PAIRS_OUTWARD  1u     /* the library's pairs point away from each other (mate-pair libraries) */
#define SIGAX_PAIRS_MAX_BINS 8192u
typedef struct sigax_pairs_opts { uint32_t flags, hist_bins, hist_shift, reserved; uint64_t max_span; } sigax_pairs_opts;
typedef struct sigax_pair_link { uint32_t a, b, count, min_span; uint64_t sum_span; } sigax_pair_link; /* 24 bytes */
int  sigax_unitigs_pairs_workspace(int device, uint64_t n_reads, uint64_t* bytes);
int  sigax_unitigs_pairs_device(int device, const void* d_mate, const void* d_lengths, uint64_t n_reads, const void* d_n_unitigs,
                                const void* d_seq_offs, const void* d_lay_offs, const void* d_uflags, const sigax_placement* d_layout,
                                const sigax_pairs_opts* opts, void* d_hist, sigax_pair_link* d_links, void* d_status24, void* d_work,
                                uint64_t work_bytes, void* stream);
/* Host buffers, synchronous.  seq_offs and lay_offs u64[n_unitigs + 1], uflags u32[n_unitigs], layout
 * sigax_placement[lay_offs[n_unitigs]]; n_unitigs or lay_offs[n_unitigs] above n_reads: SIGAX_E_ARG.  *hist u64[hist_bins] and
 * *links sigax_pair_link[status24[22]] are malloc'd; release with sigax_free.  status24 is filled. */
int  sigax_unitigs_pairs_host(int device, const uint32_t* mate, const uint32_t* lengths, uint64_t n_reads, uint64_t n_unitigs,
                              const uint64_t* seq_offs, const uint64_t* lay_offs, const uint32_t* uflags, const sigax_placement* layout,
                              const sigax_pairs_opts* opts, uint64_t** hist, sigax_pair_link** links, uint64_t status24[24]);
/* Host arithmetic only: insert_size = (uint64_t)(sum d / n) and delta = (uint64_t)sqrt(sum d^2 / n - (sum d / n)^2) in double, as
 * the reference computes them (:622-631, the population moment); span_mean and span_sd likewise from entries 14-17, not
 * truncated.  n = 0 gives zeros.  Any output may be NULL. */
int  sigax_pairs_estimate(const uint64_t status24[24], uint64_t* insert_size, uint64_t* delta, double* span_mean, double* span_sd);
/* ---- `siga unitig --scaffold`: unitigs joined through the link records (csrc/sigax_scaffold.hip) ---------------------------------
 * What consumes the link records of the block above.  The reference's own answer to paired ends, PairedReadVisitor
 * (src/bigraph_visitors.cpp:669-969), walks the graph between mates in hash-map order and is not restated; nothing below is in
 * the reference.  A scaffold is the unitig of the `siga unitig` block with unitig for read, unitig end for read end and a gap
 * for an overlap: decide per link, take degrees per unitig end, rank the lists, cut rings, place the unitigs, write the bases.
 * No result depends on the order of the links.  DESIGN.md 9i; the serial restatement the tests hold this against is
 * tests/scaffold_cases.py::expected_scaffolds.
 *
 * Input: the result of a unitig call and of the pairs call that followed it: the number of unitigs nu, seq_offs, uflags and
 * useqs of the unitig call; links, their number nl and status24 of the pairs call.  bases(u) = seq_offs[u+1] - seq_offs[u]
 * (modulo 2^64; the tables of a unitig call never wrap).  sigax_scaffold_opts: flags, min_pairs, link_ratio, min_unitig_bases,
 * insert_size, min_gap, max_gap.
 *
 * Options: flags other than SIGAX_SCAFFOLD_INSERT_FROM_STATUS refused.  With that flag insert_size = floor(status24[15] /
 * status24[14]), taken on the device -- the mean span of the pairs of the library's orientation inside a unitig -- and 0 when
 * status24[14] == 0; the insert_size field must then be 0.  1 <= min_gap <= max_gap < 2^31 and insert_size < 2^62; anything else
 * is SIGAX_E_ARG.
 *
 * Link classes.  A link (a, b, count, min_span, sum_span) falls into the first class that applies:
 *   MALFORMED  a >= 2 nu, b >= 2 nu, a >= b, or count == 0.
 *   SELF       a >> 1 == b >> 1.
 *   CIRCULAR   either unitig is flagged SIGAX_UNITIG_CIRCULAR.
 *   SHORT      bases(u) < min_unitig_bases for either unitig.
 *   THIN       count < min_pairs.
 *   otherwise it is a CANDIDATE.
 * best[e] = the largest count among the candidates at unitig end e.  A candidate is WEAK iff link_ratio > 0 and count *
 * link_ratio <= best[a] or count * link_ratio <= best[b], in u64; the rest are STRONG.  deg[e] = the strong candidates at e (a key
 * given twice counts twice).  A strong candidate is a JOIN iff deg[a] == 1 and deg[b] == 1, else it is AMBIGUOUS.
 *
 * The gap of a join: m = sum_span / count (u64 division).  If m >= insert_size the gap is min_gap, and the join counts as
 * "estimate below min_gap".  Otherwise gap = min(max(insert_size - m, min_gap), max_gap); it counts as clamped if the upper
 * clamp applied and as below min_gap if the lower one did.  Both counts run over all joins, a cycle's closing join included.
 *
 * Scaffolds are the connected components of the unitigs under joins; a circular unitig is always a scaffold of its own.  A path
 * starts at its terminal unitig with the smaller id.  A unitig entered through B lies forward, one entered through E
 * reverse-complemented (A<->T, C<->G, other bytes as they are); the first unitig is forward iff it is left through E, a single
 * unitig is forward.  offset[0] = 0, offset[i+1] = offset[i] + bases(u_i) + gap(i, i+1); the scaffold has offset[last] +
 * bases(u_last) bases: the unitigs' bases as placed and N in every gap.  A cycle starts at its smallest unitig id, forward, left
 * through E; the join that would enter the start again is not merged: the scaffold's flag has bit 0 set and flags >> 1 is that
 * join's gap.  Scaffolds are numbered by ascending id of their first unitig.
 *
 * Output: sc_offs u64[S + 1] the scaffolds' base offsets, sc_lay_offs u64[S + 1], sc_flags u32[S], sc_layout sigax_placement[nu]
 * (read = the unitig id, flags bit 0 = SIGAX_PLACED_REV, offset within the scaffold), sseqs the bases.
 * status16 = 16 u64, written (not added to): 0 scaffolds S, 1 scaffold bases (gaps included), 2 links read, 3 MALFORMED, 4 SELF,
 * 5 CIRCULAR, 6 SHORT, 7 THIN, 8 WEAK, 9 AMBIGUOUS, 10 joins merged (a cycle's closing join is not counted), 11 cycles, 12 gap
 * bases (the N of the scaffolds: the gaps of the merged joins), 13 joins with estimate below min_gap, 14 joins clamped at max_gap,
 * 15 = 1 when status16[1] > sseqs_capacity: the bases were not written for lack of room.
 *
 * sigax_scaffold_device: every buffer in device memory, asynchronous on `stream`, allocates nothing, never waits for the
 * device.  d_n_unitigs and d_n_links point at u64 ON THE DEVICE -- entry 0 of the unitig call's status block and status24[22] of
 * the pairs call -- so the call can be enqueued straight behind sigax_unitigs_pairs_device; a count above its capacity
 * (max_unitigs, max_links) is taken as the capacity.  d_seq_offs u64[max_unitigs + 1], d_uflags u32[max_unitigs], d_useqs
 * useqs_bytes bytes: no byte at or beyond useqs_bytes is read.  d_links max_links records.  d_sc_offs and d_sc_lay_offs
 * u64[max_unitigs + 1], d_sc_flags u32[max_unitigs], d_sc_layout sigax_placement[max_unitigs]; entries beyond S (nu for the
 * layout) are not written.  d_sseqs sseqs_capacity bytes, or NULL with capacity 0 for the layout alone (d_useqs may then be
 * NULL too); the bases are written only if status16[1] <= sseqs_capacity, else nothing is written to d_sseqs.  d_status24 may
 * be NULL without SIGAX_SCAFFOLD_INSERT_FROM_STATUS; d_links and d_n_links may be NULL with max_links = 0.  d_work =
 * sigax_scaffold_workspace bytes (204 bytes per unitig, none per link).  d_useqs, d_sseqs, d_sc_layout and d_work 16-byte
 * aligned, d_uflags and d_sc_flags 4-byte aligned, every other buffer 8-byte aligned.  A NULL where a buffer is required, a
 * misaligned buffer, a short workspace, bad options, max_unitigs >= 2^31, max_links >= 2^32, sseqs_capacity >= 2^43:
 * SIGAX_E_ARG, with the offending argument named in sigax_last_error().  max_unitigs = 0: SIGAX_OK, status zeros, and
 * d_sc_offs[0] = d_sc_lay_offs[0] = 0 where those two are given (all other buffers may be NULL).  Whatever the
 * tables hold -- seq_offs that do not ascend, links beyond the unitigs -- nothing outside the buffers is touched and every loop
 * has a bound the host knows: the rankings run ceil(log2 max_unitigs) + 1 rounds, twice; a bisection at most 32 steps. */
#define SIGAX_SCAFFOLD_INSERT_FROM_STATUS 1u
typedef struct sigax_scaffold_opts {
  uint32_t flags, min_pairs, link_ratio, min_unitig_bases;
  uint64_t insert_size;
  uint32_t min_gap, max_gap;
} sigax_scaffold_opts;
int  sigax_scaffold_workspace(uint64_t max_unitigs, uint64_t max_links, uint64_t* bytes);  /* host arithmetic only */
int  sigax_scaffold_device(int device, const void* d_n_unitigs, uint64_t max_unitigs, const void* d_seq_offs, const void* d_uflags,
                           const void* d_useqs, uint64_t useqs_bytes, const sigax_pair_link* d_links, const void* d_n_links,
                           uint64_t max_links, const void* d_status24, const sigax_scaffold_opts* opts, void* d_sc_offs,
                           void* d_sc_lay_offs, void* d_sc_flags, sigax_placement* d_sc_layout, void* d_sseqs, uint64_t sseqs_capacity,
                           void* d_status16, void* d_work, uint64_t work_bytes, void* stream);
/* Host buffers, synchronous.  seq_offs u64[n_unitigs + 1], uflags u32[n_unitigs], useqs seq_offs[n_unitigs] bytes (NULL when
 * sseqs is NULL), links n_links records, status24 NULL or the pairs call's (required with SIGAX_SCAFFOLD_INSERT_FROM_STATUS).
 * It runs the layout, reads the total, then writes the bases into a buffer of exactly that size: status16[15] is 0.  *sc_offs and
 * *sc_lay_offs u64[*n_scaffolds + 1], *sc_flags u32[*n_scaffolds], *sc_layout sigax_placement[n_unitigs], *sseqs status16[1] bytes
 * (pass sseqs = NULL for the layout alone); all malloc'd, release with sigax_free. */
int  sigax_scaffold_host(int device, uint64_t n_unitigs, const uint64_t* seq_offs, const uint32_t* uflags, const char* useqs,
                         const sigax_pair_link* links, uint64_t n_links, const uint64_t* status24, const sigax_scaffold_opts* opts,
                         uint64_t* n_scaffolds, uint64_t** sc_offs, uint64_t** sc_lay_offs, uint32_t** sc_flags,
                         sigax_placement** sc_layout, char** sseqs, uint64_t status16[16]);
/* ---- `siga unitig --scaffold --gapfill`: scaffold gaps closed by k-mer walks over the reads' index (csrc/sigax_gapfill.hip) -----
 * Every join of a scaffold is a run of N whose length is an estimate from insert sizes.  The FM-index of the reads knows every
 * k-mer of the sample, the ones that bridge a unitig end included: unitigs end where the overlap graph forks or runs dry, and a
 * walk over k-mers shorter than the minimum overlap often does neither there.  The reference has no gap filler (the paired
 * visitor that would walk between mates depends on hash-map order, see the `--pairs` block), so the rules below are this
 * library's own.  DESIGN.md 9k; the serial restatement the tests hold this against is tests/gapfill_cases.py::expected_gapfill.
 *
 * Input: an open index (the forward strand is enough, and it is the only one read: no result depends on which tables the
 * index holds); seq_offs and useqs of a unitig call, nu unitigs; the result of the scaffold call that followed: S, sc_lay_offs
 * and sc_layout (sc_flags is not read); sigax_gapfill_opts {flags = 0, k, min_count, slack, max_fill, reserved = 0}.
 * Preconditions: 8 <= k <= 128, min_count >= 1, slack < 2^31, max_fill < 2^31; anything else is SIGAX_E_ARG.
 *
 * count(w) = occ(w) + occ(revcomp(w)) on the forward index: exactly sigax_match_* with SIGAX_RC, so a reverse-palindromic w
 * counts twice.  Bytes outside upper-case ACGT rank as '$', so no k-mer reaches across a read's end.
 *
 * Placements.  P = sc_lay_offs[S] (0 when S = 0).  Placement p < P belongs to scaffold s(p), the largest s < S with
 * sc_lay_offs[s] <= p as a bisection finds it (lo = 0, hi = S; while hi - lo > 1: mid = (lo + hi) / 2, lo = mid if
 * sc_lay_offs[mid] <= p, else hi = mid; at most 32 steps).  Its unitig is u = sc_layout[p].read.  The placement is BAD iff
 * u >= nu, seq_offs[u+1] < seq_offs[u] or seq_offs[u+1] > useqs_bytes (no scaffold call makes one); bases(p) = seq_offs[u+1] -
 * seq_offs[u], and 0 for a bad placement.  All arithmetic is modulo 2^64.
 *
 * Gaps.  A gap is a pair of consecutive placements (p, p+1), p+1 < P, with s(p) == s(p+1).  The closing join of a circular
 * scaffold is no pair of placements: it is not a gap and stays as it is.  L = the bases of placement p's unitig as placed:
 * reverse-complemented with SIGAX_PLACED_REV (A<->T, C<->G), other bytes as they are; R = the same for p+1.  G = offset[p+1] -
 * offset[p] - bases(p), in u64.  Gaps are numbered in placement order, which is scaffold order, then placement order.
 *
 * Class of a gap: the first of these that applies.
 *   MALFORMED     placement p or p+1 is bad.
 *   SHORT         bases(L) < k or bases(R) < k.
 *   NON_ACGT      the last k bytes of L or the first k bytes of R hold a byte outside ACGT.
 *   FAR           G > max_fill.
 *   NO_ROOM       the walk scratch is too small.  A gap that comes this far needs G + slack bytes of it; its bytes begin where
 *                 the bytes of the gaps before it that came this far end, and it is NO_ROOM iff its own end lies beyond
 *                 max_walk_bases.  It stays as laid.
 *   otherwise     the outcome of the walks below.
 *
 * Walk(src, dst, limit).  Start with w = src.  For t = 1 .. limit: cand = {b in A, C, G, T : count(w[1:] + b) >= min_count}.
 * |cand| = 0 gives DEAD_END; |cand| >= 2 gives BRANCH; otherwise append b, set w = w[1:] + b, and if w == dst the walk has
 * REACHED at t and stops.  No reach after `limit` steps gives TOO_LONG.  limit = k + G + slack.
 * A walk that REACHED at step t: t < k gives OVERLAP (the unitigs overlap by k - t bases by this walk).  Otherwise f = t - k;
 * f + slack < G gives OFF_ESTIMATE; otherwise FILLED with the first f appended bases.  f = 0 is a legal fill.
 * The forward walk is Walk(last k of L, first k of R).  If and only if its outcome is DEAD_END, BRANCH or TOO_LONG the reverse
 * walk runs: Walk(revcomp(first k of R), revcomp(last k of L)); its fill is reverse-complemented.  The gap is FILLED if either
 * walk filled it -- forward wins, and the direction is recorded -- otherwise its class is the forward walk's outcome.
 *
 * Output: the scaffold tables again, every filled gap's N replaced by its fill and every other gap left as laid: sc_offs'
 * u64[S + 1], sc_layout' (the placements with their new offsets), sseqs' (N wherever neither a unitig nor a fill lies); sc_lay_offs
 * and sc_flags do not change and are not rewritten.  With D(p) = the sum of (fill - G) over the filled gaps before placement p:
 * offset'[p] = offset[p] + D(p) - D(h), h = sc_lay_offs[s(p)] taken as P when above it; scaffold s has offset'[last] + bases(last)
 * bases over its last placement, 0 without one.  One sigax_gap per gap in gap order: scaffold, left and right (unitig ids), laid
 * (G, saturated at 2^32 - 1), fill (bases; 0 unless FILLED), cls, fwd and rev (the two walks' outcomes: a class code, or
 * SIGAX_GAP_NOT_RUN), dir (0 forward, 1 reverse; 0 unless FILLED), offset (where the gap starts in its new scaffold).
 * status24 = 24 u64, written (not added to): 0 gaps; 1 + c gaps of class c for the eleven SIGAX_GAP_* codes (1 FILLED .. 11
 * MALFORMED); 12 filled forward, 13 filled in reverse, 14 fill bases, 15 N bases left in gaps, 16 scaffold bases of the new
 * tables, 17 extension steps made, 18 k-mer lookups made (8 per step), 19 rank-table sectors asked for (a diagnostic: the only
 * entry that depends on the index's tables), 20 = 1 when status[16] > sseqs_capacity: the bases were not written for lack of
 * room, 21 = 1 when any gap is NO_ROOM, 22 scaffolds S, 23 = 0.  No other result depends on scheduling or on the tables.
 *
 * sigax_gapfill_device: every buffer in device memory, asynchronous on `stream`, allocates nothing, never waits for the
 * device.  d_n_unitigs and d_n_scaffolds point at u64 ON THE DEVICE -- entry 0 of the unitig call's and of the scaffold call's
 * status block -- so the call can be enqueued straight behind sigax_scaffold_device; a count above max_unitigs is taken as
 * max_unitigs, and sc_lay_offs[S] likewise.  d_seq_offs and d_sc_lay_offs u64[max_unitigs + 1], d_sc_layout
 * sigax_placement[max_unitigs], d_useqs useqs_bytes bytes: no byte at or beyond them is read.  d_sc_offs u64[max_unitigs + 1],
 * d_sc_layout_out sigax_placement[max_unitigs], d_gaps sigax_gap[max_unitigs]; entries beyond S, P and the gaps are not
 * written.  d_sseqs sseqs_capacity bytes, or NULL with capacity 0; the bases are written only if status24[16] <=
 * sseqs_capacity.  d_work = sigax_gapfill_workspace(max_unitigs, max_walk_bases) bytes (244 per unitig, and the walk
 * scratch).  d_useqs, d_sseqs, d_sc_layout, d_sc_layout_out, d_gaps and d_work 16-byte aligned, every other buffer 8-byte
 * aligned; d_sc_layout_out must not overlap d_sc_layout.  A NULL where a buffer is required, a misaligned buffer, a short
 * workspace, bad options, max_unitigs >= 2^31, max_walk_bases or sseqs_capacity >= 2^43: SIGAX_E_ARG with the argument named
 * in sigax_last_error().  max_unitigs = 0: SIGAX_OK, status zeros, d_sc_offs[0] = 0 where given.  Whatever the tables hold --
 * offsets that do not ascend, unitig ids beyond the tables, a layout that claims more bases than useqs has -- nothing outside
 * the buffers is touched, and every loop has a bound the host knows: a bisection 32 steps, a walk k + max_fill + slack steps of
 * k symbols, at most two walks per gap. */
#define SIGAX_GAP_FILLED       0u
#define SIGAX_GAP_SHORT        1u
#define SIGAX_GAP_NON_ACGT     2u
#define SIGAX_GAP_FAR          3u
#define SIGAX_GAP_NO_ROOM      4u
#define SIGAX_GAP_DEAD_END     5u
#define SIGAX_GAP_BRANCH       6u
#define SIGAX_GAP_TOO_LONG     7u
#define SIGAX_GAP_OVERLAP      8u
#define SIGAX_GAP_OFF_ESTIMATE 9u
#define SIGAX_GAP_MALFORMED    10u
#define SIGAX_GAP_NOT_RUN      255u   /* sigax_gap.fwd / .rev: the walk was not made */
#define SIGAX_GAPFILL_AUTO     0xFFFFFFFFFFFFFFFFull  /* sigax_gapfill_host: size the walk scratch from the layout */
typedef struct sigax_gapfill_opts { uint32_t flags, k, min_count, slack, max_fill, reserved; } sigax_gapfill_opts;
typedef struct sigax_gap {
  uint32_t scaffold, left, right, laid;
  uint32_t fill;
  uint8_t  cls, fwd, rev, dir;
  uint64_t offset;
} sigax_gap; /* 32 bytes */
int  sigax_gapfill_workspace(uint64_t max_unitigs, uint64_t max_walk_bases, uint64_t* bytes);  /* host arithmetic only */
int  sigax_gapfill_device(sigax_index*, const void* d_n_unitigs, uint64_t max_unitigs, const void* d_seq_offs, const void* d_useqs,
                          uint64_t useqs_bytes, const void* d_n_scaffolds, const void* d_sc_lay_offs, const sigax_placement* d_sc_layout,
                          const sigax_gapfill_opts* opts, void* d_sc_offs, sigax_placement* d_sc_layout_out, void* d_sseqs,
                          uint64_t sseqs_capacity, sigax_gap* d_gaps, void* d_status24, void* d_work, uint64_t work_bytes,
                          uint64_t max_walk_bases, void* stream);
/* Host buffers, synchronous.  seq_offs u64[n_unitigs + 1], useqs seq_offs[n_unitigs] bytes, sc_lay_offs u64[n_scaffolds + 1],
 * sc_layout sigax_placement[sc_lay_offs[n_scaffolds]]; n_scaffolds or sc_lay_offs[n_scaffolds] above n_unitigs: SIGAX_E_ARG.
 * max_walk_bases = SIGAX_GAPFILL_AUTO sizes the walk scratch from the layout, so that no gap is NO_ROOM.  It runs the walks
 * and the layout, reads the total, then writes the bases into a buffer of exactly that size: status24[20] is 0.  *sc_offs
 * u64[n_scaffolds + 1], *sc_layout_out sigax_placement[placements], *sseqs status24[16] bytes (pass sseqs = NULL for the tables
 * alone), *gaps sigax_gap[*n_gaps]; all malloc'd, release with sigax_free. */
int  sigax_gapfill_host(sigax_index*, uint64_t n_unitigs, const uint64_t* seq_offs, const char* useqs, uint64_t n_scaffolds,
                        const uint64_t* sc_lay_offs, const sigax_placement* sc_layout, const sigax_gapfill_opts* opts,
                        uint64_t max_walk_bases, uint64_t** sc_offs, sigax_placement** sc_layout_out, char** sseqs, sigax_gap** gaps,
                        uint64_t* n_gaps, uint64_t status24[24]);
/* ---- `siga unitig --scaffold --join-overlaps`: overlapping scaffold neighbours written as one sequence (csrc/sigax_join.hip) ------
 * Two unitigs that end at a fork of the overlap graph usually share the overlap that forked.  The scaffolder estimates a negative
 * gap there, clamps it to min_gap and lays N between two sequences that run into each other; a k-mer walk cannot close such a
 * gap, because its goal lies behind its start.  This pass looks for the overlap itself: where exactly one length v makes the
 * left neighbour's last v bases the right neighbour's first v, and the reads support the sequence across the junction, the N and
 * one copy of the overlap go.  The reference has no such step; the rules are this library's own.  DESIGN.md 9l; the serial
 * restatement the tests hold this against is tests/join_cases.py::expected_join.
 *
 * Input: an open index (the forward strand is enough, and it is the only one read: no result depends on which tables the
 * index holds); nu and seq_offs of a unitig call, read for unitig lengths only; S, sc_offs, sc_lay_offs, sc_layout and sseqs
 * (sseqs_bytes bytes) of a scaffold or gapfill call; sigax_join_opts {flags = 0, min_overlap, max_overlap, slack, k, min_count,
 * reserved = 0}.  Preconditions: 8 <= min_overlap <= max_overlap <= 4096, slack < 2^31, 8 <= k <= 128, min_count >= 1; anything
 * else is SIGAX_E_ARG.  All arithmetic is modulo 2^64 unless it says otherwise.
 *
 * Placements, P and the scaffold s(p) of placement p (the 32-step bisection) are the gapfill block's.  u = sc_layout[p].read,
 * len(s) = sc_offs[s+1] - sc_offs[s].  Placement p is BAD iff u >= nu; seq_offs[u+1] < seq_offs[u]; sc_offs[s+1] < sc_offs[s];
 * sc_offs[s+1] > sseqs_bytes; or offset[p] + bases(p) > len(s) without wrapping, that is offset[p] > len(s) or bases(p) > len(s) -
 * offset[p].  bases(p) = seq_offs[u+1] - seq_offs[u], and 0 for a bad placement.  The bases of a placement are read from the
 * input sseqs as placed: X(p) = sseqs[sc_offs[s] + offset[p] .. + bases(p)).  No orientation is handled, useqs is not read,
 * and a fill that gapfill wrote stays.
 *
 * Gaps are the gapfill block's: consecutive placements (p, p+1) of one scaffold, numbered in placement order; a ring's closing
 * join is no gap.  G = offset[p+1] - offset[p] - bases(p) in u64, L = X(p), R = X(p+1).
 *
 * Class of a gap: the first of these that applies.
 *   MALFORMED    placement p or p+1 is bad.
 *   CLOSED       G = 0.
 *   FAR          G > slack.  This covers the wrapped G of neighbours that already overlap, so a second call over the output of a
 *                first joins nothing.
 *   CLOSED       one of the gap's G bytes sseqs[sc_offs[s] + offset[p] + bases(p) .. + G) is not 'N': a fill.  (At most slack
 *                bytes are read.)
 *   SHORT        hi < lo, where lo = min_overlap and hi = min(max_overlap, |L| - 1, |R| - 1), an empty L or R giving hi < lo.
 *   otherwise    the outcome of the match.
 *
 * Match.  match(v) holds iff the last v bytes of L equal the first v bytes of R byte for byte and every one of them is upper-case
 * A, C, G or T.  M = {v in [lo, hi] : match(v)}.  |M| = 0 gives NONE; |M| >= 2 gives AMBIGUOUS (tandem repeats and homopolymer
 * ends: the laid estimate is a clamp and cannot choose).  With one v the join is tested for read support over J = L ++ R[v:]:
 * the windows across the junction are the k-byte windows of J that lie neither wholly in L nor wholly in R, those that start
 * at s in [|L| - k + 1, |L| - v - 1] clipped to [0, |J| - k] -- none when v >= k - 1, since every k-mer of J is then in L or
 * in R.  count(w) is the gapfill block's, occ(w) + occ(revcomp(w)); a window with a byte outside ACGT counts 0.  A window with
 * count < min_count gives UNSUPPORTED, otherwise the gap is JOINED.
 *
 * Output.  For a JOINED gap the G bytes of N and the first v bytes of R go.  With E(p) = the sum of G + v over the joined gaps
 * (q, q+1), q < p, and h = sc_lay_offs[s(p)] taken as P when above it: offset'[p] = offset[p] - (E(p) - E(h)).  Scaffold s has
 * len(s) - (E(e) - E(h)) bases, e = sc_lay_offs[s+1] clamped likewise, and len(s) when e <= h.  The new bases are a compaction
 * of the input sseqs: per joined gap the old bytes [offset[p+1] - G, offset[p+1] + v) of its scaffold are deleted, out[x] =
 * in[x + the bytes deleted before x].  Where joins chain so closely that v1 + v2 > |R1| this is still well defined, since
 * deleted bytes equal kept ones.  sc_lay_offs and sc_flags are not rewritten.  One 32-byte sigax_join per gap in gap order:
 * scaffold, left and right (unitig ids), laid (G, saturated at 2^32 - 1), overlap (v; 0 unless JOINED or UNSUPPORTED), cls,
 * matches (|M|, saturated at 255), windows (those the support test had, max(0, k - v - 1) after the clip, whether or not an
 * early one failed; 0 unless JOINED or UNSUPPORTED), offset (offset'[p+1] of a JOINED gap, else offset'[p] + bases(p)).
 * status16 = 16 u64, written (not added to): 0 gaps; 1 + c gaps of class c for the eight SIGAX_JOIN_* codes (1 JOINED .. 8
 * MALFORMED); 9 overlap bases removed; 10 N removed; 11 scaffold bases of the new tables; 12 candidate overlaps tested, hi - lo +
 * 1 over the gaps that came to the match; 13 junction windows, as in the records; 14 = 1 when status[11] > sseqs_capacity: the
 * bases were not written for lack of room; 15 scaffolds S.  No result depends on scheduling or on the index's tables.
 *
 * sigax_join_device: every buffer in device memory, asynchronous on `stream`, allocates nothing, never waits for the device.
 * d_n_unitigs and d_n_scaffolds point at u64 ON THE DEVICE, so the call can be enqueued straight behind sigax_scaffold_device
 * or sigax_gapfill_device; a count above max_unitigs is taken as max_unitigs, and sc_lay_offs[S] likewise.  d_seq_offs,
 * d_sc_offs and d_sc_lay_offs u64[max_unitigs + 1], d_sc_layout sigax_placement[max_unitigs], d_sseqs sseqs_bytes bytes: no
 * byte at or beyond them is read.  d_sc_offs_out u64[max_unitigs + 1], d_sc_layout_out sigax_placement[max_unitigs], d_joins
 * sigax_join[max_unitigs]; entries beyond S, P and the gaps are not written.  d_sseqs_out sseqs_capacity bytes, or NULL with
 * capacity 0; the bases are written only if status16[11] <= sseqs_capacity.  d_work = sigax_join_workspace(max_unitigs) bytes
 * (116 per unitig).  d_sseqs, d_sseqs_out, d_sc_layout, d_sc_layout_out, d_joins and d_work 16-byte aligned, every other buffer
 * 8-byte aligned; d_sc_offs_out, d_sc_layout_out and d_sseqs_out must not overlap d_sc_offs, d_sc_layout and d_sseqs.  A NULL
 * where a buffer is required, a misaligned or overlapping buffer, a short workspace, bad options, max_unitigs >= 2^31,
 * sseqs_bytes or sseqs_capacity >= 2^43: SIGAX_E_ARG with the argument named in sigax_last_error().  max_unitigs = 0: SIGAX_OK,
 * status zeros, d_sc_offs_out[0] = 0 where given.  Whatever the tables hold, nothing outside the buffers is touched, and every
 * loop has a bound the host knows: a bisection 32 steps, the fill test slack bytes, the match max_overlap candidates of
 * max_overlap bases, the support test k - 2 windows of k symbols. */
#define SIGAX_JOIN_JOINED      0u
#define SIGAX_JOIN_CLOSED      1u
#define SIGAX_JOIN_FAR         2u
#define SIGAX_JOIN_SHORT       3u
#define SIGAX_JOIN_NONE        4u
#define SIGAX_JOIN_AMBIGUOUS   5u
#define SIGAX_JOIN_UNSUPPORTED 6u
#define SIGAX_JOIN_MALFORMED   7u
typedef struct sigax_join_opts { uint32_t flags, min_overlap, max_overlap, slack, k, min_count, reserved; } sigax_join_opts;
typedef struct sigax_join {
  uint32_t scaffold, left, right, laid;
  uint32_t overlap;
  uint8_t  cls, matches;
  uint16_t windows;
  uint64_t offset;
} sigax_join; /* 32 bytes */
int  sigax_join_workspace(uint64_t max_unitigs, uint64_t* bytes);  /* host arithmetic only */
int  sigax_join_device(sigax_index*, const void* d_n_unitigs, uint64_t max_unitigs, const void* d_seq_offs, const void* d_n_scaffolds,
                       const void* d_sc_offs, const void* d_sc_lay_offs, const sigax_placement* d_sc_layout, const void* d_sseqs,
                       uint64_t sseqs_bytes, const sigax_join_opts* opts, void* d_sc_offs_out, sigax_placement* d_sc_layout_out,
                       void* d_sseqs_out, uint64_t sseqs_capacity, sigax_join* d_joins, void* d_status16, void* d_work, uint64_t work_bytes,
                       void* stream);
/* Host buffers, synchronous.  seq_offs u64[n_unitigs + 1], sc_offs and sc_lay_offs u64[n_scaffolds + 1], sc_layout
 * sigax_placement[sc_lay_offs[n_scaffolds]], sseqs sc_offs[n_scaffolds] bytes; n_scaffolds or sc_lay_offs[n_scaffolds] above
 * n_unitigs: SIGAX_E_ARG.  It runs the tables, reads the total, then writes the bases into a buffer of exactly that size:
 * status16[14] is 0.  *sc_offs_out u64[n_scaffolds + 1], *sc_layout_out sigax_placement[placements], *sseqs_out status16[11]
 * bytes (pass sseqs_out = NULL for the tables alone), *joins sigax_join[*n_joins]; all malloc'd, release with sigax_free. */
int  sigax_join_host(sigax_index*, uint64_t n_unitigs, const uint64_t* seq_offs, uint64_t n_scaffolds, const uint64_t* sc_offs,
                     const uint64_t* sc_lay_offs, const sigax_placement* sc_layout, const char* sseqs, const sigax_join_opts* opts,
                     uint64_t** sc_offs_out, sigax_placement** sc_layout_out, char** sseqs_out, sigax_join** joins, uint64_t* n_joins,
                     uint64_t status16[16]);
/* ---- `siga unitig --scaffold --join-overlaps --join-mismatches`: ends that nearly agree (csrc/sigax_join.hip) -------------------------
 * On reads with errors a unitig's last read often carries a substitution in the stretch no other read of its chain covers, so the
 * two copies of an overlap differ in a base or two and the byte-exact match of the block above finds nothing.  This pass accepts,
 * where no length matches exactly, the one length whose two ends differ in a few bases, takes at each differing base the one the
 * reads support, tests the whole junction for read support and writes the consensus.  The rules are this library's own.
 * DESIGN.md 9m; the serial restatement is tests/join_approx_cases.py::expected_join_approx.
 *
 * Input and preconditions are sigax_join_*'s, with sigax_join_approx_opts {flags = 0, min_overlap, max_overlap, slack, k,
 * min_count, max_mismatches, mismatch_permille, reserved = 0}, 0 <= max_mismatches <= 16, 1 <= mismatch_permille <= 250; anything
 * else is SIGAX_E_ARG.  Placements, gaps, G, L, R, lo, hi and the classes MALFORMED, CLOSED, FAR and SHORT are the block above's.
 *
 * 1. Exact first.  M0 is the block above's M.  If M0 is not empty, the gap's class, record, support test and output are exactly
 *    the block above's and mm[g] = 0: no gap that the exact pass classes as anything but NONE changes.  With max_mismatches = 0
 *    the call equals sigax_join_* in every table, base, record and status[0..15]; mm is zeros and status[16..23] are zero.
 * 2. Second match, only for |M0| = 0 and max_mismatches >= 1.  hi' = min(hi, |L| / 2, |R| / 2) (integer division: the patches of
 *    rule 5 then land on disjoint bytes when a unitig is joined on both sides).  d(v) = the number of j in [0, v) with
 *    L[|L| - v + j] != R[j]; all 2 v bytes must be upper-case ACGT, else v is out.  B(v) = min(max_mismatches, v *
 *    mismatch_permille / 1000), in u64, the division rounded down.  M1 = {v in [lo, hi'] : d(v) <= B(v)}.  |M1| = 0 gives NONE
 *    with matches = 0; |M1| >= 2 gives AMBIGUOUS with matches = min(|M1|, 255); one v goes on with matches = 1, overlap = v and
 *    its columns j_0 < ... < j_(m-1), m = d(v), 1 <= m <= 16.
 * 3. Choice.  J^L = L ++ R[v:] and J^R = L[:|L| - v] ++ R have the same length |J| and differ in the m columns only.  |J| < k
 *    gives UNSUPPORTED with windows = 0 and taken_right = 0.  Column i lies at x_i = |L| - v + j_i; its window starts at w_i =
 *    min(max(x_i, k / 2) - k / 2, |J| - k).  c_L = count(J^L[w_i .. w_i + k)), c_R likewise over J^R; count is the gapfill
 *    block's (both strands, 0 for a window with a byte outside ACGT).  The column takes R's base iff c_R > c_L, else L's.
 *    taken_right is the number that took R's.  J* is J^L with those columns replaced.
 * 4. Support.  Every k-window of J* that starts in [max(0, |L| - v - k + 1), min(|L| - 1, |J| - k)] -- every window that touches
 *    the overlap or crosses the junction, at most v + k - 1 <= 4223 -- must have count >= min_count.  windows is that number
 *    whether or not an early one failed.  A window below min_count gives UNSUPPORTED, otherwise the gap is JOINED.  This is
 *    stricter than the exact join's test on purpose: bytes are being changed.
 * 5. Output.  Tables and compaction are the block above's with this v.  Then for each approximately JOINED gap (p, p+1) of
 *    scaffold s and each column that took R's base: out[sc_offs'[s] + offset'[p+1] + j_i] = R[j_i], R read from the input.  The
 *    patches are written only where the bases are (status[14] = 0).  By the half rule no two patches, and no patch and deletion
 *    of a neighbouring approximate join, meet.  The block above's sentence "deleted bytes equal kept ones" holds for exact joins
 *    only: an approximate join deletes R's copy of the overlap and keeps L's, patched.
 *
 * One sigax_join per gap as above, plus mm[g] = mismatches | taken_right << 8 | (approximate ? 1 << 16 : 0) for a gap that went on
 * from the second match with one v (JOINED or UNSUPPORTED), else 0.  status24: 0..15 as status16; 16 gaps JOINED through an
 * approximate match; 17 their mismatch columns; 18 columns written from the right neighbour; 19 approximate candidates tested,
 * max(0, hi' - lo + 1) over the gaps that came to the second match; 20 choice windows looked up, 2 m over the gaps that came to
 * the choice; 21..23 zero.  No result depends on lane order, scheduling, the index's optional tables or narrow/wide positions.
 *
 * sigax_join_approx_device / _host: the buffer rules, alignment, limits and the "never waits, allocates nothing" contract are
 * sigax_join_device's / _host's.  Added: d_mm u32[max_unitigs], 4-byte aligned, entries beyond the gaps not written; d_status24
 * 24 u64; d_work = sigax_join_approx_workspace(max_unitigs) bytes (156 per unitig).  *mm u32[*n_joins], malloc'd.  Added loop
 * bounds: the second match max_overlap candidates of max_overlap bases, the choice 32 windows, the support test v + k - 1
 * windows of k symbols, each base at most 16 column look-ups. */
typedef struct sigax_join_approx_opts {
  uint32_t flags, min_overlap, max_overlap, slack, k, min_count; /* as sigax_join_opts; flags = 0 */
  uint32_t max_mismatches;                                      /* 0 .. 16 */
  uint32_t mismatch_permille;                                   /* 1 .. 250 */
  uint32_t reserved;                                            /* 0 */
} sigax_join_approx_opts; /* 36 bytes */
int  sigax_join_approx_workspace(uint64_t max_unitigs, uint64_t* bytes);  /* host arithmetic only */
int  sigax_join_approx_device(sigax_index*, const void* d_n_unitigs, uint64_t max_unitigs, const void* d_seq_offs, const void* d_n_scaffolds,
                              const void* d_sc_offs, const void* d_sc_lay_offs, const sigax_placement* d_sc_layout, const void* d_sseqs,
                              uint64_t sseqs_bytes, const sigax_join_approx_opts* opts, void* d_sc_offs_out, sigax_placement* d_sc_layout_out,
                              void* d_sseqs_out, uint64_t sseqs_capacity, sigax_join* d_joins, uint32_t* d_mm, void* d_status24, void* d_work,
                              uint64_t work_bytes, void* stream);
int  sigax_join_approx_host(sigax_index*, uint64_t n_unitigs, const uint64_t* seq_offs, uint64_t n_scaffolds, const uint64_t* sc_offs,
                            const uint64_t* sc_lay_offs, const sigax_placement* sc_layout, const char* sseqs, const sigax_join_approx_opts* opts,
                            uint64_t** sc_offs_out, sigax_placement** sc_layout_out, char** sseqs_out, sigax_join** joins, uint64_t* n_joins,
                            uint32_t** mm, uint64_t status24[24]);
/* OverlapBuilder::overlap for a batch (host buffers in, host buffers out).  seqs = concatenated read bytes,
 * offs[n_reads+1]; read r of the batch is read `read_base + r` of the indexed set (only used for edges).
 * The result is filled with malloc'd arrays; release with sigax_result_free. */
int  sigax_overlap_batch(sigax_index*, const char* seqs, const uint64_t* offs, uint32_t n_reads, uint32_t read_base,
                         uint32_t min_overlap, uint32_t flags, sigax_result* out);
void sigax_result_free(sigax_result*);

/* Device-resident pipeline (what a batching runtime and bench.py use). */
int  sigax_batch_create(sigax_index*, uint32_t max_reads, uint64_t max_bases, uint32_t max_read_len, sigax_batch** out);
void sigax_batch_destroy(sigax_batch*);
/* Copy reads to the device (async on `stream`, a hipStream_t or NULL). */
int  sigax_batch_upload(sigax_batch*, const char* seqs, const uint64_t* offs, uint32_t n_reads, void* stream);
/* Use reads that already sit in device memory (d_seqs bytes, d_offs u64[n_reads+1]); max_len = longest read. */
int  sigax_batch_set_device_reads(sigax_batch*, const void* d_seqs, const void* d_offs, uint32_t n_reads,
                                  uint64_t n_bases, uint32_t max_len);
/* The batch's reads need not be consecutive reads of the indexed set: ids[r] = read r's place in the index's read table
 * (what an ED record's query field then says; blocks and substring flags do not depend on it).  This is what lets a caller
 * shard its reads by anything but position in the file -- e.g. by a locality key, so that one GPU's reads cover one part
 * of the genome deeply instead of all of it thinly (bench.py --gpus N, siga_amd/sharding.py).  The ids stay with the batch
 * object for every later run until set again; NULL = read_base + r as before.  A run whose reads are not as many as the ids
 * fails with SIGAX_E_STATE; an id beyond the indexed reads fails the upload (host form) or the run's
 * sigax_batch_finish (device form) with SIGAX_E_ARG, without touching memory outside the tables.
 * No counterpart in the reference (one process, reads in file order: src/overlap_builder.cpp:1113-1182 takes the id from
 * the read's position in the file). */
int  sigax_batch_upload_read_ids(sigax_batch*, const uint32_t* ids, uint32_t n_reads, void* stream);
int  sigax_batch_set_device_read_ids(sigax_batch*, const void* d_ids, uint32_t n_reads);
/* Locality keys of reads in device memory (d_seqs bytes, d_offs u64[n_reads+1]) into d_keys u64[n_reads], queued on `stream`
 * (a hipStream_t or NULL): key = min over the read's 16-mers of hash(canonical 16-mer) << 16 | start offset (csrc/sigax_keys.hip).
 * Reads of one stretch of the genome, either strand, get neighbouring keys: a caller that sorts its reads by key and gives each
 * GPU a contiguous range of that order (with sigax_batch_*_read_ids above) has every GPU walk a part of the index instead of
 * all of it.  Needs no index.  No counterpart in the reference. */
int  sigax_locality_keys(int device, const void* d_seqs, const void* d_offs, uint32_t n_reads, void* d_keys, void* stream);
/* How many sub-batches a run is cut into (0 = automatic).  With more than one, sub-batch i's filter/extract kernels run on
 * an internal stream beside sub-batch i+1's block finder (the first is VALU-bound, the second memory-request-bound). */
int  sigax_batch_set_subbatches(sigax_batch*, uint32_t n);
/* Enqueue the whole path: find -> filter/extract -> block offsets -> ordered blocks, or with SIGAX_EDGES the edge records.
 * Asynchronous.  The kernels run on three internal
 * streams owned by the index (finder, filter/extract, tail) and ordered against `stream`: work already on `stream` is
 * waited for, and `stream` waits for the run's last kernel.  Several batch objects of one index may be in flight at
 * once (each with its own `stream`): their finder launches queue behind each other, so batch k+1's finder starts beside
 * batch k's filter/extract tail.  A batch object must be finished before it is run again.
 * A run with SIGAX_EDGES makes its edge records straight from the blocks as filter/extract left them and does NOT put the
 * 80-byte blocks in order: block_offs, the substring flags and the edge records are its outputs, and the ordered blocks
 * are made the first time they are asked for (sigax_batch_device_outputs with d_blocks, sigax_batch_download).  A run
 * without SIGAX_EDGES orders its blocks in the run, as they are its result. */
int  sigax_batch_run(sigax_batch*, uint32_t read_base, uint32_t min_overlap, uint32_t flags, void* stream);
/* Wait for the stream, check arena overflow flags (growing arenas and re-running if needed), fill stats. */
int  sigax_batch_finish(sigax_batch*, void* stream, sigax_stats* stats);
/* Device pointers of the finished batch's outputs (valid until the next run on this batch).  Any of the four may be NULL.
 * After a run with SIGAX_EDGES a non-NULL d_blocks makes the call order the blocks first: one copy kernel on the index's tail
 * stream, which the call waits for -- the other three pointers cost nothing.  The first such call after a run (this one or
 * sigax_batch_download) does the copy; later ones return the same pointer at once.  Every sigax_batch_run, and every repeat
 * of the run inside sigax_batch_finish, starts over. */
int  sigax_batch_device_outputs(sigax_batch*, const sigax_block** d_blocks, const uint64_t** d_block_offs,
                                const uint8_t** d_substring, const sigax_edge** d_edges);
/* Everything to the host (malloc'd; release with sigax_result_free); orders the blocks as sigax_batch_device_outputs does. */
int  sigax_batch_download(sigax_batch*, sigax_result* out);
/* Only what the ASQG writer needs (OverlapPostProcess + Hit2OverlapConverter, src/overlap_builder.cpp:291-375): the
 * substring flags (n_reads bytes, caller's buffer, may be NULL) and the edge records (malloc'd; release with sigax_free). */
int  sigax_batch_download_edges(sigax_batch*, uint8_t* substring, sigax_edge** edges, uint64_t* n_edges);
/* Reads of up to max_read_len bases one batch object can take when `in_flight` batch objects share the device's free
 * memory now (the reference's threads x batch-size is a host notion; the device batch is sized from HBM). */
int  sigax_batch_size_hint(sigax_index*, uint32_t max_read_len, uint32_t min_overlap, uint32_t flags, uint32_t in_flight,
                           uint32_t* max_reads);
/* Device time of the kernels of the last finished run, measured with HIP events on the streams they were launched on,
 * summed over the run's sub-batch launches: ms[0] find, ms[1] filter/extract (32- and 64-lane launches),
 * ms[2] filter/extract (general), ms[3] block scan + edge stage pass (without SIGAX_EDGES: block scan + ordered copy),
 * ms[4] edge scan + emit pass (without SIGAX_EDGES: 0).  *n_sub = finder launches of the run (sub-batches, times
 * two when the finder runs once per strand's two-step table); the other kernels run once per sub-batch. */
int  sigax_batch_kernel_ms(sigax_batch*, float ms[5], uint32_t* n_sub);

/* How the last finished run of a batch object was carried out: what a caller needs to turn sigax_stats and
 * sigax_batch_kernel_ms into requests and bytes per launch without re-deriving the library's choices. */
typedef struct sigax_run_info {
  uint32_t n_sub;         /* sub-batches of the run */
  uint32_t find_per_sub;  /* finder launches per sub-batch (2: one per strand's table) */
  uint32_t two_step;      /* the finder gathered 128-byte two-step lines (two backward steps each); 0: 64-byte granules */
  uint32_t coop;          /* ... cooperatively through LDS (indexes of 2^31 symbols and more) */
  uint32_t read_order;    /* the finder walked the batch in its locality order */
  uint32_t cap;           /* candidate slots per chain of the run */
  uint32_t worst_cap;     /* ... had they been sized for the worst case (one per overlap length + 1) */
  uint32_t row_bits;      /* bits per entry of the index's row tables, 0 = none */
  uint32_t row_syms;      /* symbols an entry carries */
  uint32_t row_text;      /* the stretch text exists (extension rounds are read off it) */
  uint32_t row_direct;    /* ... reached through the direct maps (8 bytes per read) instead of a row table */
  uint32_t deep_k;        /* chains started from the deep start table with this K (0: from the 12-mer table or the first symbol) */
  uint64_t arena_bytes;   /* candidate arena of this batch object */
  uint64_t workspace_bytes; /* all device buffers of this batch object */
  uint64_t reruns;        /* runs of this batch object repeated so far because an arena was too small */
  float    order_ms;      /* device time of the locality ordering inside this run (0: the order of an earlier run was reused) */
} sigax_run_info;
int  sigax_batch_run_info(sigax_batch*, sigax_run_info* out);

/* ---- Multi-GPU: the one exchange step -----------------------------------------------------------------
 * Reads shard across the GPUs of a node and the index is replicated (sigax_index_clone), so the path has exactly one
 * exchange: the variable-length gather of a step's fixed-size edge records to one rank -- what replaces the serial
 * hits -> ASQG pass of src/overlap_builder.cpp:466-483 when one process drives each GPU.  Over RCCL (xGMI between the
 * MI355X of a node): ncclAllGather of the per-rank counts, then grouped ncclSend / ncclRecv of the 16-byte records.
 * Gathered in rank order.  Where every rank ran a contiguous range of the file's reads (rank r the r-th range) that is the
 * read order, the ED order of a one-GPU run; where the ranks ran key-range shards under their own ids
 * (sigax_batch_*_read_ids) it is a permutation of it, and the caller follows the gather with sigax_edges_restore_order
 * (below).  RCCL is bound at run time; without it these calls
 * fail with SIGAX_E_DEVICE and nothing else in the library is affected.  (The C++ host's `siga overlap --gpus N` drives
 * all GPUs from one process and copies each GPU's records to the host over that GPU's own PCIe link instead.) */
typedef struct sigax_comm sigax_comm;
#define SIGAX_COMM_ID_BYTES 128
/* rank 0 makes the id (ncclGetUniqueId) and ships it to the other ranks by whatever means the launcher has */
int  sigax_comm_unique_id(uint8_t id[SIGAX_COMM_ID_BYTES]);
/* collective over all `world` ranks (ncclCommInitRank), each on its own `device` */
int  sigax_comm_create(int device, int rank, int world, const uint8_t id[SIGAX_COMM_ID_BYTES], sigax_comm** out);
void sigax_comm_destroy(sigax_comm*);
/* The gather, two collectives.  sigax_gather_counts: every rank says how many records it holds; counts[world] (host)
 * receives all ranks' counts before the call returns (ncclAllGather + one host wait on `stream`), so that the root can size
 * its buffer.  sigax_gather_edges: with those counts, the transfer of the records is enqueued on `stream` (grouped ncclSend /
 * ncclRecv); d_local = this rank's counts[rank] records in device memory (e.g. sigax_batch_device_outputs' d_edges), on
 * `root` d_out (device, room for the sum of the counts) receives rank 0's records first; other ranks pass d_out = NULL. */
int  sigax_gather_counts(sigax_comm*, uint64_t n_local, uint64_t* counts, void* stream);
int  sigax_gather_edges(sigax_comm*, const sigax_edge* d_local, const uint64_t* counts, int root, sigax_edge* d_out,
                        void* stream);

/* ---- Read order of key-sharded edge records (csrc/sigax_order.hip) ---------------------------------------------------------
 * Batches that run their reads under their own ids emit their records in the batch's order of reads.  Every read is run in one
 * batch and a batch emits all records of one query contiguously, in hits order, so in the concatenation of the batches'
 * records every query owns one contiguous run, and the ED order of a one-batch run is the stable order of that list by
 * `query`.  No counterpart in the reference (one process, reads in file order: src/overlap_builder.cpp:466-483). */

/* bytes of device scratch sigax_edges_restore_order needs; host arithmetic only, no device touched */
int  sigax_edges_order_workspace(uint64_t n_edges, uint64_t n_reads, uint64_t* bytes);
/* d_in: n_edges records (at most 2^32), the concatenation of any number of batches' edge records in any batch order
 * (sigax_batch_device_outputs' d_edges, or sigax_gather_edges' d_out).
 * d_out: the same records stably ordered by query = the ED order of a one-batch run over the n_reads indexed reads.
 * d_out must not overlap d_in; both and d_work are 16-byte aligned.
 * d_query_offs: NULL or u64[n_reads+1]: records of read q are d_out[offs[q] .. offs[q+1]).
 * d_status: 2 u64 of device memory, written (not added to):
 *   {records with query >= n_reads, runs beyond the first of a query}.
 *   When either is non-zero d_out's and d_query_offs' contents are unspecified; no memory outside the buffers is touched.
 * NULL where a buffer is required, overlapping buffers and a work_bytes below sigax_edges_order_workspace's are SIGAX_E_ARG.
 * n_edges = 0: SIGAX_OK, d_query_offs all zeros, status zeros (d_in, d_out and d_work may be NULL).
 * Asynchronous on `stream` (a hipStream_t or NULL); allocates nothing. */
int  sigax_edges_restore_order(int device, const sigax_edge* d_in, uint64_t n_edges, uint64_t n_reads,
                               sigax_edge* d_out, uint64_t* d_query_offs, void* d_work, uint64_t work_bytes,
                               void* d_status, void* stream);
/* host buffers in and out, synchronous; SIGAX_E_ARG with a text that names which of the two status counts was non-zero */
int  sigax_edges_restore_order_host(int device, const sigax_edge* in, uint64_t n_edges, uint64_t n_reads,
                                    sigax_edge* out, uint64_t* query_offs);
/* Per-read bytes of a batch (sigax_batch_device_outputs' d_substring) to their reads' places: d_out[d_ids[r]] = d_flags[r],
 * r < n; positions no id names keep their value; d_status: 1 u64 = ids >= n_reads (those are not written).  Asynchronous on
 * `stream`; allocates nothing. */
int  sigax_flags_by_read_id(int device, const uint8_t* d_flags, const uint32_t* d_ids, uint64_t n, uint64_t n_reads,
                            uint8_t* d_out, void* d_status, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SIGAX_H_ */
