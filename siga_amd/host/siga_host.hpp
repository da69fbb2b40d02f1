// siga_amd/host/siga_host.hpp -- host side of the drop-in: the reference's classes for this path, re-implemented
// over the C-ABI (include/sigax.h).  Same names, argument meaning and error behaviour as the reference so that a
// maintainer can swap them in: DNASeq / readers (src/kseq.h), FMIndex (src/fmindex.h, here a handle pair living
// on the GPU), SuffixArray + BWT writers (src/suffix_array.cpp, src/bwt.cpp), OverlapBuilder
// (src/overlap_builder.h:19-45), Utils::stem (src/utils.cpp:128-135).  One source file per object: reads.cpp (readers),
// strand_index.cpp (index builders and writers), overlap_builder.cpp (FMIndex, OverlapBuilder), correct_match.cpp
// (CorrectProcessor, Matcher), locate.cpp (Locator), kmer_spectrum.cpp (KmerSpectrum), unitig.cpp (Unitigger), pairs.cpp (its paired-end side), host_capi.cpp (the sigah_* C entry points); out_file.*, asqg_text.*, reads.hpp and
// host_util.hpp are internal to the library.
#ifndef SIGA_AMD_HOST_SIGA_HOST_HPP_
#define SIGA_AMD_HOST_SIGA_HOST_HPP_

#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "../../include/sigax.h"

namespace sigah {

// src/kseq.h: DNASeq
struct DNASeq {
  std::string name, comment, seq, quality;
};
typedef std::vector<DNASeq> DNASeqList;

// gz-aware line source (Utils::ifstream, src/utils.cpp:50-90; bz2 is not supported by this build)
class LineSource;

// DNASeqReader / FASTAReader / FASTQReader (src/kseq.h:60-150, src/kseq.cpp:127-228)
class DNASeqReader {
 public:
  static DNASeqReader* create(const std::string& path);  // DNASeqReaderFactory::create; nullptr on failure
  ~DNASeqReader();
  bool read(DNASeq& sequence);
  bool failed() const;  // the input could not be read to its end (corrupt .gz); read() then returned false early
  void reset();

 private:
  DNASeqReader();
  std::unique_ptr<LineSource> _src;
  bool _fastq;
  std::string _name;
};

enum { kSeqWithQuality = 1, kSeqWithComment = 2 };
bool ReadDNASequences(const std::string& file, DNASeqList& sequences, uint32_t flags = kSeqWithQuality | kSeqWithComment);

namespace Utils {
std::string stem(const std::string& filename);
}

// One strand's index as `siga index` writes it (src/indexer.cpp:80-104): RL-BWT + the full-read SA rows.
struct StrandIndex {
  std::vector<uint8_t> runs;   // RLUnit bytes (src/rlstring.h:10-63), 31-cap (src/bwt.cpp:17)
  std::vector<uint32_t> sai;   // read ids of the j==0 suffixes in SA order (src/suffix_array.cpp:17-44)
  uint64_t nStrings, nSymbols;
  bool writeBWT(const std::string& path) const;  // src/bwt.cpp:121-178
  bool writeSAI(const std::string& path) const;  // src/suffix_array.cpp:17-44
};

// SuffixArrayBuilder "sais2" + BWT(sa, reads) (src/suffix_array_builder.cpp:472-674, src/bwt.cpp:7-32)
// threads >= 2 selects a multi-threaded bucket sort (same suffix order), 1 the SA-IS
// own_sentinels: the suffix order of `siga index -a sais` (every read's own '$', ordered by read index) instead of the
// default "sais2" order (one shared '$', comparisons running on into the next read); host only, ACGT-only reads
bool BuildStrandIndex(const char* seqs, const uint64_t* offs, uint64_t nReads, bool reverse, StrandIndex* out,
                      std::string* error, unsigned threads = 1, bool own_sentinels = false);

// the same on the GPU (sigax_build_strand); *rc = the library's code (SIGAX_E_CAPACITY: use BuildStrandIndex)
bool BuildStrandIndexGPU(const char* seqs, const uint64_t* offs, uint64_t nReads, bool reverse, int device, StrandIndex* out,
                         std::string* error, int* rc = nullptr);

// FMIndex pair resident on a GPU (FMIndex::load x2, src/overlap.cpp:41-42)
class FMIndex {
 public:
  FMIndex() : _h(nullptr) {}
  ~FMIndex();
  static bool load(const std::string& prefix, FMIndex& fmi, int device = 0);
  static bool loadForward(const std::string& prefix, FMIndex& fmi, int device = 0);  // <prefix>.bwt alone (`siga correct`)
  static bool loadForwardSai(const std::string& prefix, FMIndex& fmi, int device = 0);  // <prefix>.bwt + <prefix>.sai (`siga locate`)
  sigax_index* handle() const { return _h; }
  uint64_t length() const;

 private:
  FMIndex(const FMIndex&);
  FMIndex& operator=(const FMIndex&);
  sigax_index* _h;
};

// src/overlap_builder.h:19-45.  The reference takes (fmi, rfmi); here one FMIndex object holds both strands.
class OverlapBuilder {
 public:
  OverlapBuilder(const FMIndex* fmi, const std::string& prefix = "default", bool irreducible = true, bool rc = true)
      : _fmi(fmi), _prefix(prefix), _irreducible(irreducible), _rc(rc), _gpus(1) {}
  // reads shard over `n` GPUs of the node, starting at the index's device; the index is replicated device to device
  void setGPUs(int n) { _gpus = n < 1 ? 1 : n; }
  // build() leaves the parsed reads with the builder instead of unmapping them (a CLI about to exit: its pages go with the process)
  void keepReads(bool on) { _keep_reads = on; }
  // parse `input` and rank its names now (host threads only), e.g. while FMIndex::load is busy on another thread;
  // the next build() of the same file uses the result
  void preload(const std::string& input, size_t threads = 1, long minOverlap = -1, const std::string& output = std::string()) const;

  // HT, VT (input order), ED (hits order) to `output` (gz when the name ends with .gz).  `threads` is accepted for
  // signature compatibility (the GPU replaces the OpenMP loop); `batch` = reads per device batch.
  bool build(const std::string& input, size_t minOverlap, const std::string& output, size_t threads = 1,
             size_t batch = 1000, size_t* processed = nullptr) const;

  // `siga rmdup` (src/overlap_builder.cpp:562-704): reads without an identical / reverse-complement-identical twin of
  // smaller name and that are no substring go to `output`, the others to `duplicates`, headers as the reference
  // writes them ("<name> <name> NumDuplicates=<n>" / "<name>,seqrank=<idx> <name> NumDuplicates=<n>").
  bool rmdup(const std::string& input, const std::string& output, const std::string& duplicates, size_t threads = 1,
             size_t* processed = nullptr) const;

  const std::string& error() const { return _error; }

 private:
  const FMIndex* _fmi;
  std::string _prefix;
  bool _irreducible;
  bool _rc;
  int _gpus;
  mutable std::string _error;
  struct Preloaded;
  mutable std::shared_ptr<Preloaded> _pre;
  bool _keep_reads = false;
};

// `siga overlap -e`: every overlap of at least min_overlap columns with at most error_permille mismatches per mille, without gaps,
// found by seeds and verified on the GPU (sigax_mmoverlap_batch; the rules in include/sigax.h).  No counterpart in the reference,
// whose finder is exact.  OverlapBuilder::build is not involved.  The index needs its forward .sai table and reads of ACGT only
// (FMIndex::loadForwardSai will do); `input` must be the reads it was built from.
// The records of that path, shared by `siga overlap -e` and `siga unitig -e`: open() builds the reference text (an index that
// cannot serve -- no forward .sai, reads with other bytes than ACGT -- is refused there, with the library's message), find() runs
// sigax_mmoverlap_batch over every read of the index and hands the records on as sigax_edge with the mismatch counts beside them.
class MismatchRecords {
 public:
  MismatchRecords() = default;
  MismatchRecords(const MismatchRecords&) = delete;
  MismatchRecords& operator=(const MismatchRecords&) = delete;
  ~MismatchRecords();
  bool open(const FMIndex& index, std::string* error);
  // containments given: the call asks for the containment records too (SIGAX_MMO_CONTAINMENTS) and splits them from the
  // dovetails; both keep their order.  status8[7] then counts both kinds.
  bool find(const FMIndex& index, const sigax_mmo_params& params, size_t n, unsigned threads, std::vector<sigax_edge>* edges,
            std::vector<uint32_t>* num_diff, std::vector<uint8_t>* contained, uint64_t status8[8], std::string* error,
            std::vector<sigax_mm_edge>* containments = nullptr);

 private:
  sigax_pile_ref* _ref = nullptr;
};

class MismatchOverlapper {
 public:
  static sigax_mmo_params defaults(uint32_t error_permille) {  // the CLI's
    sigax_mmo_params p;
    p.seed_length = 24; p.seed_stride = 12; p.max_seed_hits = 256; p.min_overlap = 45; p.error_permille = error_permille;
    p.max_candidates = 512; p.max_read_len = 0; p.flags = 0;
    return p;
  }
  explicit MismatchOverlapper(const sigax_mmo_params& params) : _params(params) {}
  // --containments FILE: one line per containment record in the records' order -- contained name, container name, the first
  // column of the container that the contained read covers, + or - (reverse-complemented in the container), mismatches; tabs
  void setContainments(const std::string& path) { _containments_path = path; }
  uint64_t containments() const { return _containments; }
  // HT, VT (input order, SS:i:1 where the read is contained in another or is a duplicate of a smaller name), ED (the records'
  // order: query, target, strand and end, length; the mismatches in the last column) to `output` (gz when the name ends with .gz).
  bool run(const FMIndex& index, const std::string& input, const std::string& output, size_t threads = 1) const;
  const std::string& error() const { return _error; }
  const uint64_t* status() const { return _status; }  // the status words of sigax_mmoverlap_batch
  uint64_t records() const { return _records; }

 private:
  sigax_mmo_params _params;
  mutable uint64_t _status[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  mutable uint64_t _records = 0, _containments = 0;
  std::string _containments_path;
  mutable std::string _error;
};

// src/correct_processor.h:25-42.  The k-mer algorithm is the reference's; its "overlap" algorithm is an empty stub there and the
// pile-up of include/sigax.h here (`siga correct -a overlap`).
class CorrectProcessor {
 public:
  struct Options {
    size_t kmerSize, kmerThreshold, kmerRounds, kmerCountOffset;  // -k -x -i -O, defaults src/correct_processor.h:15-20
    bool overlap;               // -a overlap: the fields below, and `rounds` for -i
    sigax_pile_params pile;     // --seed-length --seed-stride --max-seed-hits -m -e --conflict --min-depth --max-candidates
    size_t rounds;
    Options() : kmerSize(31), kmerThreshold(3), kmerRounds(10), kmerCountOffset(1), overlap(false), rounds(1) {
      pile.seed_length = 24; pile.seed_stride = 12; pile.max_seed_hits = 256; pile.min_overlap = 45; pile.error_permille = 40;
      pile.conflict = 5; pile.min_depth = 2; pile.max_candidates = 512; pile.max_read_len = 0; pile.reserved = 0;
    }
  };
  explicit CorrectProcessor(const Options& options) : _options(options) {}
  // k-mer: reads that became all-solid are written to `output` in the input's format (FASTA/FASTQ), the rest are dropped.
  // overlap: the valid reads (rule 7) are written, qualities unchanged; the index needs its .sai table (FMIndex::loadForwardSai)
  bool process(const FMIndex& index, const std::string& input, const std::string& output, size_t threads = 1,
               size_t* processed = nullptr) const;
  const std::string& error() const { return _error; }
  // overlap: the status words of sigax_pileup_batch added up over the batches, and the reads read and written
  const uint64_t* pileStatus() const { return _pileStatus; }
  uint64_t readsIn() const { return _readsIn; }
  uint64_t readsOut() const { return _readsOut; }

 private:
  mutable uint64_t _pileStatus[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  mutable uint64_t _readsIn = 0, _readsOut = 0;
  Options _options;
  mutable std::string _error;
};

// `siga match` (src/match.cpp:38-63): for every read of every input, how often it -- or, for a read of more than maxLength
// bases, its first and its last maxLength bases -- occurs in the indexed reads, both strands unless rc is false.
class Matcher {
 public:
  static const uint64_t kNoLimit = ~0ull;
  explicit Matcher(uint64_t maxLength = kNoLimit, bool rc = true) : _maxLength(maxLength), _rc(rc) {}
  // "VT\t0|1\t<name>\t<seq>\t<count>\n" lines in read order to `output` (empty: stdout).  The inputs are read in order; one
  // that cannot be read ends the run with what came before it written, as in the reference.  batchReads = reads per device
  // batch (0: from the device's free memory).
  bool run(const FMIndex& index, const std::vector<std::string>& inputs, const std::string& output = std::string(), size_t threads = 1,
           size_t batchReads = 0, size_t* processed = nullptr) const;
  const std::string& error() const { return _error; }

 private:
  uint64_t _maxLength;
  bool _rc;
  mutable std::string _error;
};

// `siga locate`: for every query of every input, where it occurs in the indexed reads -- read index (0-based position in the
// indexed set), offset and strand -- both strands unless rc is false.  No counterpart in the reference.  The index needs its
// .sai table (FMIndex::load or FMIndex::loadForwardSai) and reads of ACGT only: run() fails with the library's message otherwise.
class Locator {
 public:
  static const uint32_t kNoLimit = 0xFFFFFFFFu;  // the library's MAX_STRING_LEN: walks as long as the index's longest read
  explicit Locator(uint32_t maxHits = 1000, uint32_t maxLength = kNoLimit, bool rc = true) : _maxHits(maxHits), _maxLength(maxLength), _rc(rc) {}
  // Per query, in input order: "QT\t<name>\t<query length>\t<total>\t<listed>\n", then "HT\t<name>\t<read index>\t<offset>\t<+|->\n"
  // per listed hit in the library's order (sigax_locate_batch) to `output` (empty: stdout).  A query that is empty, holds a byte
  // outside ACGT or occurs more than maxHits times lists nothing; a hit whose walk was cut at maxLength prints "*" for its
  // read and offset.  The inputs are read in order; one that cannot be read ends the run with what came before it written.
  // batchQueries = queries per device batch (0: 2^18).
  bool run(const FMIndex& index, const std::vector<std::string>& inputs, const std::string& output = std::string(), size_t threads = 1,
           size_t batchQueries = 0, size_t* processed = nullptr) const {
    return run(index.handle(), inputs, output, threads, batchQueries, processed);
  }
  // the same over the library's handle (what a host without the FMIndex class holds)
  bool run(sigax_index* index, const std::vector<std::string>& inputs, const std::string& output = std::string(), size_t threads = 1,
           size_t batchQueries = 0, size_t* processed = nullptr) const;
  const std::string& error() const { return _error; }

 private:
  uint32_t _maxHits, _maxLength;
  bool _rc;
  mutable std::string _error;
};

// `siga unitig`: the first step of the reference's `siga assemble`, Bigraph::simplify (src/bigraph.cpp:341-414), on the GPU: the
// reads go through the overlap stages, their edge records stay records (no ASQG), and every unbranched chain of them becomes
// one unitig (sigax_unitigs_host; the rules in include/sigax.h).  With setTrim / setGraph / setRemoved also the loop that follows
// in assemble (TrimVisitor and simplify() in turn) and the graph between the unitigs (sigax_unitigs_trim_host); with setMaxOverlap
// also that loop's MaximumOverlapVisitor (sigax_unitigs_prune_host); with setChimeric also its ChimericVisitor
// (sigax_unitigs_chimeric_host); with setPairs also the insert size estimate of its paired-end mode and the links between
// unitig ends (sigax_unitigs_pairs_host).  One GPU.
class Unitigger {
 public:
  explicit Unitigger(bool irreducible = true, bool rc = true) : _irreducible(irreducible), _rc(rc), _unitigs(0), _bases(0), _merged(0), _cycles(0) {}
  // One FASTA record per unitig, in the library's numbering, to `fasta` (empty: stdout): ">unitig-<n> KC:i:<reads>", the tag
  // only when the unitig holds more than one read, " circular=<closing overlap>" behind it for a cycle, the bases on one line.
  // `layout` not empty: one line "unitig-<n>\t<read name>\t<+|->\t<offset>" per placement to that file.
  bool run(const FMIndex& index, const std::string& input, size_t minOverlap, const std::string& fasta = std::string(),
           const std::string& layout = std::string(), size_t threads = 1);
  // reads per overlap call (0: 2^20); the records do not depend on it
  void setPieceReads(size_t n) { _piece = n; }
  // Tip trimming as the reference's `assemble` does it (TrimVisitor and simplify() in turn, src/assembler.cpp:138-159): up to
  // `rounds` rounds (-x; 0, the default: none, and the output is the one without this call) remove every dead end and island
  // of at most minBranchLength bases (-n) and, with minBranchCoverage >= 0 (-C; -1: no such test), of low coverage
  // (sigax_unitigs_trim_host; the rules in include/sigax.h).
  void setTrim(size_t rounds, size_t minBranchLength, long minBranchCoverage = -1) {
    _rounds = rounds;
    _minBranchLength = minBranchLength;
    _minBranchCoverage = minBranchCoverage;
  }
  // The graph between the unitigs as ASQG (gzip when the name ends in .gz): the header, "VT\tunitig-<n>\t<bases>\tSS:i:0" with
  // "\tCR:i:<reads>" for more than one read, then one ED line per record that was not merged, over unitig names and lengths.
  void setGraph(const std::string& path) { _graph = path; }
  // one "name\tround" line per removed read, in read order
  void setRemoved(const std::string& path) { _removed = path; }
  // Non-maximal overlap cutting in every round, before its trim step, as the default mode of the reference's `assemble` does it
  // (MaximumOverlapVisitor, src/bigraph_visitors.cpp:410-512): at a unitig that scores as unique under (numReads, genomeSize,
  // threshold; -N, -G, -T) every record shorter by `delta` (-d) or more than the longest of its read end is cut; `careful`
  // (--max-overlap-carefully) keeps it where its other end knows no better one.  delta = 0, the default: none, and run() goes
  // through the calls it went through without this.  numReads = 0: the reads of the file.  (sigax_unitigs_prune_host; the
  // rules in include/sigax.h.)
  void setMaxOverlap(size_t delta, bool careful, size_t numReads, size_t genomeSize, double threshold = 13.0) {
    _delta = delta;
    _careful = careful;
    _numReads = numReads;
    _genomeSize = genomeSize;
    _uniqThreshold = threshold;
  }
  // one "query name\ttarget name\tlength\tround" line per cut record, in record order
  void setCutEdges(const std::string& path) { _cutEdges = path; }
  // Chimeric unitig removal as the last step of every round, as the default mode of the reference's `assemble` does it with -l
  // (ChimericVisitor, src/bigraph_visitors.cpp:83-198): a unitig of at most minLength bases (-l; 0, the default: none, and run()
  // goes through the calls it went through without this) and, with minCoverage >= 0 (-A; -1: no such test), of low coverage, that
  // bridges two branched read ends, goes where a neighbour is unique under `threshold` (-T) and no other unitig there is as short
  // (within `delta`, -a) or as thin.  Needs rounds and a genome size (setTrim, setMaxOverlap).  (sigax_unitigs_chimeric_host; the
  // rules in include/sigax.h.)
  void setChimeric(size_t minLength, long minCoverage = -1, size_t delta = 0, double threshold = 0.0) {
    _chimLength = minLength;
    _chimCoverage = minCoverage;
    _chimDelta = delta;
    _chimThreshold = threshold;
  }
  // one "name\tround" line per read a chimeric step removed, in read order
  void setChimericOut(const std::string& path) { _chimericOut = path; }
  // Bubble popping between the trim and the chimeric step of every round (the reference declares SmoothingVisitor and leaves it
  // empty; the rules are include/sigax.h's): of the unitigs that join the same two read ends and hold the same number of bases
  // between them, at most maxSpan (-b; 0, the default: none, and run() goes through the calls it went through without this), the
  // one with the most reads stays; another goes where its bases differ from the winner's in at most `divergence` per mille of
  // that window (--bubble-divergence; -1: no bases test).  Needs rounds (setTrim).  (sigax_unitigs_bubble_host.)
  void setBubble(size_t maxSpan, long divergence = 50) {
    _bubbleSpan = maxSpan;
    _bubbleDivergence = divergence;
  }
  // Indel bubble popping between the bubble and the chimeric step of every round (the rules are include/sigax.h's): the arms that
  // join the same two read ends form one group whatever their spans; an arm whose span differs from the winner's by 1 to maxEdits
  // (--bubble-edits; 0, the default: none; at most 31) goes where the edit distance of the two windows is at most maxEdits and at
  // most `permille` per mille (--bubble-edit-permille) of the bases of the shorter of the two unitigs.  Needs setBubble with a span of
  // at most 4096.  (sigax_unitigs_indel_host.)
  void setBubbleEdits(size_t maxEdits, size_t permille = 50) {
    _bubbleEdits = maxEdits;
    _bubbleEditPermille = permille;
  }
  // Transitive reduction (the rules are include/sigax.h's): a pass before every round's steps and once more before the final unitigs
  // flags the records a third read explains exactly; a flagged record is not there for any step, for the unitigs or for the graph.
  // Without rounds it is "reduce, then simplify()": the way to turn the records of an exhaustive overlap run into a string graph.
  // (sigax_unitigs_reduce_host.)
  void setReduce(bool reduce) { _reduce = reduce; }
  // one "query name\ttarget name\tlength" line per record flagged in the final graph, in record order (needs setReduce)
  void setReducedEdges(const std::string& path) { _reducedEdges = path; }
  // one "name\tround" line per read a bubble step removed, in read order; then, with setBubbleEdits, one "name\tround\tindel" line
  // per read an indel step removed, in read order
  void setBubbleOut(const std::string& path) { _bubbleOut = path; }
  // The paired-end side (sigax_unitigs_pairs_host; the rules in include/sigax.h): mates are found by name as PairEnd::id does
  // (src/reads.cpp:19-41; the last character swaps 1<->2, A<->B, f<->r), every pair is looked up in the unitigs this run built,
  // and `json` gets {"pairs": {the 24 counts by name, insert_size, delta, span_mean, span_sd, hist_bins, hist_shift, histogram
  // [[bin, pairs], ...]}}: the estimate of the reference's InsertSizeEstimateVisitor (src/bigraph_visitors.cpp:517-663) and the
  // spans of the pairs of the library's orientation (inward; `outward`: outward).  `links` not empty: one line
  // "LK\tunitig-<u>\t<B|E>\tunitig-<v>\t<B|E>\t<count>\t<min_span>\t<sum_span>" per pair of unitig ends that pairs join, ascending;
  // maxSpan > 0 leaves out the pairs whose span with the two ends abutting would exceed it.  json empty, the default: none, and
  // every other output is the one without this call.
  void setPairs(const std::string& json, const std::string& links = std::string(), uint64_t maxSpan = 0, bool outward = false,
                size_t bins = 1024, size_t shift = 0) {
    _pairsOut = json;
    _linksOut = links;
    _maxSpan = maxSpan;
    _outward = outward;
    _pairsBins = bins;
    _pairsShift = shift;
  }
  // Scaffolds (sigax_scaffold_host; the rules in include/sigax.h), behind the pairs call and over its links: `fasta` gets
  // ">scaffold-<n> unitigs=<k> gaps=<k - 1>[ circular=<closing gap>]" and the bases, N in the gaps; `layout`, if not empty, one
  // line "scaffold-<n>\tunitig-<u>\t<+|->\t<offset>\t<gap before>" per placement.  A link of at least minPairs pairs between
  // unitigs of at least minUnitigBases bases that is the only strong one at both its ends joins them (linkRatio > 0: links with
  // count * linkRatio <= the largest count at either end are set aside).  insertSize < 0: floor(sum span / n) of the pairs call,
  // and a failure when no pair of the library's orientation lay inside a unitig.  fasta empty, the default: none, and every
  // other output is the one without this call.  Needs setPairs.
  void setScaffold(const std::string& fasta, const std::string& layout = std::string(), size_t minPairs = 2, size_t linkRatio = 0,
                   size_t minUnitigBases = 0, long long insertSize = -1, size_t minGap = 1, size_t maxGap = 1000000) {
    _scaffoldOut = fasta;
    _scaffoldLayout = layout;
    _scMinPairs = minPairs;
    _scLinkRatio = linkRatio;
    _scMinUnitigBases = minUnitigBases;
    _scInsertSize = insertSize;
    _scMinGap = minGap;
    _scMaxGap = maxGap;
  }
  // Gap filling (sigax_gapfill_host; the rules in include/sigax.h), behind the scaffold call and over the index the run already
  // holds: every gap whose k-mer walk arrives gets its bases instead of N before the scaffolds are written, every FASTA header
  // ends in " filled=<n>", the layout gives the new offsets and gaps, and `gaps`, if not empty, gets one GP line per gap.  Off by
  // default: every output is then the one without this call.  Needs setScaffold.
  void setGapfill(bool on, size_t kmer = 31, size_t minCount = 3, size_t slack = 100, size_t maxFill = 10000, const std::string& gaps = std::string()) {
    _gapfill = on;
    _gapKmer = kmer;
    _gapMinCount = minCount;
    _gapSlack = slack;
    _gapMaxFill = maxFill;
    _gapsOut = gaps;
  }
  // Overlapping neighbours joined (sigax_join_host; the rules in include/sigax.h), behind the scaffold call or, with gap filling,
  // behind that: two neighbours whose ends overlap by exactly one length in minOverlap .. maxOverlap, with at most `slack` N
  // between them and every k-mer across the junction seen minCount times, are written as one sequence; every FASTA header ends
  // in " joined=<n>", the layout's gap before is signed, and `joins`, if not empty, gets one JN line per gap.  Off by default.
  void setJoinOverlaps(bool on, size_t minOverlap = 16, size_t maxOverlap = 1000, size_t slack = 100, size_t kmer = 31, size_t minCount = 3,
                       const std::string& joins = std::string()) {
    _join = on;
    _joinMinOverlap = minOverlap;
    _joinMaxOverlap = maxOverlap;
    _joinSlack = slack;
    _joinKmer = kmer;
    _joinMinCount = minCount;
    _joinsOut = joins;
  }
  uint64_t joinGaps() const { return _joinGaps; }
  uint64_t joinsMade() const { return _joinsMade; }
  uint64_t joinOverlapBases() const { return _joinOverlapBases; }
  uint64_t joinNRemoved() const { return _joinNRemoved; }
  // Ends that nearly agree (sigax_join_approx_host; needs setJoinOverlaps): where no overlap length matches exactly, the one length
  // whose ends differ in at most min(mismatches, v * permille / 1000) bases is taken, each differing base settled by the reads.
  // The headers then go on with " corrected=<n>" and the JN lines with "\t<mismatches>\t<taken from the right>".  0 = off.
  void setJoinMismatches(size_t mismatches, size_t permille = 50) {
    _joinMismatches = mismatches;
    _joinMismatchPermille = permille;
  }
  // Mismatch overlaps in (`-e`; the rules of the `siga overlap -e` block of include/sigax.h): the records come from
  // MismatchRecords over every read of the index instead of the exact overlap stages, every record that touches a contained read
  // is dropped before the unitig call, so that such a read ends up as a unitig of its own, and no output shows those unitigs;
  // unitig numbers stay the call's.  The irreducible / rc flags of the constructor play no part.  `contained`, if not empty, gets
  // the names of the contained reads, one per line, in input order.  With --pairs a pair with a contained mate is no pair.
  // unitigs() counts the call's unitigs, the hidden ones among them (unitigsHidden()).  With trim rounds a contained read on
  // its own is an island like any other: the trim step may remove it, and setRemoved's file then lists it with its round.
  void setMismatch(const sigax_mmo_params& params, const std::string& contained = std::string()) {
    _mismatch = true;
    _mmo = params;
    _containedOut = contained;
  }
  // With setMismatch: the containment records are asked for too, and right behind the unitig call sigax_contained_place_host gives
  // every contained read the placement its container implies (the rules in include/sigax.h).  Its layout then feeds the consensus
  // pass, the KC:i: counts, the layout file (a placed contained read's line ends in "\tcontained"), the graph's CR:i: and the pairs:
  // a pair whose contained mate is placed is a pair again, and containedMates() counts only those still unplaced.  setRemoved's
  // file does not list a placed contained read.  The hidden unitigs are still recognised from the call's own layout, and unitig
  // numbers stay.
  void setPlaceContained(bool on) { _placeContained = on; }
  const uint64_t* placeStatus() const { return _placeStatus; }  // status8 of sigax_contained_place_host
  const uint64_t* placeClasses() const { return _placeClasses; }  // reads per SIGAX_CP_* class
  // The consensus pass (sigax_consensus_host; the rules in include/sigax.h) right behind the unitig call and before anything reads
  // the bases: every column by majority vote over the reads laid over it; every FASTA header then ends in " changed=<columns>".
  void setConsensus(bool on, size_t minVotes = 1) {
    _consensus = on;
    _minVotes = minVotes;
  }
  uint64_t containedReads() const { return _containedReads; }
  uint64_t unitigsHidden() const { return _unitigsHidden; }    // unitigs of one contained read each, which no output shows
  uint64_t containedMates() const { return _containedMates; }  // pairs left out because a mate is contained
  uint64_t consensusChanged() const { return _consChanged; }   // columns the vote replaced
  const uint64_t* consensusStatus() const { return _consStatus; }
  const uint64_t* mismatchStatus() const { return _mmStatus; }
  uint64_t joinsApproximate() const { return _joinsApprox; }
  uint64_t joinCorrected() const { return _joinCorrected; }
  uint64_t gaps() const { return _gaps; }
  uint64_t gapsFilled() const { return _gapsFilled; }
  uint64_t gapFillBases() const { return _gapFillBases; }
  uint64_t gapBasesLeft() const { return _gapBasesLeft; }
  uint64_t scaffolds() const { return _scaffolds; }
  uint64_t scaffoldJoins() const { return _scJoins; }          // joins merged
  uint64_t scaffoldAmbiguous() const { return _scAmbiguous; }  // strong links that are not the only one at an end
  uint64_t scaffoldGapBases() const { return _scGapBases; }
  uint64_t pairs() const { return _pairs; }
  uint64_t pairsSame() const { return _pairsSame; }      // both mates in one unitig that is no ring
  uint64_t pairsAcross() const { return _pairsAcross; }  // the mates in two unitigs
  uint64_t pairLinks() const { return _pairLinks; }      // link records
  uint64_t insertSize() const { return _insertSize; }
  uint64_t insertDelta() const { return _insertDelta; }
  uint64_t chimericUnitigs() const { return _chimUnitigs; }
  uint64_t chimericReads() const { return _chimReads; }
  uint64_t bubblesPopped() const { return _bubPopped; }  // arms popped
  uint64_t bubbleReads() const { return _bubReads; }
  uint64_t bubblesKept() const { return _bubKept; }      // losers kept because they failed the bases test, over the rounds
  uint64_t indelsPopped() const { return _indPopped; }   // arms the indel steps popped
  uint64_t indelReads() const { return _indReads; }
  uint64_t indelsKept() const { return _indKept; }       // compared losers kept, over the rounds
  uint64_t indelsNotCompared() const { return _indSkipped; }  // losers of the winner's span or more than maxEdits from it, over the rounds
  uint64_t reducedFirst() const { return _redFirst; }    // records the first reduction pass flagged
  uint64_t reducedFinal() const { return _redFinal; }    // records flagged in the final graph
  uint64_t reducePasses() const { return _redPasses; }   // passes that ran
  uint64_t recordsCut() const { return _recordsCut; }
  uint64_t cutRounds() const { return _cutRounds; }    // rounds in which something was cut
  uint64_t trimRounds() const { return _trimRounds; }  // rounds that removed something (with setMaxOverlap: or cut something)
  uint64_t islands() const { return _islands; }
  uint64_t deadEnds() const { return _deadEnds; }
  uint64_t readsRemoved() const { return _readsRemoved; }
  uint64_t unitigs() const { return _unitigs; }
  uint64_t bases() const { return _bases; }
  uint64_t merged() const { return _merged; }  // simple records merged
  uint64_t cycles() const { return _cycles; }
  const std::string& error() const { return _error; }

 private:
  bool _irreducible, _rc;
  uint64_t _unitigs, _bases, _merged, _cycles;
  size_t _piece = 0;
  size_t _rounds = 0, _minBranchLength = 150;
  long _minBranchCoverage = -1;
  std::string _graph, _removed, _cutEdges;
  uint64_t _trimRounds = 0, _islands = 0, _deadEnds = 0, _readsRemoved = 0, _recordsCut = 0, _cutRounds = 0;
  size_t _delta = 0, _numReads = 0, _genomeSize = 0;
  bool _careful = false;
  double _uniqThreshold = 13.0;
  size_t _chimLength = 0, _chimDelta = 0;
  long _chimCoverage = -1;
  double _chimThreshold = 0.0;
  std::string _chimericOut;
  uint64_t _chimUnitigs = 0, _chimReads = 0;
  size_t _bubbleSpan = 0;
  long _bubbleDivergence = 50;
  std::string _bubbleOut;
  uint64_t _bubPopped = 0, _bubReads = 0, _bubKept = 0;
  size_t _bubbleEdits = 0, _bubbleEditPermille = 50;
  uint64_t _indPopped = 0, _indReads = 0, _indKept = 0, _indSkipped = 0;
  bool _reduce = false;
  std::string _reducedEdges;
  uint64_t _redFirst = 0, _redFinal = 0, _redPasses = 0;
  std::string _pairsOut, _linksOut;
  uint64_t _maxSpan = 0;
  bool _outward = false;
  size_t _pairsBins = 1024, _pairsShift = 0;
  uint64_t _pairs = 0, _pairsSame = 0, _pairsAcross = 0, _pairLinks = 0, _insertSize = 0, _insertDelta = 0;
  std::string _scaffoldOut, _scaffoldLayout;
  size_t _scMinPairs = 2, _scLinkRatio = 0, _scMinUnitigBases = 0, _scMinGap = 1, _scMaxGap = 1000000;
  long long _scInsertSize = -1;
  uint64_t _scaffolds = 0, _scJoins = 0, _scAmbiguous = 0, _scGapBases = 0;
  bool _mismatch = false, _consensus = false, _placeContained = false;
  uint64_t _placeStatus[8] = {0, 0, 0, 0, 0, 0, 0, 0}, _placeClasses[6] = {0, 0, 0, 0, 0, 0};
  sigax_mmo_params _mmo = {24, 12, 256, 45, 0, 512, 0, 0};
  size_t _minVotes = 1;
  std::string _containedOut;
  uint64_t _containedReads = 0, _containedMates = 0, _consChanged = 0, _unitigsHidden = 0;
  uint64_t _consStatus[8] = {0, 0, 0, 0, 0, 0, 0, 0}, _mmStatus[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  bool _gapfill = false;
  size_t _gapKmer = 31, _gapMinCount = 3, _gapSlack = 100, _gapMaxFill = 10000;
  std::string _gapsOut;
  uint64_t _gaps = 0, _gapsFilled = 0, _gapFillBases = 0, _gapBasesLeft = 0;
  bool _join = false;
  size_t _joinMinOverlap = 16, _joinMaxOverlap = 1000, _joinSlack = 100, _joinKmer = 31, _joinMinCount = 3;
  std::string _joinsOut;
  uint64_t _joinGaps = 0, _joinsMade = 0, _joinOverlapBases = 0, _joinNRemoved = 0;
  size_t _joinMismatches = 0, _joinMismatchPermille = 50;
  uint64_t _joinsApprox = 0, _joinCorrected = 0;
  std::string _error;
};

// `siga preqc`: the k-mer count distribution of strings drawn from the index itself (KmerDistribution::sample,
// src/kmerdistr.cpp:7-36: FMIndex::getString of a row, then occ(w) + occ(revcomp(w)) for its windows), the number one reads
// `siga correct -x` off.  The reads file is not needed: the strings come back out of the .bwt.
class KmerSpectrum {
 public:
  struct Options {
    size_t kmerSize, samples, seed, maxCount;  // -k, -n (the reference's _samples), --seed, --max-count
    bool all;                                  // --all: every read once (rows 0 .. n_strings - 1) instead of sampled rows
    Options() : kmerSize(31), samples(50000), seed(1), maxCount(1024), all(false) {}
  };
  explicit KmerSpectrum(const Options& options) : _options(options), _strings(0), _bases(0), _windows(0), _rows(0) {}
  // walks the rows and counts their windows on the GPU, batch by batch (batchRows = rows per device batch, 0: from the
  // device's free memory); one histogram accumulates over the batches
  bool run(const FMIndex& index, size_t batchRows = 0);
  // histogram()[c] = windows whose k-mer occurs c times, both strands together; the last entry = maxCount or more
  const std::vector<uint64_t>& histogram() const { return _hist; }
  uint64_t strings() const { return _strings; }  // strings of at least k bases
  uint64_t bases() const { return _bases; }      // their bases (what KmerDistribution::sample returns)
  uint64_t windows() const { return _windows; }
  // {"KmerDistribution": {"k", "mode", "samples", "seed", "strings", "bases", "windows", "max_count", "distribution": [[count,
  // windows], ...]}} and a newline; the distribution lists the non-empty bins in ascending order
  std::string json() const;
  const std::string& error() const { return _error; }

 private:
  Options _options;
  std::vector<uint64_t> _hist;
  uint64_t _strings, _bases, _windows, _rows;
  std::string _error;
};

}  // namespace sigah

#endif
