// siga_amd/host/unitig.cpp -- Unitigger (`siga unitig`): the reads through the overlap stages, their edge records compacted into unitigs.
#include <cstdio>

#include "asqg_text.hpp"
#include "host_util.hpp"
#include "pairs.hpp"
#include "reads.hpp"
#include "siga_host.hpp"

namespace sigah {

namespace {
// what sigax_unitigs_host gave back; the arrays are the library's (sigax_free)
struct Unitigs {
  uint64_t n = 0;
  uint64_t *seq_offs = nullptr, *lay_offs = nullptr;
  uint32_t* uflags = nullptr;
  sigax_placement* layout = nullptr;
  char* useqs = nullptr;
  uint32_t* removed = nullptr;  // the two of sigax_unitigs_trim_host
  sigax_edge* uedges = nullptr;
  uint32_t* cut = nullptr;  // sigax_unitigs_prune_host's
  Unitigs() = default;
  Unitigs(const Unitigs&) = delete;
  Unitigs& operator=(const Unitigs&) = delete;
  ~Unitigs() {
    sigax_free(seq_offs);
    sigax_free(lay_offs);
    sigax_free(uflags);
    sigax_free(layout);
    sigax_free(useqs);
    sigax_free(removed);
    sigax_free(uedges);
    sigax_free(cut);
  }
};

bool write_all(FILE* f, const std::string& t) { return t.empty() || fwrite(t.data(), 1, t.size(), f) == t.size(); }
}  // namespace

// The unitig graph as ASQG: the header, one VT line per unitig, one ED line per lifted record (AsqgWriter's formatter over the
// unitigs' names and lengths).
static bool write_graph_file(const std::string& path, const Unitigs& u, uint64_t n_uedges, size_t minOverlap, const std::vector<uint8_t>& hidden) {
  OutFile out(path);
  if (!out.ok()) return false;
  out.write(asqg_header(minOverlap));
  std::string t;
  std::vector<std::string> names((size_t)u.n);
  for (uint64_t k = 0; k < u.n; ++k) {
    names[k] = "unitig-";
    append_u64(names[k], k);
    if (!hidden.empty() && hidden[k]) continue;  // (a contained read on its own: no record touches it)
    const uint64_t cnt = u.lay_offs[k + 1] - u.lay_offs[k];
    t += "VT\t";
    t += names[k];
    t += '\t';
    t.append(u.useqs + u.seq_offs[k], u.seq_offs[k + 1] - u.seq_offs[k]);
    t += "\tSS:i:0";
    if (cnt > 1) {
      t += "\tCR:i:";
      append_u64(t, cnt);
    }
    t += '\n';
    if (t.size() >= ((size_t)1 << 20)) {
      out.write(t);
      t.clear();
    }
  }
  for (uint64_t i = 0; i < n_uedges; ++i) {
    const sigax_edge& e = u.uedges[i];
    if (e.query >= u.n || e.target >= u.n) return false;
    append_edge_line(t, e, names[e.query], names[e.target], u.seq_offs[e.query + 1] - u.seq_offs[e.query],
                     u.seq_offs[e.target + 1] - u.seq_offs[e.target]);
    if (t.size() >= ((size_t)1 << 20)) {
      out.write(t);
      t.clear();
    }
  }
  out.write(t);
  return out.close();
}

// The reads go through OverlapBuilder's device stages (sigax_overlap_batch: finder, filter, extractor, edge records) a piece
// at a time under their ids in the file; no VT or ED line is formatted.  The collected records and the reads then make one
// sigax_unitigs_host call.
bool Unitigger::run(const FMIndex& index, const std::string& input, size_t minOverlap, const std::string& fasta, const std::string& layout,
                    size_t threads) {
  _error.clear();
  _unitigs = _bases = _merged = _cycles = _trimRounds = _islands = _deadEnds = _readsRemoved = _recordsCut = _cutRounds = _chimUnitigs = _chimReads = _pairs = _pairsSame = _pairsAcross = _pairLinks = _insertSize = _insertDelta = 0;
  _scaffolds = _scJoins = _scAmbiguous = _scGapBases = 0;
  _gaps = _gapsFilled = _gapFillBases = _gapBasesLeft = 0;
  _joinGaps = _joinsMade = _joinOverlapBases = _joinNRemoved = _joinsApprox = _joinCorrected = 0;
  _containedReads = _containedMates = _consChanged = _unitigsHidden = 0;
  for (int k = 0; k < 8; ++k) _consStatus[k] = _mmStatus[k] = _placeStatus[k] = 0;
  for (int k = 0; k < 6; ++k) _placeClasses[k] = 0;
  auto fail = [&](const std::string& e) { return _error = e, false; };
  if (!index.handle()) return fail("FMIndex not loaded");
  if (!_mismatch && !_containedOut.empty()) return fail("contained reads are only written with mismatch overlaps");
  if (!_mismatch && _placeContained) return fail("contained reads are only placed with mismatch overlaps");
  if (_consensus && (_minVotes < 1 || _minVotes > 0xFFFFFFFFull)) return fail("consensus min-votes out of range");
  MismatchRecords mm;  // the reference text once, before any file is touched: an index that cannot serve is refused here
  if (_mismatch && !mm.open(index, &_error)) return false;
  const HostSettings hs;
  const unsigned nt = host_threads(threads, hs);
  ReadStore reads;
  if (!LoadReads(input, &reads, nt, hs)) return fail("Failed to read file " + input);
  const size_t n = reads.size();
  std::vector<uint32_t> lengths, ranks;
  name_ranks(reads, nt, &lengths, &ranks);
  if (n > 0 && sigax_index_set_reads(index.handle(), lengths.data(), ranks.data(), n) != SIGAX_OK)
    return fail(std::string("failed to load suffix array index: ") + sigax_last_error());
  sigax_index_info inf;
  if (sigax_index_info_get(index.handle(), &inf) != SIGAX_OK) return fail(sigax_last_error());
  const uint32_t flags = SIGAX_EDGES | (_irreducible ? SIGAX_IRREDUCIBLE : 0u) | (_rc ? SIGAX_RC : 0u);
  std::vector<sigax_edge> edges;
  std::vector<uint64_t> offs;
  const size_t per = _piece ? _piece : (size_t)1 << 20;
  std::vector<uint8_t> contained;  // -e: one byte per read
  std::vector<sigax_mm_edge> containments;  // --place-contained: where every contained read lies in its containers
  if (_mismatch) {
    if (inf.n_strings != n) return fail(input + " holds " + std::to_string(n) + " reads, the index " + std::to_string(inf.n_strings));
    sigax_mmo_params p = _mmo;
    p.min_overlap = (uint32_t)std::min<size_t>(minOverlap, 0xFFFFFFFFull);
    std::vector<uint32_t> num_diff;
    if (!mm.find(index, p, n, nt, &edges, &num_diff, &contained, _mmStatus, &_error, _placeContained ? &containments : nullptr)) return false;
    // a record that touches a contained read is dropped: the read stays a unitig of its own, which no output shows
    size_t kept = 0;
    for (size_t i = 0; i < edges.size(); ++i)
      if (!contained[edges[i].query] && !contained[edges[i].target]) edges[kept++] = edges[i];
    edges.resize(kept);
    for (size_t r = 0; r < n; ++r) _containedReads += contained[r] ? 1 : 0;
  }
  for (size_t base = 0; base < n && !_mismatch; base += per) {
    const size_t cnt = std::min(per, n - base);
    offs.resize(cnt + 1);
    for (size_t i = 0; i <= cnt; ++i) offs[i] = reads.offs[base + i] - reads.offs[base];
    sigax_result res;
    if (sigax_overlap_batch(index.handle(), reads.seqs.data() + reads.offs[base], offs.data(), (uint32_t)cnt, (uint32_t)base, (uint32_t)minOverlap,
                            flags, &res) != SIGAX_OK)
      return fail(std::string("overlap failed: ") + sigax_last_error());
    edges.insert(edges.end(), res.edges, res.edges + res.n_edges);
    sigax_result_free(&res);
  }
  Unitigs u;
  uint64_t status[40] = {0};
  const bool trim = _rounds > 0 || !_graph.empty() || !_removed.empty();
  if (!_chimericOut.empty() && _chimLength == 0) return fail("chimeric reads are only written with a min-chimeric length");
  if (!_bubbleOut.empty() && _bubbleSpan == 0) return fail("bubble reads are only written with a max-bubble span");
  if (_bubbleEdits > 0 && (_bubbleSpan == 0 || _bubbleSpan > SIGAX_INDEL_MAX_SPAN)) return fail("bubble edits need a max-bubble span of 1 to 4096");
  if (_bubbleEdits > SIGAX_INDEL_MAX_EDITS || _bubbleEditPermille > 0xFFFFFFFFull) return fail("bubble edits or their per mille out of range");
  if (!_cutEdges.empty() && _delta == 0) return fail("cut records are only written with a max-overlap delta");
  if (!_reducedEdges.empty() && !_reduce) return fail("transitive records are only written with the reduction");
  if (_pairsOut.empty() && !_linksOut.empty()) return fail("links are only written with the pairs statistics");
  if (!_pairsOut.empty() && (_pairsBins == 0 || _pairsBins > SIGAX_PAIRS_MAX_BINS || _pairsShift > 31)) return fail("pairs bins or shift out of range");
  if (_pairsOut.empty() && !_scaffoldOut.empty()) return fail("scaffolds are only built with the pairs statistics");
  if (_scaffoldOut.empty() && !_scaffoldLayout.empty()) return fail("the scaffold layout is only written with the scaffolds");
  if (!_scaffoldOut.empty() && (_scMinPairs > 0xFFFFFFFFull || _scLinkRatio > 0xFFFFFFFFull || _scMinUnitigBases > 0xFFFFFFFFull || _scMinGap < 1 ||
                                _scMaxGap < _scMinGap || _scMaxGap >= (1ull << 31) || _scInsertSize >= (1ll << 62)))
    return fail("scaffold options out of range");
  if (_gapfill && _scaffoldOut.empty()) return fail("gaps are only filled in scaffolds");
  if (_gapfill && (_gapKmer < 8 || _gapKmer > 128 || _gapMinCount < 1 || _gapMinCount > 0xFFFFFFFFull || _gapSlack >= (1ull << 31) ||
                   _gapMaxFill >= (1ull << 31)))
    return fail("gap filling options out of range");
  if (_join && _scaffoldOut.empty()) return fail("overlaps are only joined in scaffolds");
  if (_join && (_joinMinOverlap < 8 || _joinMaxOverlap < _joinMinOverlap || _joinMaxOverlap > 4096 || _joinSlack >= (1ull << 31) || _joinKmer < 8 ||
                _joinKmer > 128 || _joinMinCount < 1 || _joinMinCount > 0xFFFFFFFFull || _joinMismatches > 16 || _joinMismatchPermille < 1 ||
                _joinMismatchPermille > 250))
    return fail("overlap joining options out of range");
  if (trim || _delta > 0 || _reduce) {
    if (_rounds > 64) return fail("at most 64 trim rounds");
    if (_minBranchLength > 0xFFFFFFFFull || _minBranchCoverage >= (long)0xFFFFFFFFll) return fail("branch length or coverage out of range");
  }
  // the steps asked for: each call is the one before it with one more step in its rounds, and more scratch
  const int level = _reduce ? 6 : _bubbleEdits > 0 ? 5 : _bubbleSpan > 0 ? 4 : _chimLength > 0 ? 3 : _delta > 0 ? 2 : trim ? 1 : 0;
  if (level >= 2 && _delta > 0xFFFFFFFFull) return fail("max-overlap delta out of range");
  if (level >= 3 && (_chimLength > 0xFFFFFFFFull || _chimDelta > 0xFFFFFFFFull || _chimCoverage >= (long)0xFFFFFFFFll))
    return fail("chimeric length, delta or coverage out of range");
  if (level >= 4 && (_bubbleSpan > 0xFFFFFFFFull || _bubbleDivergence >= (long)0xFFFFFFFFll)) return fail("bubble span or divergence out of range");
  sigax_reduce_opts ropts;
  sigax_indel_opts& iopts = ropts.indel;
  sigax_bubble_opts& opts = iopts.bubble;
  sigax_chimeric_opts& co = opts.chimeric;
  sigax_prune_opts& po = co.prune;
  po.max_rounds = (uint32_t)_rounds;
  po.min_branch_length = (uint32_t)_minBranchLength;
  po.min_branch_coverage = _minBranchCoverage < 0 ? SIGAX_TRIM_NO_COVERAGE : (uint32_t)_minBranchCoverage;
  po.delta = (uint32_t)_delta;
  po.careful = _careful ? 1u : 0u;
  po.reserved = 0;
  po.num_reads = _numReads ? _numReads : n;
  po.genome_size = _genomeSize;
  po.uniq_threshold = _uniqThreshold;
  co.min_chimeric_length = (uint32_t)_chimLength;
  co.min_chimeric_coverage = _chimCoverage < 0 ? SIGAX_TRIM_NO_COVERAGE : (uint32_t)_chimCoverage;
  co.chimeric_delta = (uint32_t)_chimDelta;
  co.reserved2 = 0;
  co.chimeric_threshold = _chimThreshold;
  opts.max_bubble_span = (uint32_t)_bubbleSpan;
  opts.max_divergence_permille = _bubbleDivergence < 0 ? SIGAX_BUBBLE_NO_BASES : (uint32_t)_bubbleDivergence;
  opts.reserved3[0] = opts.reserved3[1] = 0;
  iopts.max_edits = (uint32_t)_bubbleEdits;
  iopts.max_edit_permille = (uint32_t)_bubbleEditPermille;
  iopts.reserved4[0] = iopts.reserved4[1] = 0;
  ropts.reduce = _reduce ? 1u : 0u;
  ropts.reserved5[0] = ropts.reserved5[1] = ropts.reserved5[2] = 0;
  sigax_edge** const uedges = _graph.empty() ? nullptr : &u.uedges;
  if (level == 6) {
    if (sigax_unitigs_reduce_host(inf.device, edges.data(), edges.size(), lengths.data(), reads.seqs.data(), reads.offs.data(), n,
                                  (uint32_t)minOverlap, &ropts, &u.n, &u.seq_offs, &u.lay_offs, &u.uflags, &u.layout, &u.useqs, &u.removed, &u.cut,
                                  uedges, status) != SIGAX_OK)
      return fail(std::string("unitig failed: ") + sigax_last_error());
  } else if (level == 5) {
    if (sigax_unitigs_indel_host(inf.device, edges.data(), edges.size(), lengths.data(), reads.seqs.data(), reads.offs.data(), n,
                                 (uint32_t)minOverlap, &iopts, &u.n, &u.seq_offs, &u.lay_offs, &u.uflags, &u.layout, &u.useqs, &u.removed, &u.cut,
                                 uedges, status) != SIGAX_OK)
      return fail(std::string("unitig failed: ") + sigax_last_error());
  } else if (level == 4) {
    if (sigax_unitigs_bubble_host(inf.device, edges.data(), edges.size(), lengths.data(), reads.seqs.data(), reads.offs.data(), n,
                                  (uint32_t)minOverlap, &opts, &u.n, &u.seq_offs, &u.lay_offs, &u.uflags, &u.layout, &u.useqs, &u.removed, &u.cut,
                                  uedges, status) != SIGAX_OK)
      return fail(std::string("unitig failed: ") + sigax_last_error());
  } else if (level == 3) {
    if (sigax_unitigs_chimeric_host(inf.device, edges.data(), edges.size(), lengths.data(), reads.seqs.data(), reads.offs.data(), n,
                                    (uint32_t)minOverlap, &co, &u.n, &u.seq_offs, &u.lay_offs, &u.uflags, &u.layout, &u.useqs, &u.removed, &u.cut,
                                    uedges, status) != SIGAX_OK)
      return fail(std::string("unitig failed: ") + sigax_last_error());
  } else if (level == 2) {
    if (sigax_unitigs_prune_host(inf.device, edges.data(), edges.size(), lengths.data(), reads.seqs.data(), reads.offs.data(), n, (uint32_t)minOverlap,
                                 &po, &u.n, &u.seq_offs, &u.lay_offs, &u.uflags, &u.layout, &u.useqs, &u.removed, &u.cut, uedges,
                                 status) != SIGAX_OK)
      return fail(std::string("unitig failed: ") + sigax_last_error());
  } else if (level == 1) {
    const sigax_trim_opts to = {po.max_rounds, po.min_branch_length, po.min_branch_coverage, 0};
    if (sigax_unitigs_trim_host(inf.device, edges.data(), edges.size(), lengths.data(), reads.seqs.data(), reads.offs.data(), n, (uint32_t)minOverlap,
                                &to, &u.n, &u.seq_offs, &u.lay_offs, &u.uflags, &u.layout, &u.useqs, &u.removed, uedges, status) != SIGAX_OK)
      return fail(std::string("unitig failed: ") + sigax_last_error());
  } else {
    if (sigax_unitigs_host(inf.device, edges.data(), edges.size(), lengths.data(), reads.seqs.data(), reads.offs.data(), n, (uint32_t)minOverlap,
                           &u.n, &u.seq_offs, &u.lay_offs, &u.uflags, &u.layout, &u.useqs) != SIGAX_OK)
      return fail(std::string("unitig failed: ") + sigax_last_error());
    sigax_unitigs_last_status(status);
  }
  _unitigs = status[0];
  _bases = status[1];
  _merged = status[4];
  _cycles = status[5];
  _trimRounds = status[6];
  _islands = status[7];
  _deadEnds = status[8];
  _readsRemoved = status[9];
  _recordsCut = status[12];
  _cutRounds = status[13];
  _chimUnitigs = status[16];
  _chimReads = status[17];
  _bubPopped = status[20];
  _bubReads = status[21];
  _bubKept = status[23];
  _indPopped = status[24];
  _indReads = status[25];
  _indKept = status[27];
  _indSkipped = status[28];
  _redFirst = status[32];
  _redFinal = status[33];
  _redPasses = status[34];
  // -e: the unitigs of one contained read each, which no output shows; their numbers stay taken
  std::vector<uint8_t> hidden;
  if (_mismatch) {
    hidden.assign((size_t)u.n, 0);
    for (uint64_t k = 0; k < u.n; ++k)
      _unitigsHidden += hidden[k] = u.lay_offs[k + 1] - u.lay_offs[k] == 1 && contained[u.layout[u.lay_offs[k]].read] ? 1 : 0;
  }
  // --place-contained: the contained reads into the layout, before anything reads it; what is hidden was settled above
  struct Classes {
    uint8_t* p = nullptr;
    ~Classes() { sigax_free(p); }
  } cls;
  auto placed = [&](size_t r) { return cls.p && cls.p[r] == SIGAX_CP_PLACED; };
  if (_placeContained) {
    const sigax_contained_opts popts = {{0, 0, 0, 0}};
    uint64_t* lo2 = nullptr;
    sigax_placement* lay2 = nullptr;
    if (sigax_contained_place_host(inf.device, u.n, u.seq_offs, u.lay_offs, u.layout, lengths.data(), n, contained.data(), containments.data(),
                                   containments.size(), &popts, &lo2, &lay2, &cls.p, _placeStatus) != SIGAX_OK)
      return fail(std::string("placing the contained reads failed: ") + sigax_last_error());
    sigax_free(u.lay_offs);
    sigax_free(u.layout);
    u.lay_offs = lo2;
    u.layout = lay2;
    for (size_t r = 0; r < n; ++r) _placeClasses[cls.p[r] < 6 ? cls.p[r] : 5] += 1;
  }
  // the vote, before anything reads the bases
  struct Changed {
    uint32_t* p = nullptr;
    ~Changed() { sigax_free(p); }
  } changed;
  if (_consensus) {
    const sigax_consensus_opts copts = {(uint32_t)_minVotes, {0, 0, 0}};
    if (sigax_consensus_host(inf.device, u.n, u.seq_offs, u.lay_offs, u.layout, lengths.data(), reads.seqs.data(), reads.offs.data(), n, &copts,
                             u.useqs, &changed.p, nullptr, _consStatus) != SIGAX_OK)
      return fail(std::string("consensus failed: ") + sigax_last_error());
    _consChanged = _consStatus[2];
  }
  if (!_pairsOut.empty()) {  // over the unitigs as they stand, whichever call built them; the other outputs do not depend on it
    PairsRequest rq;
    rq.json = _pairsOut;
    rq.links = _linksOut;
    rq.maxSpan = _maxSpan;
    rq.outward = _outward;
    rq.bins = (uint32_t)_pairsBins;
    rq.shift = (uint32_t)_pairsShift;
    ScaffoldRequest sq;
    sq.fasta = _scaffoldOut;
    sq.layout = _scaffoldLayout;
    sq.minPairs = (uint32_t)_scMinPairs;
    sq.linkRatio = (uint32_t)_scLinkRatio;
    sq.minUnitigBases = (uint32_t)_scMinUnitigBases;
    sq.minGap = (uint32_t)_scMinGap;
    sq.maxGap = (uint32_t)_scMaxGap;
    sq.haveInsertSize = _scInsertSize >= 0;
    sq.insertSize = _scInsertSize >= 0 ? (uint64_t)_scInsertSize : 0;
    if (_gapfill) {  // over the index this run has open
      sq.index = index.handle();
      sq.gapKmer = (uint32_t)_gapKmer;
      sq.gapMinCount = (uint32_t)_gapMinCount;
      sq.gapSlack = (uint32_t)_gapSlack;
      sq.gapMaxFill = (uint32_t)_gapMaxFill;
      sq.gaps = _gapsOut;
    }
    if (_join) {  // likewise
      sq.joinIndex = index.handle();
      sq.joinMinOverlap = (uint32_t)_joinMinOverlap;
      sq.joinMaxOverlap = (uint32_t)_joinMaxOverlap;
      sq.joinSlack = (uint32_t)_joinSlack;
      sq.joinKmer = (uint32_t)_joinKmer;
      sq.joinMinCount = (uint32_t)_joinMinCount;
      sq.joinMismatches = (uint32_t)_joinMismatches;
      sq.joinMismatchPermille = (uint32_t)_joinMismatchPermille;
      sq.joins = _joinsOut;
    }
    uint64_t st24[24], st16[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t gp24[24] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    uint64_t jn24[24] = {0};
    std::vector<uint32_t> mate = mates_by_name(reads, ranks);
    if (_mismatch)  // a pair with a contained mate is no pair
      for (size_t r = 0; r < n; ++r) {
        const uint32_t m = mate[r];
        if (m != SIGAX_NO_MATE && m < n && ((contained[r] && !placed(r)) || (contained[m] && !placed(m)))) {
          if (mate[m] == r) {
            mate[m] = SIGAX_NO_MATE;
            ++_containedMates;
          }
          mate[r] = SIGAX_NO_MATE;
        }
      }
    rq.haveContainedMates = _mismatch;
    rq.containedMates = _containedMates;
    const std::string e = run_pairs(inf.device, mate, lengths, u.n, u.seq_offs, u.lay_offs, u.uflags, u.layout, rq, st24,
                                    &_insertSize, &_insertDelta, &sq, u.useqs, st16, gp24, jn24);
    if (!e.empty()) return fail(e);
    _joinGaps = jn24[0];
    _joinsMade = jn24[1];
    _joinOverlapBases = jn24[9];
    _joinNRemoved = jn24[10];
    _joinsApprox = jn24[16];
    _joinCorrected = jn24[18];
    _gaps = gp24[0];
    _gapsFilled = gp24[1];
    _gapFillBases = gp24[14];
    _gapBasesLeft = gp24[15];
    _scaffolds = st16[0];
    _scJoins = st16[10];
    _scAmbiguous = st16[9];
    _scGapBases = st16[12];
    _pairs = st24[2];
    _pairsSame = st24[4];
    _pairsAcross = st24[18];
    _pairLinks = st24[22];
  }
  // ">unitig-<n>[ KC:i:<reads>][ circular=<closing overlap>]": the coverage tag only above 1, as FastaVisitor writes it
  // (src/bigraph_visitors.cpp:248-257)
  FILE* out = fasta.empty() ? stdout : fopen(fasta.c_str(), "wb");
  if (!out) return fail("Failed to create " + fasta);
  std::string t;
  bool ok = true;
  for (uint64_t k = 0; k < u.n && ok; ++k) {
    const bool last = k + 1 == u.n;
    if (!hidden.empty() && hidden[k]) {
      if (last) {
        ok = write_all(out, t);
        t.clear();
      }
      continue;
    }
    const uint64_t cnt = u.lay_offs[k + 1] - u.lay_offs[k];
    t += ">unitig-";
    append_u64(t, k);
    if (cnt > 1) {
      t += " KC:i:";
      append_u64(t, cnt);
    }
    if (u.uflags[k] & SIGAX_UNITIG_CIRCULAR) {
      t += " circular=";
      append_u64(t, u.uflags[k] >> 1);
    }
    if (_consensus) {
      t += " changed=";
      append_u64(t, changed.p[k]);
    }
    t += '\n';
    t.append(u.useqs + u.seq_offs[k], u.seq_offs[k + 1] - u.seq_offs[k]);
    t += '\n';
    if (t.size() >= ((size_t)1 << 20) || k + 1 == u.n) {
      ok = write_all(out, t);
      t.clear();
    }
  }
  if (fflush(out) != 0) ok = false;
  if (out != stdout) fclose(out);
  if (!ok) return fail("Failed to write " + (fasta.empty() ? std::string("stdout") : fasta));
  if (!_graph.empty() && !write_graph_file(_graph, u, status[11], minOverlap, hidden)) return fail("Failed to write " + _graph);
  if (!_containedOut.empty()) {  // the names of the contained reads, in input order
    FILE* rf = fopen(_containedOut.c_str(), "wb");
    if (!rf) return fail("Failed to create " + _containedOut);
    t.clear();
    for (size_t r = 0; r < n; ++r)
      if (contained[r]) {
        const std::string_view name = reads.name(r);
        t.append(name.data(), name.size());
        t += '\n';
      }
    ok = write_all(rf, t);
    if (fclose(rf) != 0) ok = false;
    if (!ok) return fail("Failed to write " + _containedOut);
    t.clear();
  }
  if (!_removed.empty()) {
    FILE* rf = fopen(_removed.c_str(), "wb");
    if (!rf) return fail("Failed to create " + _removed);
    t.clear();
    for (size_t r = 0; r < n; ++r)
      if (u.removed[r] && !placed(r)) {
        const std::string_view name = reads.name(r);
        t.append(name.data(), name.size());
        t += '\t';
        append_u64(t, u.removed[r] & ~(SIGAX_REMOVED_CHIMERIC | SIGAX_REMOVED_BUBBLE | SIGAX_REMOVED_INDEL));
        t += '\n';
      }
    ok = write_all(rf, t);
    if (fclose(rf) != 0) ok = false;
    if (!ok) return fail("Failed to write " + _removed);
    t.clear();
  }
  if (!_chimericOut.empty()) {
    FILE* rf = fopen(_chimericOut.c_str(), "wb");
    if (!rf) return fail("Failed to create " + _chimericOut);
    t.clear();
    for (size_t r = 0; r < n; ++r)
      if (u.removed[r] & SIGAX_REMOVED_CHIMERIC) {
        const std::string_view name = reads.name(r);
        t.append(name.data(), name.size());
        t += '\t';
        append_u64(t, u.removed[r] & ~SIGAX_REMOVED_CHIMERIC);
        t += '\n';
      }
    ok = write_all(rf, t);
    if (fclose(rf) != 0) ok = false;
    if (!ok) return fail("Failed to write " + _chimericOut);
    t.clear();
  }
  if (!_bubbleOut.empty()) {
    FILE* rf = fopen(_bubbleOut.c_str(), "wb");
    if (!rf) return fail("Failed to create " + _bubbleOut);
    t.clear();
    for (size_t r = 0; r < n; ++r)
      if (u.removed[r] & SIGAX_REMOVED_BUBBLE) {
        const std::string_view name = reads.name(r);
        t.append(name.data(), name.size());
        t += '\t';
        append_u64(t, u.removed[r] & ~SIGAX_REMOVED_BUBBLE);
        t += '\n';
      }
    for (size_t r = 0; r < n; ++r)  // the reads of the indel steps behind them, marked: lines of the old kind are as they were
      if (u.removed[r] & SIGAX_REMOVED_INDEL) {
        const std::string_view name = reads.name(r);
        t.append(name.data(), name.size());
        t += '\t';
        append_u64(t, u.removed[r] & ~SIGAX_REMOVED_INDEL);
        t += "\tindel\n";
      }
    ok = write_all(rf, t);
    if (fclose(rf) != 0) ok = false;
    if (!ok) return fail("Failed to write " + _bubbleOut);
    t.clear();
  }
  if (!_cutEdges.empty()) {
    FILE* cf = fopen(_cutEdges.c_str(), "wb");
    if (!cf) return fail("Failed to create " + _cutEdges);
    t.clear();
    for (size_t i = 0; i < edges.size() && ok; ++i)
      if ((u.cut[i] & ~SIGAX_CUT_TRANSITIVE) && edges[i].query < n && edges[i].target < n) {  // (bit 31 is the reduction's flag, no round)
        const std::string_view q = reads.name(edges[i].query), tg = reads.name(edges[i].target);
        t.append(q.data(), q.size());
        t += '\t';
        t.append(tg.data(), tg.size());
        t += '\t';
        append_u64(t, edges[i].length);
        t += '\t';
        append_u64(t, u.cut[i] & ~SIGAX_CUT_TRANSITIVE);
        t += '\n';
        if (t.size() >= ((size_t)1 << 20)) {
          ok = write_all(cf, t);
          t.clear();
        }
      }
    if (ok) ok = write_all(cf, t);
    if (fclose(cf) != 0) ok = false;
    if (!ok) return fail("Failed to write " + _cutEdges);
    t.clear();
  }
  if (!_reducedEdges.empty()) {  // "query name\ttarget name\tlength", the records flagged in the final graph, in record order
    FILE* cf = fopen(_reducedEdges.c_str(), "wb");
    if (!cf) return fail("Failed to create " + _reducedEdges);
    t.clear();
    for (size_t i = 0; i < edges.size() && ok; ++i)
      if ((u.cut[i] & SIGAX_CUT_TRANSITIVE) && edges[i].query < n && edges[i].target < n) {
        const std::string_view q = reads.name(edges[i].query), tg = reads.name(edges[i].target);
        t.append(q.data(), q.size());
        t += '\t';
        t.append(tg.data(), tg.size());
        t += '\t';
        append_u64(t, edges[i].length);
        t += '\n';
        if (t.size() >= ((size_t)1 << 20)) {
          ok = write_all(cf, t);
          t.clear();
        }
      }
    if (ok) ok = write_all(cf, t);
    if (fclose(cf) != 0) ok = false;
    if (!ok) return fail("Failed to write " + _reducedEdges);
    t.clear();
  }
  if (layout.empty()) return true;
  // "unitig-<n>\t<read name>\t<+|->\t<offset>", placements in layout order
  FILE* lf = fopen(layout.c_str(), "wb");
  if (!lf) return fail("Failed to create " + layout);
  t.clear();
  for (uint64_t k = 0; k < u.n && ok; ++k) {
    for (uint64_t p = u.lay_offs[k]; p < u.lay_offs[k + 1] && (hidden.empty() || !hidden[k]); ++p) {
      const sigax_placement& pl = u.layout[p];
      const std::string_view name = reads.name(pl.read);
      t += "unitig-";
      append_u64(t, k);
      t += '\t';
      t.append(name.data(), name.size());
      t += (pl.flags & SIGAX_PLACED_REV) ? "\t-\t" : "\t+\t";
      append_u64(t, pl.offset);
      if (pl.flags & SIGAX_PLACED_CONTAINED) t += "\tcontained";
      t += '\n';
    }
    if (t.size() >= ((size_t)1 << 20) || k + 1 == u.n) {
      ok = write_all(lf, t);
      t.clear();
    }
  }
  if (fclose(lf) != 0) ok = false;
  if (!ok) return fail("Failed to write " + layout);
  return true;
}

}  // namespace sigah
