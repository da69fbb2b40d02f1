// siga_amd/host/pairs.cpp -- `siga unitig --pairs`: mates by name, the pairs call over the unitigs, its two files; and
// `--scaffold`: the scaffold call over the unitigs and the links, its two files.
#include "pairs.hpp"

#include <algorithm>
#include <cstdio>

#include "host_util.hpp"

namespace sigah {

std::vector<uint32_t> mates_by_name(const ReadStore& rs, const std::vector<uint32_t>& ranks) {
  const size_t n = rs.size();
  std::vector<uint32_t> mate(n, SIGAX_NO_MATE);
  if (n == 0) return mate;
  // one read per rank, and how many share it: the names in sorted order without comparing any twice
  uint32_t top = 0;
  for (size_t i = 0; i < n; ++i) top = std::max(top, ranks[i]);
  std::vector<uint32_t> first((size_t)top + 1, SIGAX_NO_MATE), count((size_t)top + 1, 0);
  for (size_t i = 0; i < n; ++i) {
    if (count[ranks[i]]++ == 0) first[ranks[i]] = (uint32_t)i;
  }
  std::vector<uint32_t> sorted;  // the ranks that occur, ascending: their names ascend
  sorted.reserve((size_t)top + 1);
  for (uint32_t r = 0; r <= top; ++r)
    if (count[r]) sorted.push_back(r);
  std::string want;
  for (size_t i = 0; i < n; ++i) {
    const std::string_view name = rs.name(i);
    if (name.empty() || count[ranks[i]] != 1) continue;
    char c = name.back();
    switch (c) {
      case 'A': c = 'B'; break;
      case 'B': c = 'A'; break;
      case '1': c = '2'; break;
      case '2': c = '1'; break;
      case 'f': c = 'r'; break;
      case 'r': c = 'f'; break;
      default: continue;
    }
    want.assign(name.data(), name.size());
    want.back() = c;
    const auto it = std::lower_bound(sorted.begin(), sorted.end(), std::string_view(want),
                                     [&](uint32_t r, std::string_view w) { return rs.name(first[r]) < w; });
    if (it != sorted.end() && rs.name(first[*it]) == std::string_view(want) && count[*it] == 1) mate[i] = first[*it];
  }
  return mate;
}

namespace {
const char* const kStatusNames[24] = {"mate_entries", "malformed", "pairs", "unplaced", "same", "inward", "outward", "tandem",
                                      "ring", "far", "d_n", "d_sum", "d_sq_low", "d_sq_high", "span_n", "span_sum",
                                      "span_sq_low", "span_sq_high", "across", "ring_links_dropped", "over_max_span", "linked_pairs",
                                      "link_records", "reserved"};

bool write_file(const std::string& path, const std::string& t) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) return false;
  bool ok = t.empty() || fwrite(t.data(), 1, t.size(), f) == t.size();
  if (fclose(f) != 0) ok = false;
  return ok;
}

void append_double(std::string& t, double v) {
  char buf[40];
  snprintf(buf, sizeof buf, "%.17g", v);
  t += buf;
}

const char* const kGapClasses[11] = {"FILLED", "SHORT", "NON_ACGT", "FAR", "NO_ROOM", "DEAD_END", "BRANCH", "TOO_LONG", "OVERLAP", "OFF_ESTIMATE",
                                     "MALFORMED"};
const char* gap_class(uint32_t c) { return c < 11 ? kGapClasses[c] : "NOT_RUN"; }
const char* const kJoinClasses[8] = {"JOINED", "CLOSED", "FAR", "SHORT", "NONE", "AMBIGUOUS", "UNSUPPORTED", "MALFORMED"};

// sigax_scaffold_host, then ">scaffold-<n> unitigs=<k> gaps=<k - 1>[ circular=<closing gap>]" and the bases per scaffold, and
// one line "scaffold-<n>\tunitig-<u>\t<+|->\t<offset>\t<gap before>" per placement (0 before a scaffold's first).  With
// rq.index the gaps are filled first (sigax_gapfill_host): the bases, the offsets and the gaps before are the new ones, every
// header ends in " filled=<gaps filled>", and rq.gaps gets one line per gap:
// "GP\tscaffold-<n>\tunitig-<left>\tunitig-<right>\t<laid>\t<class>\t<forward walk>\t<reverse walk>\t<+|->\t<fill>\t<offset>"
// (the offsets of the gapfill call's tables).  With rq.joinIndex overlapping neighbours are then joined (sigax_join_host): the
// bases and the offsets are the new ones, the gap before is signed, -<overlap> for a joined pair, every header ends in
// " joined=<gaps joined>", and rq.joins gets one line per gap:
// "JN\tscaffold-<n>\tunitig-<left>\tunitig-<right>\t<laid>\t<class>\t<overlap>\t<matches>\t<windows>\t<offset>"
// With rq.joinMismatches > 0 the join is sigax_join_approx_host: the headers go on with " corrected=<columns taken from the right
// neighbour>" and every JN line with "\t<mismatches>\t<taken from the right>"
std::string run_scaffold(int device, uint64_t n_unitigs, const uint64_t* seq_offs, const uint32_t* uflags, const char* useqs,
                         const sigax_pair_link* links, uint64_t n_links, const uint64_t status24[24], const ScaffoldRequest& rq,
                         uint64_t status16[16], uint64_t gap24[24], uint64_t join24[24]) {
  if (!rq.haveInsertSize && status24[14] == 0)
    return "no pair of the library's orientation lies inside a unitig: there is no insert size to estimate the gaps from; give --insert-size";
  sigax_scaffold_opts opts;
  opts.flags = rq.haveInsertSize ? 0u : SIGAX_SCAFFOLD_INSERT_FROM_STATUS;
  opts.min_pairs = rq.minPairs;
  opts.link_ratio = rq.linkRatio;
  opts.min_unitig_bases = rq.minUnitigBases;
  opts.insert_size = rq.haveInsertSize ? rq.insertSize : 0;
  opts.min_gap = rq.minGap;
  opts.max_gap = rq.maxGap;
  uint64_t ns = 0, *sc_offs = nullptr, *sc_lay = nullptr;
  uint32_t* sc_flags = nullptr;
  sigax_placement* lay = nullptr;
  char* seqs = nullptr;
  if (sigax_scaffold_host(device, n_unitigs, seq_offs, uflags, useqs, links, n_links, status24, &opts, &ns, &sc_offs, &sc_lay, &sc_flags, &lay, &seqs,
                          status16) != SIGAX_OK)
    return std::string("scaffold failed: ") + sigax_last_error();
  std::string fa, lt, gt, jt;
  std::vector<uint64_t> filled, joined, corrected;
  if (rq.index) {
    sigax_gapfill_opts go = {0u, rq.gapKmer, rq.gapMinCount, rq.gapSlack, rq.gapMaxFill, 0u};
    uint64_t *offs2 = nullptr, ng = 0, st[24];
    sigax_placement* lay2 = nullptr;
    char* seqs2 = nullptr;
    sigax_gap* gaps = nullptr;
    if (sigax_gapfill_host(rq.index, n_unitigs, seq_offs, useqs, ns, sc_lay, lay, &go, SIGAX_GAPFILL_AUTO, &offs2, &lay2, &seqs2, &gaps, &ng, st) !=
        SIGAX_OK) {
      sigax_free(sc_offs);
      sigax_free(sc_lay);
      sigax_free(sc_flags);
      sigax_free(lay);
      sigax_free(seqs);
      return std::string("gap filling failed: ") + sigax_last_error();
    }
    sigax_free(sc_offs);
    sigax_free(lay);
    sigax_free(seqs);
    sc_offs = offs2;
    lay = lay2;
    seqs = seqs2;
    filled.assign(ns, 0);
    for (uint64_t g = 0; g < ng; ++g) {
      const sigax_gap& x = gaps[g];
      if (x.cls == SIGAX_GAP_FILLED && x.scaffold < ns) ++filled[x.scaffold];
      gt += "GP\tscaffold-";
      append_u64(gt, x.scaffold);
      gt += "\tunitig-";
      append_u64(gt, x.left);
      gt += "\tunitig-";
      append_u64(gt, x.right);
      gt += '\t';
      append_u64(gt, x.laid);
      gt += '\t';
      gt += gap_class(x.cls);
      gt += '\t';
      gt += gap_class(x.fwd);
      gt += '\t';
      gt += gap_class(x.rev);
      gt += x.dir ? "\t-\t" : "\t+\t";
      append_u64(gt, x.fill);
      gt += '\t';
      append_u64(gt, x.offset);
      gt += '\n';
    }
    sigax_free(gaps);
    if (gap24)
      for (int k = 0; k < 24; ++k) gap24[k] = st[k];
  }
  if (rq.joinIndex) {
    sigax_join_opts jo = {0u, rq.joinMinOverlap, rq.joinMaxOverlap, rq.joinSlack, rq.joinKmer, rq.joinMinCount, 0u};
    sigax_join_approx_opts ao = {0u, rq.joinMinOverlap, rq.joinMaxOverlap, rq.joinSlack, rq.joinKmer, rq.joinMinCount, rq.joinMismatches,
                                 rq.joinMismatchPermille, 0u};
    uint64_t *offs2 = nullptr, nj = 0, st[24] = {0};
    sigax_placement* lay2 = nullptr;
    char* seqs2 = nullptr;
    sigax_join* recs = nullptr;
    uint32_t* mm = nullptr;  // with --join-mismatches: per gap mismatches | taken from the right << 8 | approximate << 16
    const int rc = rq.joinMismatches
                       ? sigax_join_approx_host(rq.joinIndex, n_unitigs, seq_offs, ns, sc_offs, sc_lay, lay, seqs, &ao, &offs2, &lay2, &seqs2, &recs, &nj, &mm, st)
                       : sigax_join_host(rq.joinIndex, n_unitigs, seq_offs, ns, sc_offs, sc_lay, lay, seqs, &jo, &offs2, &lay2, &seqs2, &recs, &nj, st);
    if (rc != SIGAX_OK) {
      sigax_free(sc_offs);
      sigax_free(sc_lay);
      sigax_free(sc_flags);
      sigax_free(lay);
      sigax_free(seqs);
      return std::string("joining overlaps failed: ") + sigax_last_error();
    }
    sigax_free(sc_offs);
    sigax_free(lay);
    sigax_free(seqs);
    sc_offs = offs2;
    lay = lay2;
    seqs = seqs2;
    joined.assign(ns, 0);
    corrected.assign(ns, 0);
    for (uint64_t g = 0; g < nj; ++g) {
      const sigax_join& x = recs[g];
      if (x.cls == SIGAX_JOIN_JOINED && x.scaffold < ns) ++joined[x.scaffold];
      if (mm && x.cls == SIGAX_JOIN_JOINED && x.scaffold < ns) corrected[x.scaffold] += (mm[g] >> 8) & 0xFFu;
      jt += "JN\tscaffold-";
      append_u64(jt, x.scaffold);
      jt += "\tunitig-";
      append_u64(jt, x.left);
      jt += "\tunitig-";
      append_u64(jt, x.right);
      jt += '\t';
      append_u64(jt, x.laid);
      jt += '\t';
      jt += x.cls < 8 ? kJoinClasses[x.cls] : "?";
      jt += '\t';
      append_u64(jt, x.overlap);
      jt += '\t';
      append_u64(jt, x.matches);
      jt += '\t';
      append_u64(jt, x.windows);
      jt += '\t';
      append_u64(jt, x.offset);
      if (mm) {
        jt += '\t';
        append_u64(jt, mm[g] & 0xFFu);
        jt += '\t';
        append_u64(jt, (mm[g] >> 8) & 0xFFu);
      }
      jt += '\n';
    }
    sigax_free(recs);
    sigax_free(mm);
    if (join24)
      for (int k = 0; k < 24; ++k) join24[k] = st[k];
  }
  for (uint64_t s = 0; s < ns; ++s) {
    const uint64_t k = sc_lay[s + 1] - sc_lay[s];
    fa += ">scaffold-";
    append_u64(fa, s);
    fa += " unitigs=";
    append_u64(fa, k);
    fa += " gaps=";
    append_u64(fa, k ? k - 1 : 0);
    if (sc_flags[s] & 1u) {
      fa += " circular=";
      append_u64(fa, sc_flags[s] >> 1);
    }
    if (rq.index) {
      fa += " filled=";
      append_u64(fa, filled[s]);
    }
    if (rq.joinIndex) {
      fa += " joined=";
      append_u64(fa, joined[s]);
      if (rq.joinMismatches) {
        fa += " corrected=";
        append_u64(fa, corrected[s]);
      }
    }
    fa += '\n';
    fa.append(seqs + sc_offs[s], sc_offs[s + 1] - sc_offs[s]);
    fa += '\n';
    for (uint64_t p = sc_lay[s]; p < sc_lay[s + 1]; ++p) {
      const sigax_placement& x = lay[p];
      lt += "scaffold-";
      append_u64(lt, s);
      lt += "\tunitig-";
      append_u64(lt, x.read);
      lt += (x.flags & SIGAX_PLACED_REV) ? "\t-\t" : "\t+\t";
      append_u64(lt, x.offset);
      lt += '\t';
      uint64_t gap = 0;
      if (p > sc_lay[s]) {
        const sigax_placement& b = lay[p - 1];
        gap = x.offset - b.offset - (seq_offs[b.read + 1] - seq_offs[b.read]);
      }
      if (rq.joinIndex && (int64_t)gap < 0) {  // neighbours that were joined: the overlap, signed
        lt += '-';
        gap = 0 - gap;
      }
      append_u64(lt, gap);
      lt += '\n';
    }
  }
  sigax_free(sc_offs);
  sigax_free(sc_lay);
  sigax_free(sc_flags);
  sigax_free(lay);
  sigax_free(seqs);
  if (!write_file(rq.fasta, fa)) return "Failed to write " + rq.fasta;
  if (!rq.layout.empty() && !write_file(rq.layout, lt)) return "Failed to write " + rq.layout;
  if (rq.index && !rq.gaps.empty() && !write_file(rq.gaps, gt)) return "Failed to write " + rq.gaps;
  if (rq.joinIndex && !rq.joins.empty() && !write_file(rq.joins, jt)) return "Failed to write " + rq.joins;
  return std::string();
}
}  // namespace

std::string run_pairs(int device, const std::vector<uint32_t>& mate, const std::vector<uint32_t>& lengths, uint64_t n_unitigs,
                      const uint64_t* seq_offs, const uint64_t* lay_offs, const uint32_t* uflags, const sigax_placement* layout,
                      const PairsRequest& rq, uint64_t status24[24], uint64_t* insert_size, uint64_t* delta, const ScaffoldRequest* sc,
                      const char* useqs, uint64_t status16[16], uint64_t gap24[24], uint64_t join24[24]) {
  sigax_pairs_opts opts;
  opts.flags = rq.outward ? SIGAX_PAIRS_OUTWARD : 0u;
  opts.hist_bins = rq.bins;
  opts.hist_shift = rq.shift;
  opts.reserved = 0;
  opts.max_span = rq.maxSpan;
  uint64_t* hist = nullptr;
  sigax_pair_link* links = nullptr;
  if (sigax_unitigs_pairs_host(device, mate.data(), lengths.data(), mate.size(), n_unitigs, seq_offs, lay_offs, uflags, layout, &opts, &hist, &links,
                               status24) != SIGAX_OK)
    return std::string("pairs failed: ") + sigax_last_error();
  double span_mean = 0, span_sd = 0;
  sigax_pairs_estimate(status24, insert_size, delta, &span_mean, &span_sd);
  // {"pairs": {<the 24 counts by name>, "insert_size", "delta", "span_mean", "span_sd", "hist_bins", "hist_shift", "histogram":
  // [[bin, pairs], ...]}} and a newline; the histogram lists the non-empty bins in ascending order
  std::string t = "{\"pairs\": {";
  for (int k = 0; k < 24; ++k) {
    t += '"';
    t += kStatusNames[k];
    t += "\": ";
    append_u64(t, status24[k]);
    t += ", ";
  }
  t += "\"insert_size\": ";
  append_u64(t, *insert_size);
  t += ", \"delta\": ";
  append_u64(t, *delta);
  t += ", \"span_mean\": ";
  append_double(t, span_mean);
  t += ", \"span_sd\": ";
  append_double(t, span_sd);
  if (rq.haveContainedMates) {
    t += ", \"contained_mates\": ";
    append_u64(t, rq.containedMates);
  }
  t += ", \"hist_bins\": ";
  append_u64(t, rq.bins);
  t += ", \"hist_shift\": ";
  append_u64(t, rq.shift);
  t += ", \"histogram\": [";
  bool any = false;
  for (uint32_t b = 0; b < rq.bins; ++b)
    if (hist[b]) {
      if (any) t += ", ";
      any = true;
      t += '[';
      append_u64(t, b);
      t += ", ";
      append_u64(t, hist[b]);
      t += ']';
    }
  t += "]}}\n";
  bool ok = write_file(rq.json, t);
  std::string bad = ok ? "" : rq.json;
  if (ok && !rq.links.empty()) {
    // "LK\tunitig-<u>\t<B|E>\tunitig-<v>\t<B|E>\t<count>\t<min_span>\t<sum_span>", in record order
    t.clear();
    for (uint64_t i = 0; i < status24[22]; ++i) {
      const sigax_pair_link& l = links[i];
      t += "LK\tunitig-";
      append_u64(t, l.a >> 1);
      t += (l.a & 1u) ? "\tE\tunitig-" : "\tB\tunitig-";
      append_u64(t, l.b >> 1);
      t += (l.b & 1u) ? "\tE\t" : "\tB\t";
      append_u64(t, l.count);
      t += '\t';
      append_u64(t, l.min_span);
      t += '\t';
      append_u64(t, l.sum_span);
      t += '\n';
    }
    ok = write_file(rq.links, t);
    if (!ok) bad = rq.links;
  }
  std::string e = ok ? std::string() : "Failed to write " + bad;
  if (ok && sc && !sc->fasta.empty()) e = run_scaffold(device, n_unitigs, seq_offs, uflags, useqs, links, status24[22], status24, *sc, status16, gap24, join24);
  sigax_free(hist);
  sigax_free(links);
  return e;
}

}  // namespace sigah
