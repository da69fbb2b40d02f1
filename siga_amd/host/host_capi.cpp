// siga_amd/host/host_capi.cpp -- the C entry points of libsiga_host.so (siga_amd/host.py binds them through ctypes).
#include <algorithm>
#include <cstdio>
#include <thread>

#include "asqg_text.hpp"
#include "host_util.hpp"
#include "out_file.hpp"
#include "reads.hpp"
#include "siga_host.hpp"

// FMIndex::load (both strands) or FMIndex::loadForward (<prefix>.bwt alone); false: the message is in err
static bool load_index(sigah::FMIndex& fmi, const char* prefix, int device, bool forward_only, char* err, uint64_t errcap) {
  if (forward_only ? sigah::FMIndex::loadForward(prefix, fmi, device) : sigah::FMIndex::load(prefix, fmi, device)) return true;
  if (err && errcap) snprintf(err, errcap, "Failed to load FMIndex from %s: %s", prefix, sigax_last_error());
  return false;
}

// ------------------------------------------------------------------------------------------------------
// C entry points for tests/bench (ctypes)
// ------------------------------------------------------------------------------------------------------
extern "C" {

// `siga index` for in-memory reads: writes <prefix>.{bwt,sai,rbwt,rsai}; returns 0 or -1 (message in err)
int sigah_index_build(const char* seqs, const uint64_t* offs, uint64_t n_reads, const char* prefix, int threads, char* err,
                      uint64_t errcap) {
  sigah::StrandIndex fwd, rev;
  std::string e1, e2;
  bool ok1 = false, ok2 = false;
  if (threads == 2) {  // one SA-IS per strand, side by side
    std::thread t([&] { ok2 = sigah::BuildStrandIndex(seqs, offs, n_reads, true, &rev, &e2); });
    ok1 = sigah::BuildStrandIndex(seqs, offs, n_reads, false, &fwd, &e1);
    t.join();
  } else {  // 1 thread: SA-IS; more: the multi-threaded bucket sort, one strand after the other
    ok1 = sigah::BuildStrandIndex(seqs, offs, n_reads, false, &fwd, &e1, (unsigned)std::max(threads, 1));
    ok2 = sigah::BuildStrandIndex(seqs, offs, n_reads, true, &rev, &e2, (unsigned)std::max(threads, 1));
  }
  std::string p(prefix);
  if (ok1 && ok2) {
    ok1 = fwd.writeSAI(p + ".sai") && fwd.writeBWT(p + ".bwt");
    ok2 = rev.writeSAI(p + ".rsai") && rev.writeBWT(p + ".rbwt");
    if (!ok1 || !ok2) e1 = "cannot write index files with prefix " + p;
  }
  if (!(ok1 && ok2)) {
    if (err && errcap) snprintf(err, errcap, "%s", (e1.empty() ? e2 : e1).c_str());
    return -1;
  }
  return 0;
}

// `siga index` on the GPU: both strands through sigax_build_strand; an input too repetitive for the device sort is
// built by the host SA-IS instead (said on stderr).  device < 0: host builder only.
int sigah_index_build_dev(const char* seqs, const uint64_t* offs, uint64_t n_reads, const char* prefix, int device, int threads,
                          int do_fwd, int do_rev, char* err, uint64_t errcap) {
  if (device < 0) {
    if (do_fwd && do_rev) return sigah_index_build(seqs, offs, n_reads, prefix, threads, err, errcap);
  }
  std::string p(prefix), e;
  // the files of one strand are written on a side thread while the other strand is sorted; the second sort works in the
  // device memory of the first
  struct Session {
    Session() { sigax_build_session(1); }
    ~Session() { sigax_build_session(0); }
  } session;
  std::thread writer;
  bool write_ok = true;
  auto join_writer = [&] {
    if (writer.joinable()) writer.join();
  };
  for (int rev = 0; rev < 2; ++rev) {
    if ((rev == 0 && !do_fwd) || (rev == 1 && !do_rev)) continue;
    auto ix = std::make_shared<sigah::StrandIndex>();
    int rc = 0;
    bool ok = device >= 0 && sigah::BuildStrandIndexGPU(seqs, offs, n_reads, rev != 0, device, ix.get(), &e, &rc);
    if (!ok && (device < 0 || rc == SIGAX_E_CAPACITY)) {
      if (device >= 0) fprintf(stderr, "siga index: %s; using the host suffix sorter\n", e.c_str());
      ok = sigah::BuildStrandIndex(seqs, offs, n_reads, rev != 0, ix.get(), &e, (unsigned)std::max(threads, 1));
    }
    if (!ok) {
      join_writer();
      if (err && errcap) snprintf(err, errcap, "%s", e.c_str());
      return -1;
    }
    join_writer();
    writer = std::thread([ix, p, rev, &write_ok] {  // the strand's two files side by side
      bool ok_sai = true;
      std::thread sai([&] { ok_sai = ix->writeSAI(p + (rev ? ".rsai" : ".sai")); });
      const bool ok_bwt = ix->writeBWT(p + (rev ? ".rbwt" : ".bwt"));
      sai.join();
      if (!(ok_sai && ok_bwt)) write_ok = false;
    });
  }
  join_writer();
  if (!write_ok) {
    if (err && errcap) snprintf(err, errcap, "cannot write index files with prefix %s", p.c_str());
    return -1;
  }
  return 0;
}

// `siga index READS` with the device builder (device < 0: host builder)
int sigah_index_file_dev(const char* reads_path, const char* prefix, int device, int threads, int do_fwd, int do_rev, char* err,
                         uint64_t errcap) {
  const sigah::HostSettings hs;
  sigah::PhaseTimer pt(hs.timing);
  sigah::ReadStore rs;
  if (!sigah::LoadReads(reads_path, &rs, sigah::host_threads((size_t)std::max(threads, 1), hs), hs)) {
    if (err && errcap) snprintf(err, errcap, "Failed to open input file %s", reads_path);
    return -1;
  }
  pt.lap("parse reads");
  int rc = sigah_index_build_dev(rs.seqs.data(), rs.offs.data(), rs.size(), prefix, device, threads, do_fwd, do_rev, err, errcap);
  pt.lap("suffix sort + index files");
  return rc;
}

// `siga index -a sais READS`: the SAISBuilder order (src/suffix_array_builder.cpp:31-172), host suffix sorter only
int sigah_index_file_sais(const char* reads_path, const char* prefix, int threads, int do_fwd, int do_rev, char* err, uint64_t errcap) {
  const sigah::HostSettings hs;
  sigah::ReadStore rs;
  if (!sigah::LoadReads(reads_path, &rs, sigah::host_threads((size_t)std::max(threads, 1), hs), hs)) {
    if (err && errcap) snprintf(err, errcap, "Failed to open input file %s", reads_path);
    return -1;
  }
  const std::string p(prefix);
  for (int rev = 0; rev < 2; ++rev) {
    if ((rev == 0 && !do_fwd) || (rev == 1 && !do_rev)) continue;
    sigah::StrandIndex ix;
    std::string e;
    if (!sigah::BuildStrandIndex(rs.seqs.data(), rs.offs.data(), rs.size(), rev != 0, &ix, &e, (unsigned)std::max(threads, 1), true)) {
      if (err && errcap) snprintf(err, errcap, "%s", e.c_str());
      return -1;
    }
    if (!(ix.writeSAI(p + (rev ? ".rsai" : ".sai")) && ix.writeBWT(p + (rev ? ".rbwt" : ".bwt")))) {
      if (err && errcap) snprintf(err, errcap, "cannot write index files with prefix %s", p.c_str());
      return -1;
    }
  }
  return 0;
}

// `siga index READS`
int sigah_index_file(const char* reads_path, const char* prefix, int threads, char* err, uint64_t errcap) {
  sigah::DNASeqList reads;
  if (!sigah::ReadDNASequences(reads_path, reads, 0)) {
    if (err && errcap) snprintf(err, errcap, "Failed to open input file %s", reads_path);
    return -1;
  }
  std::string seqs;
  std::vector<uint64_t> offs(1, 0);
  for (auto& r : reads) {
    seqs += r.seq;
    offs.push_back(seqs.size());
  }
  return sigah_index_build(seqs.data(), offs.data(), reads.size(), prefix, threads, err, errcap);
}

// `siga overlap`: FMIndex::load + OverlapBuilder::build, reads sharded over `gpus` GPUs starting at `device`
int sigah_overlap_file_gpus(const char* reads_path, const char* prefix, uint64_t min_overlap, const char* output, int irreducible,
                            int rc, uint64_t threads, uint64_t batch, int device, int gpus, char* err, uint64_t errcap) {
  sigah::FMIndex fmi;
  if (!load_index(fmi, prefix, device, false, err, errcap)) return -1;
  sigah::OverlapBuilder builder(&fmi, prefix, irreducible != 0, rc != 0);
  builder.setGPUs(gpus);
  if (!builder.build(reads_path, min_overlap, output, threads, batch)) {
    if (err && errcap) snprintf(err, errcap, "%s", builder.error().c_str());
    return -1;
  }
  return 0;
}

// `siga overlap` on one GPU (what a default-constructed builder runs on: OverlapBuilder::_gpus starts as 1)
int sigah_overlap_file(const char* reads_path, const char* prefix, uint64_t min_overlap, const char* output, int irreducible,
                       int rc, uint64_t threads, uint64_t batch, int device, char* err, uint64_t errcap) {
  return sigah_overlap_file_gpus(reads_path, prefix, min_overlap, output, irreducible, rc, threads, batch, device, 1, err, errcap);
}

// `siga overlap -e`: FMIndex::loadForwardSai + MismatchOverlapper::run; status8 (may be NULL) receives the status words of
// sigax_mmoverlap_batch
// containments (may be NULL or empty): `--containments FILE`
int sigah_overlap_mismatch_containments_file(const char* reads_path, const char* prefix, const char* output, const char* containments,
                                             const sigax_mmo_params* params, uint64_t threads, int device, uint64_t* status8, char* err,
                                             uint64_t errcap) {
  sigah::FMIndex fmi;
  if (!params) {
    if (err && errcap) snprintf(err, errcap, "params is NULL");
    return -1;
  }
  if (!sigah::FMIndex::loadForwardSai(prefix, fmi, device)) {
    if (err && errcap) snprintf(err, errcap, "Failed to load FMIndex from %s: %s", prefix, sigax_last_error());
    return -1;
  }
  sigah::MismatchOverlapper finder(*params);
  if (containments && *containments) finder.setContainments(containments);
  if (!finder.run(fmi, reads_path, output, (size_t)threads)) {
    if (err && errcap) snprintf(err, errcap, "%s", finder.error().c_str());
    return -1;
  }
  if (status8)
    for (int k = 0; k < 8; ++k) status8[k] = finder.status()[k];
  return 0;
}

int sigah_overlap_mismatch_file(const char* reads_path, const char* prefix, const char* output, const sigax_mmo_params* params, uint64_t threads,
                                int device, uint64_t* status8, char* err, uint64_t errcap) {
  return sigah_overlap_mismatch_containments_file(reads_path, prefix, output, nullptr, params, threads, device, status8, err, errcap);
}

// `siga rmdup`: FMIndex::load + OverlapBuilder::rmdup
int sigah_rmdup_file(const char* reads_path, const char* prefix, const char* output, const char* duplicates, int device,
                     char* err, uint64_t errcap) {
  sigah::FMIndex fmi;
  if (!load_index(fmi, prefix, device, false, err, errcap)) return -1;
  sigah::OverlapBuilder builder(&fmi, prefix);
  if (!builder.rmdup(reads_path, output, duplicates)) {
    if (err && errcap) snprintf(err, errcap, "%s", builder.error().c_str());
    return -1;
  }
  return 0;
}

// `siga correct`: FMIndex::load(prefix.bwt) + CorrectProcessor::process
int sigah_correct_file(const char* reads_path, const char* prefix, const char* output, uint64_t k, uint64_t threshold,
                       uint64_t rounds, uint64_t offset, int device, char* err, uint64_t errcap) {
  sigah::FMIndex fmi;
  if (!load_index(fmi, prefix, device, true, err, errcap)) return -1;
  sigah::CorrectProcessor::Options o;
  o.kmerSize = k; o.kmerThreshold = threshold; o.kmerRounds = rounds; o.kmerCountOffset = offset;
  sigah::CorrectProcessor proc(o);
  if (!proc.process(fmi, reads_path, output)) {
    if (err && errcap) snprintf(err, errcap, "%s", proc.error().c_str());
    return -1;
  }
  return 0;
}

// `siga correct -a overlap`: FMIndex::loadForwardSai + CorrectProcessor::process with the pile-up; status8 (may be NULL) receives
// the status words of sigax_pileup_batch added up over the batches
int sigah_correct_overlap_file(const char* reads_path, const char* prefix, const char* output, const sigax_pile_params* params,
                               uint64_t rounds, int device, uint64_t* status8, char* err, uint64_t errcap) {
  sigah::FMIndex fmi;
  if (!sigah::FMIndex::loadForwardSai(prefix, fmi, device)) {
    if (err && errcap) snprintf(err, errcap, "Failed to load FMIndex from %s: %s", prefix, sigax_last_error());
    return -1;
  }
  sigah::CorrectProcessor::Options o;
  o.overlap = true;
  if (params) o.pile = *params;
  o.rounds = rounds;
  sigah::CorrectProcessor proc(o);
  if (!proc.process(fmi, reads_path, output)) {
    if (err && errcap) snprintf(err, errcap, "%s", proc.error().c_str());
    return -1;
  }
  if (status8)
    for (int k = 0; k < 8; ++k) status8[k] = proc.pileStatus()[k];
  return 0;
}

// `siga match`: FMIndex::load(prefix.bwt) + Matcher::run over n_paths inputs; out_path "" = stdout; max_length ~0 = no limit;
// batch_reads 0 = device batches sized from the free memory
int sigah_match_files(const char* const* paths, uint64_t n_paths, const char* prefix, uint64_t max_length, int rc, int device,
                      const char* out_path, uint64_t batch_reads, char* err, uint64_t errcap) {
  sigah::FMIndex fmi;
  if (!load_index(fmi, prefix, device, true, err, errcap)) return -1;
  std::vector<std::string> inputs;
  for (uint64_t i = 0; i < n_paths; ++i) inputs.push_back(paths[i]);
  sigah::Matcher matcher(max_length, rc != 0);
  if (!matcher.run(fmi, inputs, out_path ? out_path : "", 1, (size_t)batch_reads)) {
    if (err && errcap) snprintf(err, errcap, "%s", matcher.error().c_str());
    return -1;
  }
  return 0;
}

// `siga locate`: FMIndex::loadForwardSai + Locator::run over n_paths inputs; out_path "" = stdout; batch_queries 0 = the default
int sigah_locate_files(const char* const* paths, uint64_t n_paths, const char* prefix, uint32_t max_hits, uint32_t max_length, int rc,
                       int device, const char* out_path, uint64_t batch_queries, char* err, uint64_t errcap) {
  sigah::FMIndex fmi;
  if (!sigah::FMIndex::loadForwardSai(prefix, fmi, device)) {
    if (err && errcap) snprintf(err, errcap, "Failed to load FMIndex from %s: %s", prefix, sigax_last_error());
    return -1;
  }
  std::vector<std::string> inputs;
  for (uint64_t i = 0; i < n_paths; ++i) inputs.push_back(paths[i]);
  sigah::Locator locator(max_hits, max_length, rc != 0);
  if (!locator.run(fmi, inputs, out_path ? out_path : "", 1, (size_t)batch_queries)) {
    if (err && errcap) snprintf(err, errcap, "%s", locator.error().c_str());
    return -1;
  }
  return 0;
}

// `siga unitig`: FMIndex::load + Unitigger::run; fasta_path "" = stdout, layout_path "" = no layout file; piece_reads = reads per
// overlap call (0: the default)
static int unitig_file(sigah::Unitigger& unitigger, const char* reads_path, const char* prefix, uint64_t min_overlap, int device,
                       const char* fasta_path, const char* layout_path, uint64_t piece_reads, char* err, uint64_t errcap) {
  sigah::FMIndex fmi;
  if (!sigah::FMIndex::load(prefix, fmi, device)) {
    if (err && errcap) snprintf(err, errcap, "Failed to load FMIndex from %s: %s", prefix, sigax_last_error());
    return -1;
  }
  unitigger.setPieceReads((size_t)piece_reads);
  if (!unitigger.run(fmi, reads_path, (size_t)min_overlap, fasta_path ? fasta_path : "", layout_path ? layout_path : "")) {
    if (err && errcap) snprintf(err, errcap, "%s", unitigger.error().c_str());
    return -1;
  }
  return 0;
}
int sigah_unitig_file(const char* reads_path, const char* prefix, uint64_t min_overlap, int irreducible, int rc, int device,
                      const char* fasta_path, const char* layout_path, uint64_t piece_reads, char* err, uint64_t errcap) {
  sigah::Unitigger unitigger(irreducible != 0, rc != 0);
  return unitig_file(unitigger, reads_path, prefix, min_overlap, device, fasta_path, layout_path, piece_reads, err, errcap);
}
// ... with tip trimming (cut_terminal rounds, min_branch_coverage -1: no coverage test), the unitig graph (graph_path "" = none)
// and the removed reads (removed_path "" = none); status8 (unless NULL) = {unitigs, bases, merged, circular, trim rounds, islands,
// dead ends, reads removed}
int sigah_unitig_trim_file(const char* reads_path, const char* prefix, uint64_t min_overlap, int irreducible, int rc, int device,
                           const char* fasta_path, const char* layout_path, uint64_t piece_reads, uint64_t cut_terminal,
                           uint64_t min_branch_length, int64_t min_branch_coverage, const char* graph_path, const char* removed_path,
                           uint64_t* status8, char* err, uint64_t errcap) {
  sigah::Unitigger unitigger(irreducible != 0, rc != 0);
  unitigger.setTrim((size_t)cut_terminal, (size_t)min_branch_length, (long)min_branch_coverage);
  unitigger.setGraph(graph_path ? graph_path : "");
  unitigger.setRemoved(removed_path ? removed_path : "");
  const int r = unitig_file(unitigger, reads_path, prefix, min_overlap, device, fasta_path, layout_path, piece_reads, err, errcap);
  if (r == 0 && status8) {
    const uint64_t s[8] = {unitigger.unitigs(), unitigger.bases(),    unitigger.merged(),   unitigger.cycles(),
                           unitigger.trimRounds(), unitigger.islands(), unitigger.deadEnds(), unitigger.readsRemoved()};
    for (int k = 0; k < 8; ++k) status8[k] = s[k];
  }
  return r;
}
// ... and with non-maximal overlap cutting in the rounds (delta 0 = none; num_reads 0 = the reads of the file) and the cut records
// (cut_path "" = none); status10 (unless NULL) = status8, then {records cut, rounds that cut}
int sigah_unitig_prune_file(const char* reads_path, const char* prefix, uint64_t min_overlap, int irreducible, int rc, int device,
                            const char* fasta_path, const char* layout_path, uint64_t piece_reads, uint64_t cut_terminal,
                            uint64_t min_branch_length, int64_t min_branch_coverage, const char* graph_path, const char* removed_path,
                            uint64_t delta, int careful, uint64_t num_reads, uint64_t genome_size, double uniq_threshold,
                            const char* cut_path, uint64_t* status10, char* err, uint64_t errcap) {
  sigah::Unitigger unitigger(irreducible != 0, rc != 0);
  unitigger.setTrim((size_t)cut_terminal, (size_t)min_branch_length, (long)min_branch_coverage);
  unitigger.setGraph(graph_path ? graph_path : "");
  unitigger.setRemoved(removed_path ? removed_path : "");
  unitigger.setMaxOverlap((size_t)delta, careful != 0, (size_t)num_reads, (size_t)genome_size, uniq_threshold);
  unitigger.setCutEdges(cut_path ? cut_path : "");
  const int r = unitig_file(unitigger, reads_path, prefix, min_overlap, device, fasta_path, layout_path, piece_reads, err, errcap);
  if (r == 0 && status10) {
    const uint64_t s[10] = {unitigger.unitigs(),    unitigger.bases(),   unitigger.merged(),   unitigger.cycles(),       unitigger.trimRounds(),
                            unitigger.islands(),    unitigger.deadEnds(), unitigger.readsRemoved(), unitigger.recordsCut(), unitigger.cutRounds()};
    for (int k = 0; k < 10; ++k) status10[k] = s[k];
  }
  return r;
}
// ... and with chimeric unitig removal as the last step of a round (min_chimeric_length 0 = none; min_chimeric_coverage -1: no
// coverage test) and the reads it removed (chimeric_path "" = none); status12 (unless NULL) = status10, then {chimeric unitigs,
// their reads}
int sigah_unitig_chimeric_file(const char* reads_path, const char* prefix, uint64_t min_overlap, int irreducible, int rc, int device,
                               const char* fasta_path, const char* layout_path, uint64_t piece_reads, uint64_t cut_terminal,
                               uint64_t min_branch_length, int64_t min_branch_coverage, const char* graph_path, const char* removed_path,
                               uint64_t delta, int careful, uint64_t num_reads, uint64_t genome_size, double uniq_threshold,
                               const char* cut_path, uint64_t min_chimeric_length, int64_t min_chimeric_coverage, uint64_t chimeric_delta,
                               double chimeric_threshold, const char* chimeric_path, uint64_t* status12, char* err, uint64_t errcap) {
  sigah::Unitigger unitigger(irreducible != 0, rc != 0);
  unitigger.setTrim((size_t)cut_terminal, (size_t)min_branch_length, (long)min_branch_coverage);
  unitigger.setGraph(graph_path ? graph_path : "");
  unitigger.setRemoved(removed_path ? removed_path : "");
  unitigger.setMaxOverlap((size_t)delta, careful != 0, (size_t)num_reads, (size_t)genome_size, uniq_threshold);
  unitigger.setCutEdges(cut_path ? cut_path : "");
  unitigger.setChimeric((size_t)min_chimeric_length, (long)min_chimeric_coverage, (size_t)chimeric_delta, chimeric_threshold);
  unitigger.setChimericOut(chimeric_path ? chimeric_path : "");
  const int r = unitig_file(unitigger, reads_path, prefix, min_overlap, device, fasta_path, layout_path, piece_reads, err, errcap);
  if (r == 0 && status12) {
    const uint64_t s[12] = {unitigger.unitigs(),  unitigger.bases(),        unitigger.merged(),     unitigger.cycles(),    unitigger.trimRounds(),
                            unitigger.islands(),  unitigger.deadEnds(),     unitigger.readsRemoved(), unitigger.recordsCut(), unitigger.cutRounds(),
                            unitigger.chimericUnitigs(), unitigger.chimericReads()};
    for (int k = 0; k < 12; ++k) status12[k] = s[k];
  }
  return r;
}
// ... and with bubble popping between the trim and the chimeric step of a round (max_bubble_span 0 = none; bubble_divergence -1: no
// bases test) and the reads it removed (bubbles_path "" = none); status15 (unless NULL) = status12, then {arms popped, their reads,
// losers kept on divergence}
int sigah_unitig_bubble_file(const char* reads_path, const char* prefix, uint64_t min_overlap, int irreducible, int rc, int device,
                             const char* fasta_path, const char* layout_path, uint64_t piece_reads, uint64_t cut_terminal,
                             uint64_t min_branch_length, int64_t min_branch_coverage, const char* graph_path, const char* removed_path,
                             uint64_t delta, int careful, uint64_t num_reads, uint64_t genome_size, double uniq_threshold,
                             const char* cut_path, uint64_t min_chimeric_length, int64_t min_chimeric_coverage, uint64_t chimeric_delta,
                             double chimeric_threshold, const char* chimeric_path, uint64_t max_bubble_span, int64_t bubble_divergence,
                             const char* bubbles_path, uint64_t* status15, char* err, uint64_t errcap) {
  sigah::Unitigger unitigger(irreducible != 0, rc != 0);
  unitigger.setTrim((size_t)cut_terminal, (size_t)min_branch_length, (long)min_branch_coverage);
  unitigger.setGraph(graph_path ? graph_path : "");
  unitigger.setRemoved(removed_path ? removed_path : "");
  unitigger.setMaxOverlap((size_t)delta, careful != 0, (size_t)num_reads, (size_t)genome_size, uniq_threshold);
  unitigger.setCutEdges(cut_path ? cut_path : "");
  unitigger.setChimeric((size_t)min_chimeric_length, (long)min_chimeric_coverage, (size_t)chimeric_delta, chimeric_threshold);
  unitigger.setChimericOut(chimeric_path ? chimeric_path : "");
  unitigger.setBubble((size_t)max_bubble_span, (long)bubble_divergence);
  unitigger.setBubbleOut(bubbles_path ? bubbles_path : "");
  const int r = unitig_file(unitigger, reads_path, prefix, min_overlap, device, fasta_path, layout_path, piece_reads, err, errcap);
  if (r == 0 && status15) {
    const uint64_t s[15] = {unitigger.unitigs(),  unitigger.bases(),        unitigger.merged(),     unitigger.cycles(),    unitigger.trimRounds(),
                            unitigger.islands(),  unitigger.deadEnds(),     unitigger.readsRemoved(), unitigger.recordsCut(), unitigger.cutRounds(),
                            unitigger.chimericUnitigs(), unitigger.chimericReads(), unitigger.bubblesPopped(), unitigger.bubbleReads(),
                            unitigger.bubblesKept()};
    for (int k = 0; k < 15; ++k) status15[k] = s[k];
  }
  return r;
}
// ... and with indel bubble popping between the bubble and the chimeric step of a round (bubble_edits 0 = none; at most 31, and then
// max_bubble_span 1 to 4096); bubbles_path also lists the reads it removed ("name<TAB>round<TAB>indel"); status19 (unless NULL) =
// status15, then {arms the indel steps popped, their reads, compared losers kept, losers not compared}
int sigah_unitig_indel_file(const char* reads_path, const char* prefix, uint64_t min_overlap, int irreducible, int rc, int device,
                            const char* fasta_path, const char* layout_path, uint64_t piece_reads, uint64_t cut_terminal,
                            uint64_t min_branch_length, int64_t min_branch_coverage, const char* graph_path, const char* removed_path,
                            uint64_t delta, int careful, uint64_t num_reads, uint64_t genome_size, double uniq_threshold,
                            const char* cut_path, uint64_t min_chimeric_length, int64_t min_chimeric_coverage, uint64_t chimeric_delta,
                            double chimeric_threshold, const char* chimeric_path, uint64_t max_bubble_span, int64_t bubble_divergence,
                            const char* bubbles_path, uint64_t bubble_edits, uint64_t bubble_edit_permille, uint64_t* status19, char* err,
                            uint64_t errcap) {
  sigah::Unitigger unitigger(irreducible != 0, rc != 0);
  unitigger.setTrim((size_t)cut_terminal, (size_t)min_branch_length, (long)min_branch_coverage);
  unitigger.setGraph(graph_path ? graph_path : "");
  unitigger.setRemoved(removed_path ? removed_path : "");
  unitigger.setMaxOverlap((size_t)delta, careful != 0, (size_t)num_reads, (size_t)genome_size, uniq_threshold);
  unitigger.setCutEdges(cut_path ? cut_path : "");
  unitigger.setChimeric((size_t)min_chimeric_length, (long)min_chimeric_coverage, (size_t)chimeric_delta, chimeric_threshold);
  unitigger.setChimericOut(chimeric_path ? chimeric_path : "");
  unitigger.setBubble((size_t)max_bubble_span, (long)bubble_divergence);
  unitigger.setBubbleOut(bubbles_path ? bubbles_path : "");
  unitigger.setBubbleEdits((size_t)bubble_edits, (size_t)bubble_edit_permille);
  const int r = unitig_file(unitigger, reads_path, prefix, min_overlap, device, fasta_path, layout_path, piece_reads, err, errcap);
  if (r == 0 && status19) {
    const uint64_t s[19] = {unitigger.unitigs(),  unitigger.bases(),        unitigger.merged(),     unitigger.cycles(),    unitigger.trimRounds(),
                            unitigger.islands(),  unitigger.deadEnds(),     unitigger.readsRemoved(), unitigger.recordsCut(), unitigger.cutRounds(),
                            unitigger.chimericUnitigs(), unitigger.chimericReads(), unitigger.bubblesPopped(), unitigger.bubbleReads(),
                            unitigger.bubblesKept(), unitigger.indelsPopped(), unitigger.indelReads(), unitigger.indelsKept(),
                            unitigger.indelsNotCompared()};
    for (int k = 0; k < 19; ++k) status19[k] = s[k];
  }
  return r;
}

// ... and with the transitive reduction (reduce), mismatch overlaps in (error_permille >= 0: `siga unitig -e`; the four seed
// options as `siga overlap -e` takes them; contained_path "" = none) and the consensus pass (consensus < 0: on exactly with
// error_permille; min_votes); status24 (unless NULL) = status19, then {records transitive in the final graph, contained reads,
// columns the vote changed, columns of depth below 2, 0}
// ... and with the contained reads placed (place_contained: `--place-contained`, with error_permille only); status24[23] = the
// contained reads placed
int sigah_unitig_placed_file(const char* reads_path, const char* prefix, uint64_t min_overlap, int irreducible, int rc, int device,
                                const char* fasta_path, const char* layout_path, uint64_t piece_reads, uint64_t cut_terminal,
                                uint64_t min_branch_length, int64_t min_branch_coverage, const char* graph_path, const char* removed_path,
                                uint64_t delta, int careful, uint64_t num_reads, uint64_t genome_size, double uniq_threshold,
                                const char* cut_path, uint64_t min_chimeric_length, int64_t min_chimeric_coverage, uint64_t chimeric_delta,
                                double chimeric_threshold, const char* chimeric_path, uint64_t max_bubble_span, int64_t bubble_divergence,
                                const char* bubbles_path, uint64_t bubble_edits, uint64_t bubble_edit_permille, int reduce,
                                int64_t error_permille, uint64_t seed_length, uint64_t seed_stride, uint64_t max_seed_hits,
                                uint64_t max_candidates, int consensus, uint64_t min_votes, const char* contained_path, int place_contained,
                                uint64_t* status24, char* err, uint64_t errcap) {
  sigah::Unitigger unitigger(irreducible != 0, rc != 0);
  unitigger.setPlaceContained(place_contained != 0);
  unitigger.setTrim((size_t)cut_terminal, (size_t)min_branch_length, (long)min_branch_coverage);
  unitigger.setGraph(graph_path ? graph_path : "");
  unitigger.setRemoved(removed_path ? removed_path : "");
  unitigger.setMaxOverlap((size_t)delta, careful != 0, (size_t)num_reads, (size_t)genome_size, uniq_threshold);
  unitigger.setCutEdges(cut_path ? cut_path : "");
  unitigger.setChimeric((size_t)min_chimeric_length, (long)min_chimeric_coverage, (size_t)chimeric_delta, chimeric_threshold);
  unitigger.setChimericOut(chimeric_path ? chimeric_path : "");
  unitigger.setBubble((size_t)max_bubble_span, (long)bubble_divergence);
  unitigger.setBubbleOut(bubbles_path ? bubbles_path : "");
  unitigger.setBubbleEdits((size_t)bubble_edits, (size_t)bubble_edit_permille);
  unitigger.setReduce(reduce != 0);
  const bool mismatches = error_permille >= 0;
  auto u32 = [](uint64_t v) { return (uint32_t)std::min<uint64_t>(v, 0xFFFFFFFFull); };  // (the library names the field out of range)
  if (mismatches) {
    sigax_mmo_params p = sigah::MismatchOverlapper::defaults(u32((uint64_t)error_permille));
    p.seed_length = u32(seed_length);
    p.seed_stride = u32(seed_stride);
    p.max_seed_hits = u32(max_seed_hits);
    p.max_candidates = u32(max_candidates);
    p.min_overlap = u32(min_overlap);
    uint64_t probe = 0;
    if (sigax_mmoverlap_workspace(0, 0, &p, 0, &probe) != SIGAX_OK) {
      if (err && errcap) snprintf(err, errcap, "%s", sigax_last_error());
      return -1;
    }
    unitigger.setMismatch(p, contained_path ? contained_path : "");
  } else if (contained_path && contained_path[0]) {
    if (err && errcap) snprintf(err, errcap, "contained reads are only written with mismatch overlaps");
    return -1;
  }
  unitigger.setConsensus(consensus < 0 ? mismatches : consensus != 0, (size_t)min_votes);
  const int r = unitig_file(unitigger, reads_path, prefix, min_overlap, device, fasta_path, layout_path, piece_reads, err, errcap);
  if (r == 0 && status24) {
    const uint64_t s[24] = {unitigger.unitigs(),  unitigger.bases(),        unitigger.merged(),     unitigger.cycles(),    unitigger.trimRounds(),
                            unitigger.islands(),  unitigger.deadEnds(),     unitigger.readsRemoved(), unitigger.recordsCut(), unitigger.cutRounds(),
                            unitigger.chimericUnitigs(), unitigger.chimericReads(), unitigger.bubblesPopped(), unitigger.bubbleReads(),
                            unitigger.bubblesKept(), unitigger.indelsPopped(), unitigger.indelReads(), unitigger.indelsKept(),
                            unitigger.indelsNotCompared(), unitigger.reducedFinal(), unitigger.containedReads(), unitigger.consensusChanged(),
                            unitigger.consensusStatus()[3], unitigger.placeStatus()[3]};
    for (int k = 0; k < 24; ++k) status24[k] = s[k];
  }
  return r;
}

int sigah_unitig_consensus_file(const char* reads_path, const char* prefix, uint64_t min_overlap, int irreducible, int rc, int device,
                                const char* fasta_path, const char* layout_path, uint64_t piece_reads, uint64_t cut_terminal,
                                uint64_t min_branch_length, int64_t min_branch_coverage, const char* graph_path, const char* removed_path,
                                uint64_t delta, int careful, uint64_t num_reads, uint64_t genome_size, double uniq_threshold,
                                const char* cut_path, uint64_t min_chimeric_length, int64_t min_chimeric_coverage, uint64_t chimeric_delta,
                                double chimeric_threshold, const char* chimeric_path, uint64_t max_bubble_span, int64_t bubble_divergence,
                                const char* bubbles_path, uint64_t bubble_edits, uint64_t bubble_edit_permille, int reduce,
                                int64_t error_permille, uint64_t seed_length, uint64_t seed_stride, uint64_t max_seed_hits,
                                uint64_t max_candidates, int consensus, uint64_t min_votes, const char* contained_path, uint64_t* status24,
                                char* err, uint64_t errcap) {
  return sigah_unitig_placed_file(reads_path, prefix, min_overlap, irreducible, rc, device, fasta_path, layout_path, piece_reads, cut_terminal,
                                  min_branch_length, min_branch_coverage, graph_path, removed_path, delta, careful, num_reads, genome_size,
                                  uniq_threshold, cut_path, min_chimeric_length, min_chimeric_coverage, chimeric_delta, chimeric_threshold,
                                  chimeric_path, max_bubble_span, bubble_divergence, bubbles_path, bubble_edits, bubble_edit_permille, reduce,
                                  error_permille, seed_length, seed_stride, max_seed_hits, max_candidates, consensus, min_votes, contained_path, 0,
                                  status24, err, errcap);
}

// `siga preqc`: FMIndex::loadForward + KmerSpectrum; the JSON object goes to out_path, or to stdout when it is empty
int sigah_preqc(const char* prefix, uint64_t k, uint64_t samples, uint64_t seed, int all, uint64_t max_count, int device,
                const char* out_path, uint64_t batch_rows, char* err, uint64_t errcap) {
  sigah::FMIndex fmi;
  if (!load_index(fmi, prefix, device, true, err, errcap)) return -1;
  sigah::KmerSpectrum::Options o;
  o.kmerSize = k;
  o.samples = samples;
  o.seed = seed;
  o.all = all != 0;
  o.maxCount = max_count;
  sigah::KmerSpectrum spectrum(o);
  if (!spectrum.run(fmi, (size_t)batch_rows)) {
    if (err && errcap) snprintf(err, errcap, "%s", spectrum.error().c_str());
    return -1;
  }
  const std::string text = spectrum.json();
  FILE* f = out_path && out_path[0] ? fopen(out_path, "wb") : stdout;
  const bool ok = f && fwrite(text.data(), 1, text.size(), f) == text.size() && fflush(f) == 0;
  if (f && f != stdout) fclose(f);
  if (!ok && err && errcap) snprintf(err, errcap, "Failed to write %s", out_path && out_path[0] ? out_path : "stdout");
  return ok ? 0 : -1;
}

// test hook: parse a reads file with the parallel loader (mode 0) or the record-at-a-time DNASeqReader (mode 1) and dump
// "name\tcomment\tseq\tquality\n" per read; mode 2: the parallel loader and the edge converter's read table, "rank\tlength\n"
// per read; returns the number of reads or -1
int64_t sigah_parse_file(const char* path, int mode, const char* out_path, int threads) {
  FILE* f = fopen(out_path, "wb");
  if (!f) return -1;
  const sigah::HostSettings hs;
  int64_t n = -1;
  if (mode == 3) {  // parse only (timing aid): nothing written
    sigah::ReadStore rs;
    if (sigah::LoadReads(path, &rs, (unsigned)std::max(threads, 1), hs)) n = (int64_t)rs.size();
  } else if (mode == 2) {
    sigah::ReadStore rs;
    if (sigah::LoadReads(path, &rs, (unsigned)std::max(threads, 1), hs)) {
      std::vector<uint32_t> lengths, ranks;
      sigah::name_ranks(rs, (unsigned)std::max(threads, 1), &lengths, &ranks);
      n = (int64_t)rs.size();
      for (size_t i = 0; i < rs.size(); ++i) fprintf(f, "%u\t%u\n", ranks[i], lengths[i]);
    }
  } else if (mode == 0) {
    sigah::ReadStore rs;
    if (sigah::LoadReads(path, &rs, (unsigned)std::max(threads, 1), hs)) {
      n = (int64_t)rs.size();
      for (size_t i = 0; i < rs.size(); ++i) {
        std::string line;
        line.append(rs.name(i)); line += '\t'; line.append(rs.comment(i)); line += '\t'; line.append(rs.seq(i)); line += '\t';
        line.append(rs.quality(i)); line += '\n';
        fwrite(line.data(), 1, line.size(), f);
      }
    }
  } else {
    sigah::DNASeqList reads;
    if (sigah::ReadDNASequences(path, reads)) {
      n = (int64_t)reads.size();
      for (auto& r : reads) {
        std::string line = r.name + "\t" + r.comment + "\t" + r.seq + "\t" + r.quality + "\n";
        fwrite(line.data(), 1, line.size(), f);
      }
    }
  }
  fclose(f);
  return n;
}

// Test hook (CPU tests, sanitizer builds): the text side of OverlapBuilder::build without a GPU -- the reads of `path` through
// the loader, then the writer build() uses (AsqgWriter: VT lines with the substring flags given, the ED lines of the given
// edge records, the output stream, gz by name), fed as if batches of SIGA_BATCH_READS reads came back one by one (the whole
// input when unset); all edge records go in with the last batch.  Returns the number of reads, -1 on failure.
int64_t sigah_format_asqg(const char* path, const uint8_t* substring, const sigax_edge* edges, uint64_t n_edges, uint64_t min_overlap,
                          const char* out_path, int threads) {
  const sigah::HostSettings hs;
  const unsigned nt = (unsigned)std::max(threads, 1);
  sigah::ReadStore rs;
  if (!sigah::LoadReads(path, &rs, nt, hs)) return -1;
  std::vector<uint32_t> lengths, ranks;
  sigah::name_ranks(rs, nt, &lengths, &ranks);
  const size_t n = rs.size();
  for (uint64_t i = 0; i < n_edges; ++i)
    if (edges[i].query >= n || edges[i].target >= n) return -1;
  sigah::OutFile out(out_path, nt);
  if (!out.ok()) return -1;
  const std::string header = sigah::asqg_header((size_t)min_overlap);
  out.write(header);
  std::unique_ptr<sigah::VtAhead> ahead;
  if (hs.vt_ahead_wanted() && n > 0) ahead.reset(new sigah::VtAhead(&rs, nt, header, out.gz(), hs));
  const size_t per = hs.batch_reads ? hs.batch_reads : std::max<size_t>(n, 1);
  sigah::AsqgWriter writer(out, rs, lengths, nt, hs, std::move(ahead), 1000, nullptr, (n + per - 1) / per);  // (the records are the caller's)
  for (size_t lo = 0; lo < n; lo += per) {
    const bool last = lo + per >= n;
    writer.add_batch(lo, std::min(per, n - lo), substring ? substring + lo : nullptr, last ? edges : nullptr, last ? n_edges : 0);
  }
  return writer.finish() ? (int64_t)n : -1;
}

// Utils::ofstream as used for <prefix>.asqg.gz: write `n` bytes in `pieces` write() calls (gz when the name ends with .gz)
int sigah_write_file(const char* path, const char* data, uint64_t n, uint64_t pieces) {
  sigah::OutFile out(path);
  if (!out.ok()) return -1;
  uint64_t step = pieces ? (n + pieces - 1) / pieces : n;
  for (uint64_t b = 0; b < n; b += step ? step : 1) out.write(data + b, (size_t)std::min<uint64_t>(step, n - b));
  return out.close() ? 0 : -1;
}

void sigah_stem(const char* path, char* out, uint64_t cap) { snprintf(out, cap, "%s", sigah::Utils::stem(path).c_str()); }

}  // extern "C"
