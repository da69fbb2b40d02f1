// siga_amd/host/pairs.hpp -- internal: the paired-end side of `siga unitig` (pairs.cpp).
#ifndef SIGA_AMD_HOST_PAIRS_HPP_
#define SIGA_AMD_HOST_PAIRS_HPP_

#include <cstdint>
#include <string>
#include <vector>

#include "reads.hpp"
#include "siga_host.hpp"

namespace sigah {

// The mate of every read by name, as PairEnd::id finds it (src/reads.cpp:19-41): the mate's name is the read's with its last
// character swapped 1<->2, A<->B or f<->r.  SIGAX_NO_MATE where the name ends otherwise, the mate's name is absent, or either
// of the two names occurs more than once.  `ranks` = name_ranks' (equal names, equal rank).
std::vector<uint32_t> mates_by_name(const ReadStore& rs, const std::vector<uint32_t>& ranks);

struct PairsRequest {
  std::string json, links;  // files; links may be empty
  uint64_t maxSpan = 0;
  bool outward = false;
  uint32_t bins = 1024, shift = 0;
  bool haveContainedMates = false;  // `siga unitig -e`: the JSON also gets "contained_mates"
  uint64_t containedMates = 0;
};
struct ScaffoldRequest {
  std::string fasta, layout;  // files; fasta empty: no scaffolds; layout may be empty
  uint32_t minPairs = 2, linkRatio = 0, minUnitigBases = 0, minGap = 1, maxGap = 1000000;
  bool haveInsertSize = false;  // else floor(sum span / n) of the pairs call
  uint64_t insertSize = 0;
  // gap filling behind the scaffold call (sigax_gapfill_host): index NULL = none; gaps may be empty
  sigax_index* index = nullptr;
  uint32_t gapKmer = 31, gapMinCount = 3, gapSlack = 100, gapMaxFill = 10000;
  std::string gaps;
  // overlapping neighbours joined behind the scaffold or gapfill call (sigax_join_host): joinIndex NULL = none; joins may be empty
  sigax_index* joinIndex = nullptr;
  uint32_t joinMinOverlap = 16, joinMaxOverlap = 1000, joinSlack = 100, joinKmer = 31, joinMinCount = 3;
  uint32_t joinMismatches = 0, joinMismatchPermille = 50;  // joinMismatches > 0: sigax_join_approx_host
  std::string joins;
};
// sigax_unitigs_pairs_host over a unitig call's result, then the two files; with sc->fasta also sigax_scaffold_host over the
// unitigs (useqs: their bases) and the links, then its two files and status16; with sc->index also sigax_gapfill_host over the
// scaffolds before they are written, sc->gaps and gap24; with sc->joinIndex then sigax_join_host (sigax_join_approx_host with sc->joinMismatches), sc->joins and
// join24 (entries 16 .. 23 zero without mismatches).
// -> "" or what went wrong
std::string run_pairs(int device, const std::vector<uint32_t>& mate, const std::vector<uint32_t>& lengths, uint64_t n_unitigs,
                      const uint64_t* seq_offs, const uint64_t* lay_offs, const uint32_t* uflags, const sigax_placement* layout,
                      const PairsRequest& rq, uint64_t status24[24], uint64_t* insert_size, uint64_t* delta,
                      const ScaffoldRequest* sc = nullptr, const char* useqs = nullptr, uint64_t status16[16] = nullptr,
                      uint64_t gap24[24] = nullptr, uint64_t join24[24] = nullptr);

}  // namespace sigah

#endif
