// siga_amd/csrc/sigax_consensus.h -- what sigax_consensus.hip and sigax_consensus.cpp share: the arguments of the consensus pass
// over a unitig call's layout (`siga unitig -e`; the rules are in include/sigax.h).
#ifndef SIGA_AMD_SIGAX_CONSENSUS_H_
#define SIGA_AMD_SIGAX_CONSENSUS_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sigax.h"
#include "sigax_kernels.h"

struct ConsArgs {
  const unsigned long long* n_unitigs;   // on the device: entry 0 of the unitig call's status block
  unsigned long long max_unitigs;        // seq_offs and lay_offs hold max_unitigs + 1 entries, changed max_unitigs
  const unsigned long long* seq_offs;
  const unsigned long long* lay_offs;
  const sigax_placement* layout;         // n_reads records
  const uint32_t* lengths;
  const unsigned char* seqs;
  const unsigned long long* offs;        // n_reads + 1
  unsigned long long n_reads;
  uint32_t min_votes;
  unsigned char* useqs;                  // offs[n_reads] - offs[0] bytes, in and out
  uint32_t* changed;                     // max_unitigs u32, zeroed
  unsigned char* support;                // as useqs, or NULL
  unsigned long long* status;            // 8 u64
  unsigned long long* cnt;               // CONS_WORDS u64, zeroed: the counters, slotted as the trim counters are; the longest read
                                         // at CONS_MAX_LEN, the largest depth at CONS_MAX_DEPTH
};
// the counters: columns, columns changed, columns of depth below 2, own bases that stayed on a tie, columns held back by min_votes,
// placements skipped as invalid
enum { CONS_C_COLUMNS = 0, CONS_C_CHANGED = 1, CONS_C_SHALLOW = 2, CONS_C_TIES = 3, CONS_C_HELD = 4, CONS_C_INVALID = 5, CONS_COUNTERS = 6,
       CONS_MAX_LEN = counter_words(CONS_COUNTERS), CONS_MAX_DEPTH = CONS_MAX_LEN + 1, CONS_WORDS = CONS_MAX_LEN + 2,
       CONS_GRID = 2048 };

hipError_t launch_consensus(const ConsArgs& a, hipStream_t st);

#endif
