// siga_amd/csrc/sigax_contained.h -- what sigax_contained.hip and sigax_contained.cpp share: the arguments of the pass that places
// contained reads in a unitig call's layout (`siga unitig -e --place-contained`; the rules are in include/sigax.h).
#ifndef SIGA_AMD_SIGAX_CONTAINED_H_
#define SIGA_AMD_SIGAX_CONTAINED_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sigax.h"
#include "sigax_kernels.h"

// the counters of a call, u64 each, zeroed before it; CP_TOTAL is written by the scan of the per-unitig counts
enum { CP_C_CONTAINED = 0, CP_C_INVALID_RECORDS, CP_C_PLACED, CP_C_NO_CHAIN, CP_C_ROOT_REMOVED, CP_C_LONGEST, CP_TOTAL, CP_WORDS = 8 };
static const uint32_t CP_NONE = 0xFFFFFFFFu;

struct ContArgs {
  const unsigned long long* n_unitigs;   // on the device: entry 0 of the unitig call's status block
  unsigned long long max_unitigs;        // seq_offs, lay_offs and lay_offs2 hold max_unitigs + 1 entries
  const unsigned long long* seq_offs;
  const unsigned long long* lay_offs;
  const sigax_placement* layout;         // n_reads records
  const uint32_t* lengths;
  unsigned long long n_reads;
  const unsigned char* contained;        // n_reads
  const sigax_mm_edge* conts;            // n_conts containment records
  unsigned long long n_conts;
  // out
  unsigned long long* lay_offs2;
  sigax_placement* layout2;              // n_reads records, 0xFF where nothing is placed
  unsigned char* place_class;            // n_reads
  unsigned long long* status;            // 8 u64
  // scratch
  unsigned long long* best1;             // [n_reads]: per contained read the least (contained[target], num_diff) of its valid records
  unsigned long long* best2;             // [n_reads]: among those the least (target, reversed, offset): the choice; ~0: none
  uint32_t* slot;                        // [n_reads]: the first placement that names the read, CP_NONE: none
  uint32_t* owner;                       // [n_reads]: the unitig a placement belongs to, CP_NONE: none
  uint4* state[2];                       // [n_reads] each: {ancestor or CP_NONE, reversed in it, offset in it, steps to it}
  uint32_t* pu;                          // [n_reads]: the unitig a contained read is placed in, CP_NONE: not placed
  uint32_t* pflags;                      // [n_reads]
  unsigned long long* poff;              // [n_reads]
  unsigned long long* keys[2];           // [n_reads] each: the sort's keys
  uint32_t* vals[2];                     // [n_reads] each: the sort's values, read ids
  uint32_t* kept;                        // [n_reads]: 1 where a placement of the layout goes on into layout2
  unsigned long long* keptscan;          // [n_reads + 1]
  uint32_t* cnt;                         // [max_unitigs]: placements of a unitig in layout2
  unsigned long long* partial;           // scan_partials_needed(max(n_reads, max_unitigs)) u64
  unsigned long long* words;             // CP_WORDS u64, zeroed
  void* sort_tmp;
  unsigned long long sort_tmp_bytes;
  unsigned rounds;                       // unitig_rounds(n_reads): the pointer-doubling launches
};

hipError_t contained_sort_bytes(unsigned long long n, unsigned long long* bytes);  // a size query, launches nothing
hipError_t launch_contained_place(const ContArgs& a, hipStream_t st);

#endif
