// siga_amd/csrc/sigax_pileup.h -- argument blocks and launch wrappers shared by sigax_pileup.hip and sigax_pileup.cpp
// (`siga correct -a overlap`).  The seeds, their hits and the reference text come from sigax_seeded.h.
#ifndef SIGA_AMD_SIGAX_PILEUP_H_
#define SIGA_AMD_SIGAX_PILEUP_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sigax.h"
#include "sigax_seeded.h"

// counters of a round, in the caller's scratch (u64 each, zeroed before the round)
enum { PILE_C_LONG = 0, PILE_C_OVER, PILE_C_LOCATED, PILE_C_REPEATS, PILE_C_TESTED, PILE_C_ACCEPTED, PILE_C_CHANGED, PILE_C_COUNT = 8 };

struct PileArgs {
  const unsigned char* seqs;
  const unsigned long long* offs;        // [n_reads + 1]
  unsigned long long n_reads;
  sigax_pile_params p;
  uint32_t len_cap;                      // columns a wave's LDS holds: max_read_len rounded up to 64
  uint32_t tab_cap;                      // slots of a wave's table of candidates, a power of two (cand_tab_cap)
  SeedHits<const uint4> L;               // its seeds and their hits: read only
  RefText R;
  // out
  unsigned char* out_seqs;
  unsigned char* valid;
  unsigned char* changed;
  unsigned long long* counters;          // PILE_C_COUNT u64, zeroed
  unsigned long long* status;            // 8 u64, written by k_pile_status
};
int launch_pile(const PileArgs& a, hipStream_t st);  // hipSuccess or the error of raising the LDS limit
void launch_pile_status(const PileArgs& a, hipStream_t st);
// the dynamic LDS of a wave
uint32_t pile_lds_bytes(uint32_t len_cap, uint32_t tab_cap);

// Measurement aid of tools/pileup_bench.py, exported but not part of include/sigax.h and not stable: the pile-up kernel and the
// status words alone, over the seeds and hits a sigax_pileup_device call with the same arguments left in d_work.  It cannot tell
// whether such a call was made; the kernel bounds every access all the same.  Same argument checks as sigax_pileup_device.
extern "C" int sigax_pileup_pile_device(sigax_index*, const void* d_seqs, const void* d_offs, uint64_t n_reads, uint64_t n_bases,
                                        const sigax_pile_params*, const void* d_ref_text, const void* d_ref_offs, void* d_out_seqs,
                                        void* d_valid, void* d_changed, void* d_status8, void* d_work, uint64_t work_bytes,
                                        uint64_t hits_cap, void* stream);

#endif
