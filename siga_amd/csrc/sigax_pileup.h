// siga_amd/csrc/sigax_pileup.h -- argument blocks and launch wrappers shared by sigax_pileup.hip and sigax_pileup.cpp
// (`siga correct -a overlap`).
#ifndef SIGA_AMD_SIGAX_PILEUP_H_
#define SIGA_AMD_SIGAX_PILEUP_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sigax.h"

// counters of a round, in the caller's scratch (u64 each, zeroed before the round)
enum { PILE_C_LONG = 0, PILE_C_OVER, PILE_C_LOCATED, PILE_C_REPEATS, PILE_C_TESTED, PILE_C_ACCEPTED, PILE_C_CHANGED, PILE_C_COUNT = 8 };

// Reference text by read id: the lengths pass has left lens[i] and stretch[i] of BWT row i; k_ref_order turns them into
// rows_by_id[sai[stretch[i]]] = i and lens_by_id[...] = lens[i], which the scan and the write pass take.
struct RefOrderArgs {
  const uint32_t* lens;                  // [n] by row
  const unsigned long long* stretch;     // [n] by row
  const uint32_t* sai;                   // [n]
  unsigned long long n;
  unsigned long long* rows_by_id;        // [n], preset to n (a row out of range: length 0)
  uint32_t* lens_by_id;                  // [n], zeroed
  unsigned long long* bad;               // 1 u64, zeroed: rows whose walk was cut or whose stretch names no read
};
void launch_ref_order(const RefOrderArgs& a, hipStream_t st);
void launch_ref_iota(unsigned long long* rows, unsigned long long n, hipStream_t st);  // rows[i] = i

struct PileArgs {
  const unsigned char* seqs;
  const unsigned long long* offs;        // [n_reads + 1]
  unsigned long long n_reads;
  sigax_pile_params p;
  uint32_t len_cap;                      // columns a wave's LDS holds: max_read_len rounded up to 64
  uint32_t tab_cap;                      // slots of a wave's table of candidates, a power of two
  // seeds
  uint32_t* seed_cnt;                    // [n_reads]
  unsigned long long* seed_start;        // [n_reads + 1]
  unsigned long long* seed_total;        // 1 u64: seed_start[n_reads]
  unsigned long long seed_cap;           // seed slots (queries of the locate call)
  unsigned char* seed_bytes;             // [seed_cap * S + 16]
  unsigned long long* seed_offs;         // [seed_cap + 1]
  // what locate left
  const uint32_t* qflags;                // [seed_cap]
  const unsigned long long* hit_offs;    // [seed_cap + 1]
  const sigax_hit* hits;                 // [hits_cap]
  unsigned long long hits_cap;
  const unsigned long long* loc_status;  // 4 u64: [0] = hits listed
  // reference text
  const unsigned char* ref_text;
  const unsigned long long* ref_offs;    // [n_ref + 1]
  unsigned long long n_ref;
  // out
  unsigned char* out_seqs;
  unsigned char* valid;
  unsigned char* changed;
  unsigned long long* counters;          // PILE_C_COUNT u64, zeroed
  unsigned long long* status;            // 8 u64, written by k_pile_status
};
void launch_pile_seed_count(const PileArgs& a, hipStream_t st);
void launch_pile_seed_fill(const PileArgs& a, hipStream_t st);
int launch_pile(const PileArgs& a, hipStream_t st);  // hipSuccess or the error of raising the LDS limit
void launch_pile_status(const PileArgs& a, hipStream_t st);
// slots of the candidate table for K candidates, and the dynamic LDS of a wave
uint32_t pile_tab_cap(uint32_t max_candidates);
uint32_t pile_lds_bytes(uint32_t len_cap, uint32_t tab_cap);

// Measurement aid of tools/pileup_bench.py, exported but not part of include/sigax.h and not stable: the pile-up kernel and the
// status words alone, over the seeds and hits a sigax_pileup_device call with the same arguments left in d_work.  It cannot tell
// whether such a call was made; the kernel bounds every access all the same.  Same argument checks as sigax_pileup_device.
extern "C" int sigax_pileup_pile_device(sigax_index*, const void* d_seqs, const void* d_offs, uint64_t n_reads, uint64_t n_bases,
                                        const sigax_pile_params*, const void* d_ref_text, const void* d_ref_offs, void* d_out_seqs,
                                        void* d_valid, void* d_changed, void* d_status8, void* d_work, uint64_t work_bytes,
                                        uint64_t hits_cap, void* stream);

#endif
