// siga_amd/csrc/sigax_mmoverlap.h -- argument blocks and launch wrappers shared by sigax_mmoverlap.hip and sigax_mmoverlap.cpp
// (`siga overlap -e`).  The seeds, their hits and the reference text come from sigax_seeded.h.
#ifndef SIGA_AMD_SIGAX_MMOVERLAP_H_
#define SIGA_AMD_SIGAX_MMOVERLAP_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sigax.h"
#include "sigax_seeded.h"

// counters of a call, in the caller's scratch (u64 each, zeroed before the call)
enum { MMO_C_LENGTH = 0, MMO_C_OVER, MMO_C_LOCATED, MMO_C_REPEATS, MMO_C_TESTED, MMO_C_ACCEPTED, MMO_C_COUNT = 8 };

// What k_mmo finds is on its way to k_mmo_commit in the place of the read's own hits, 16 bytes each: a record as {canonical query,
// target, length, af | num_diff << 8}, a read to flag as its containment record {read id, container, o, af |
// num_diff << 8 | length << 19}.
struct MmoArgs {
  RefText R;                             // the indexed reads by id: queries and candidates alike
  const uint32_t* name_rank;             // [n_ref]
  unsigned long long first_read, n_reads;
  sigax_mmo_params p;                    // max_read_len filled in
  uint32_t tab_cap;                      // slots of a wave's table of candidates, a power of two (cand_tab_cap)
  SeedHits<uint4> L;                     // the seeds' hits: read by k_mmo, then a read's own stretch holds what it found
  // found, per read of the call
  uint32_t* n_rec;                       // [n_reads]: records, from the front of the read's stretch of hits
  uint32_t* n_flag;                      // [n_reads]: read ids to flag, from the back of it
  unsigned long long* rec_offs;          // [n_reads + 1]: the scan of n_rec
  unsigned long long* rec_total;         // 1 u64
  // out
  sigax_mm_edge* edges;
  unsigned long long edges_cap;
  unsigned long long* cursor;            // 1 u64: records in edges[]
  unsigned char* contained;              // [n_ref]
  unsigned long long* counters;          // MMO_C_COUNT u64, zeroed
  unsigned long long* status;            // 8 u64, written by k_mmo_status
};
uint32_t mmo_lds_bytes(uint32_t tab_cap);  // the dynamic LDS of a wave: the table alone, the read's codes are in registers
int launch_mmo(const MmoArgs& a, hipStream_t st);  // hipSuccess or the error of raising the LDS limit
void launch_mmo_commit(const MmoArgs& a, hipStream_t st);  // k_mmo_commit, then k_mmo_status

// finish: the raw records in (query, target, af, length, reserved) order, each once
struct MmoFinishArgs {
  sigax_mm_edge* edges;                  // [n]
  unsigned long long n;
  unsigned long long* keys[2];           // [n] each
  unsigned long long* vals[2];           // [n] each
  sigax_mm_edge* sorted;                 // [n]
  uint32_t* head;                        // [n]
  unsigned long long* scan;              // [n + 1]
  unsigned long long* partial;           // scan_partials_needed(n)
  unsigned long long* n_unique;          // 1 u64, the caller's
  void* sort_tmp;
  unsigned long long sort_tmp_bytes;
};
hipError_t mmo_sort_bytes(unsigned long long n, unsigned long long* bytes);
hipError_t launch_mmo_finish(const MmoFinishArgs& a, hipStream_t st);

// Measurement aid of tools/mmoverlap_bench.py, exported but not part of include/sigax.h and not stable: sigax_mmoverlap_device cut
// short.  stages = 1: the seeds and their hits alone; 2: those and k_mmo, nothing committed (no record, no flag, the cursor as it
// was; d_status8 is not written).  Same argument checks as sigax_mmoverlap_device.
extern "C" int sigax_mmoverlap_stages_device(sigax_index*, const void* d_ref_text, const void* d_ref_offs, uint64_t first_read, uint64_t n_reads,
                                             uint64_t n_bases, const sigax_mmo_params*, sigax_mm_edge* d_edges, uint64_t edges_cap, void* d_cursor,
                                             void* d_contained, void* d_status8, void* d_work, uint64_t work_bytes, uint64_t hits_cap, void* stream,
                                             int stages);

#endif
