// siga_amd/csrc/sigax_seeded.hip -- the kernels of the seeding stage (sigax_seeded.h; gfx950 / CDNA4, wave64), before the locate
// kernels take over.  No counterpart in the reference.
//
//   k_ref_iota, k_ref_order  the reference text by read id, around the row walk of sigax_spectrum.hip: rows 0 .. n_strings - 1
//                            are walked for their lengths and stretches, k_ref_order files row and length under the read id
//                            sai[stretch], the scan gives the offsets and the walk's write pass the bytes
//   k_seed_count             one lane per read: the seeds it has, none for a read the verifying kernel does not take
//   k_seed_fill              one lane per seed slot: the seed's bytes and its offset, as the query table of sigax_locate_device
#include <hip/hip_runtime.h>

#include "sigax_rank.h"
#include "sigax_seeded.h"

namespace {

__global__ __launch_bounds__(256) void k_ref_iota(u64* rows, u64 n) {
  const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
  if (i < n) rows[i] = i;
}

__global__ __launch_bounds__(256) void k_ref_order(RefOrderArgs A) {
  const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
  u32 bad = 0;
  if (i < A.n) {
    const u64 s = A.stretch[i];
    const u32 id = s < A.n ? A.sai[s] : 0xFFFFFFFFu;
    if ((u64)id < A.n) {
      A.rows_by_id[id] = i;
      A.lens_by_id[id] = A.lens[i];
    } else {
      bad = 1;
    }
  }
  wave_add(A.bad, (u64)bad);
}

__global__ __launch_bounds__(256) void k_seed_count(SeedArgs A) {
  const u64 r = (u64)blockIdx.x * 256 + threadIdx.x;
  if (r >= A.n_reads) return;
  const u64 n = A.offs[r + 1] - A.offs[r];
  A.seed_cnt[r] = (n < A.S || n > A.max_read_len) ? 0u : seeds_of((u32)n, A.S, A.T);
}

__global__ __launch_bounds__(256) void k_seed_fill(SeedArgs A) {
  const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
  if (i >= A.seed_cap) return;
  const u32 S = A.S;
  u64 total = *A.seed_total;
  total = total < A.seed_cap ? total : A.seed_cap;
  A.seed_offs[i] = (i < total ? i : total) * S;  // the slots behind the seeds are empty queries
  if (i == 0) A.seed_offs[A.seed_cap] = total * S;
  if (i >= total) return;
  const u64 r = last_at_most(A.seed_start, A.n_reads, i);  // the last read that starts at or before this seed: the one that has it
  const u64 b0 = A.offs[r];
  const u32 n = (u32)(A.offs[r + 1] - b0), j = (u32)(i - A.seed_start[r]);
  if (n < S || j >= seeds_of(n, S, A.T)) return;  // (not with a seed_start made from these reads)
  const u32 p = j < seeds_regular(n, S, A.T) ? j * A.T : n - S;
  const unsigned char* src = A.seqs + b0 + p;
  unsigned char* dst = A.seed_bytes + i * S;
  for (u32 k = 0; k < S; ++k) dst[k] = src[k];
}

}  // namespace

void launch_ref_iota(unsigned long long* rows, unsigned long long n, hipStream_t st) {
  if (n) hipLaunchKernelGGL(k_ref_iota, dim3(blocks_of(n)), dim3(256), 0, st, rows, n);
}

void launch_ref_order(const RefOrderArgs& a, hipStream_t st) {
  if (a.n) hipLaunchKernelGGL(k_ref_order, dim3(blocks_of(a.n)), dim3(256), 0, st, a);
}

void launch_seed_count(const SeedArgs& a, hipStream_t st) {
  if (a.n_reads) hipLaunchKernelGGL(k_seed_count, dim3(blocks_of(a.n_reads)), dim3(256), 0, st, a);
}

void launch_seed_fill(const SeedArgs& a, hipStream_t st) {
  if (a.seed_cap) hipLaunchKernelGGL(k_seed_fill, dim3(blocks_of(a.seed_cap)), dim3(256), 0, st, a);
}
