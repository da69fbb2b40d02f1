// siga_amd/csrc/sigax_device.h -- the small pieces the kernels of `siga unitig` and of the assembly behind it share
// (sigax_unitig.hip, sigax_pairs.hip, sigax_scaffold.hip, sigax_gapfill.hip, sigax_join.hip; sigax_fm.h, and through it sigax_rank.h
// and the kernels of sigax_kernels.hip, take the typedefs and the wave sum from here, sigax_seeded.h its 64-bit shuffle), each piece once:
//   waves       wave_sum, wave_min32, wave_max32; wave_add: a wave's sum added once, by lane 0, when it is not zero; shfl64
//   counters    a counter block is TRIM_SLOTS partial sums per counter, TRIM_STRIDE words apart (sigax_kernels.h): counter_slot,
//               counter_total
//   bases       comp_byte
//   tables      last_at_most (the bisection over an ascending u64 table), head_dir, placement_offset, and the bounds of the
//               scaffold tables (ScafBounds, scaffold_bounds, scaffold_of)
//   launch      blocks_of (host)
// Device-inline only; every translation unit gets its own copy.
#ifndef SIGA_AMD_SIGAX_DEVICE_H_
#define SIGA_AMD_SIGAX_DEVICE_H_

#include <hip/hip_runtime.h>

#include "sigax_kernels.h"

namespace {

typedef unsigned long long u64;
typedef unsigned int u32;

// ---- wave reductions ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ u64 wave_sum(u64 v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ u32 wave_min32(u32 v) {
  for (int off = 32; off > 0; off >>= 1) {
    const u32 o = (u32)__shfl_xor((int)v, off, 64);
    v = o < v ? o : v;
  }
  return v;
}
__device__ __forceinline__ u32 wave_max32(u32 v) {
  for (int off = 32; off > 0; off >>= 1) {
    const u32 o = (u32)__shfl_xor((int)v, off, 64);
    v = o > v ? o : v;
  }
  return v;
}
// this wave's sum of v, added once to *at
__device__ __forceinline__ void wave_add(u64* at, u64 v) {
  const u64 t = wave_sum(v);
  if (t && (threadIdx.x & 63u) == 0u) atomicAdd(at, t);
}
// v of lane `lane` of the wave
__device__ __forceinline__ u64 shfl64(u64 v, u32 lane) {
  return (u64)(u32)__shfl((int)(u32)v, (int)lane, 64) | ((u64)(u32)__shfl((int)(u32)(v >> 32), (int)lane, 64) << 32);
}

// ---- counter blocks -----------------------------------------------------------------------------------------------------------------
// where this wave adds to counter c of `block`: the slot of its number.  WAVES: the waves of a workgroup, 4 in the 256-lane
// kernels, 1 in the kernels that run one wave a workgroup
template <u32 WAVES = 4>
__device__ __forceinline__ u64* counter_slot(u64* block, u32 c) {
  const u32 wave = blockIdx.x * WAVES + (threadIdx.x >> 6);
  return block + ((u64)c * TRIM_SLOTS + (wave & (TRIM_SLOTS - 1u))) * TRIM_STRIDE;
}
__device__ __forceinline__ u64 counter_total(const u64* block, u32 c) {
  u64 v = 0;
  for (u32 s = 0; s < TRIM_SLOTS; ++s) v += block[((u64)c * TRIM_SLOTS + s) * TRIM_STRIDE];
  return v;
}

// ---- bases --------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ u32 comp_byte(u32 b) {
  return b == 'A' ? 'T' : b == 'T' ? 'A' : b == 'C' ? 'G' : b == 'G' ? 'C' : b;
}

// ---- tables -------------------------------------------------------------------------------------------------------------------------
// the last k < n with T[k] <= p in an ascending table (0 where there is none); at most 32 steps: n < 2^32
__device__ __forceinline__ u64 last_at_most(const u64* T, u64 n, u64 p) {
  u64 lo = 0, hi = n;
  for (int step = 0; step < 32 && hi - lo > 1; ++step) {
    const u64 mid = (lo + hi) >> 1;
    if (T[mid] <= p)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}
// Of the two final rank entries of a read (of a unitig), the direction that leads to the head of its unitig (scaffold): the terminal
// with the smaller id (one on its own: B, so that it is entered through B and placed forward)
__device__ __forceinline__ u32 head_dir(const uint4 a0, const uint4 a1) { return (a0.y >> 1) <= (a1.y >> 1) ? 0u : 1u; }
__device__ __forceinline__ u64 placement_offset(const sigax_placement* lay, u64 p) {
  const uint4 v = reinterpret_cast<const uint4*>(lay)[p];
  return (u64)v.z | ((u64)v.w << 32);
}
// what of the scaffold tables can be read: the unitigs, the scaffolds and the placements, each clamped to max_unitigs
struct ScafBounds {
  u64 nu, S, P;
};
template <class Args>
__device__ __forceinline__ ScafBounds scaffold_bounds(const Args& A) {
  const u64 n = A.max_unitigs;
  ScafBounds c;
  c.nu = *A.n_unitigs;
  c.nu = c.nu < n ? c.nu : n;
  c.S = *A.n_scaffolds;
  c.S = c.S < n ? c.S : n;
  c.P = c.S ? A.sc_lay_offs[c.S] : 0ull;
  c.P = c.P < n ? c.P : n;
  return c;
}
// the scaffold of placement p: the last s with sc_lay_offs[s] <= p
template <class Args>
__device__ __forceinline__ u64 scaffold_of(const Args& A, u64 S, u64 p) {
  return last_at_most(A.sc_lay_offs, S, p);
}

// ---- launch (host) ------------------------------------------------------------------------------------------------------------------
inline unsigned blocks_of(u64 n) { return (unsigned)((n + 255) / 256); }

}  // namespace

#endif
