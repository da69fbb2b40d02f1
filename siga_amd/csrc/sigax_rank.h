// siga_amd/csrc/sigax_rank.h -- device helpers shared by the kernels that walk the forward strand symbol by symbol
// (sigax_match.hip, sigax_spectrum.hip, sigax_locate.hip): byte -> rank, Occ out of a one-step granule, the pair counts of a
// two-step line (fm_layout.h), and the wave reductions they report their statistics with.  Device code only; every
// translation unit gets its own copy.
#ifndef SIGA_AMD_SIGAX_RANK_H_
#define SIGA_AMD_SIGAX_RANK_H_

#include <hip/hip_runtime.h>

#include "fm_layout.h"

namespace {

typedef unsigned long long u64;
typedef unsigned int u32;

template <bool WIDE> struct PosOf { typedef u32 type; };
template <> struct PosOf<true> { typedef u64 type; };

// alphabet.h:19-39: byte -> rank, branch-free (as base_rank of sigax_kernels.hip); complement in rank space
__device__ __forceinline__ u32 base_rank(u32 ch) {
  const u32 i = (ch >> 1) & 3u;
  const u32 expect = (0x47544341u >> (i * 8)) & 0xFFu;  // "ACTG"
  const u32 rank = (0x3421u >> (i * 4)) & 0xFu;         // 1, 2, 4, 3
  return expect == ch ? rank : 0u;
}
__device__ __forceinline__ u32 comp_rank(u32 r) { return r ? 5u - r : 0u; }

template <typename T>
__device__ __forceinline__ T sel4(u32 i, T v0, T v1, T v2, T v3) {  // v[i], i in 0..3, out of registers
  const T t01 = (i & 1u) ? v1 : v0, t23 = (i & 1u) ? v3 : v2;
  return (i & 2u) ? t23 : t01;
}

__device__ __forceinline__ u64 wave_sum(u64 v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ u64 first_lane64(u64 v) {
  return (u64)__builtin_amdgcn_readfirstlane((u32)v) | ((u64)__builtin_amdgcn_readfirstlane((u32)(v >> 32)) << 32);
}

// ---- one-step granule (fm_layout.h): A, C, G, T among BWT[0, p) ---------------------------------------------------
struct Gran1 {
  uint4 k0, k1, k2, k3;
};
__device__ __forceinline__ void chunk_count(const uint4& k, int take, u32& a, u32& c, u32& g, u32& t) {
  const u32 m = take >= 32 ? 0xFFFFFFFFu : (take <= 0 ? 0u : ((1u << take) - 1u));
  const u32 x0 = k.y & m, x1 = k.z & m, x2 = k.w & m;
  a += __popc(x0 & ~x1);
  c += __popc(x1 & ~x0);
  g += __popc(x0 & x1);
  t += __popc(x2);
}
// Occ(rank r, p - 1) for the clamped position pc out of its granule; r = 0: the '$' column (fm_layout.h)
template <bool WIDE>
__device__ __forceinline__ u64 gran_rank(const FmStrand& s, const Gran1& q, u64 pc, u32 r) {
  const int rem = (int)(pc & 127u);
  u32 a = q.k0.x, c = q.k1.x, g = q.k2.x, t = q.k3.x;
  chunk_count(q.k0, rem, a, c, g, t);
  chunk_count(q.k1, rem - 32, a, c, g, t);
  chunk_count(q.k2, rem - 64, a, c, g, t);
  chunk_count(q.k3, rem - 96, a, c, g, t);
  u64 A = a, C = c, G = g, T = t;
  if (WIDE) {
    const u64* sb = s.super + (pc >> SIGAX_SUPER_SHIFT) * 4;
    A += sb[0]; C += sb[1]; G += sb[2]; T += sb[3];
  }
  return r == 0 ? pc - (A + C + G + T) : sel4<u64>(r - 1u, A, C, G, T);
}
__device__ __forceinline__ Gran1 gran_load(const FmStrand& s, u64 pc) {
  const uint4* q = reinterpret_cast<const uint4*>(s.granules) + (pc >> 7) * 4;
  Gran1 o;
  o.k0 = q[0]; o.k1 = q[1]; o.k2 = q[2]; o.k3 = q[3];
  return o;
}

// ---- two-step line (fm_layout.h) ------------------------------------------------------------------------------------
struct Gran2 {  // the five 16-byte pieces of a line one double step needs
  uint4 s, pc, p5, p6, p7;  // one-symbol counts; pair counts [first symbol c][x = A..T]; planes
};
__device__ __forceinline__ Gran2 gran2_load(const uint32_t* gran2, u64 p, u32 c) {
  const uint4* q = reinterpret_cast<const uint4*>(gran2 + (p >> 6) * SIGAX_GRAN2_WORDS);
  Gran2 o;
  o.s = q[0]; o.pc = q[c]; o.p5 = q[5]; o.p6 = q[6]; o.p7 = q[7];
  return o;
}
// rows j < p of the line's 64 with c1(j) = c (one) and with c1(j) = c, c2(j) = e (two), counters included; r = p & 63
__device__ __forceinline__ void rank2(const Gran2& q, u32 r, u32 c, u32 e, u32& one, u32& two) {
  const u32 m0 = r >= 32 ? 0xFFFFFFFFu : ((1u << r) - 1u);
  const u32 m1 = r > 32 ? ((1u << (r - 32)) - 1u) : 0u;
  one = sel4<u32>(c - 1u, q.s.x, q.s.y, q.s.z, q.s.w);
  two = sel4<u32>(e - 1u, q.pc.x, q.pc.y, q.pc.z, q.pc.w);
  auto word = [&](u32 y, u32 z, u32 w, u32 y2, u32 z2, u32 w2, u32 m) {
    const u32 E = sel4<u32>(c - 1u, y & ~z, z & ~y, y & z, w) & m;                       // rows whose first symbol is c
    const u32 X = sel4<u32>(e - 1u, y2 & ~z2, z2 & ~y2, y2 & z2, w2) & E;                // ... and whose second is e
    one += __popc(E);
    two += __popc(X);
  };
  word(q.p5.x, q.p5.z, q.p6.x, q.p6.z, q.p7.x, q.p7.z, m0);
  word(q.p5.y, q.p5.w, q.p6.y, q.p6.w, q.p7.y, q.p7.w, m1);
}

}  // namespace

#endif
