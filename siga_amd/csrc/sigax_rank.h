// siga_amd/csrc/sigax_rank.h -- what the kernels that walk the forward strand symbol by symbol share (sigax_match.hip,
// sigax_spectrum.hip, sigax_locate.hip), each piece once:
//   leaves    Occ out of a one-step granule (Gran1, gran_rank), the pair counts of a two-step line (Gran2, rank2; fm_layout.h);
//             PosOf, byte -> rank, chunk_count, sel4 and first_lane64 are sigax_fm.h's, the wave sum is sigax_device.h's
//   search    the workgroup's constants (SearchSh, search_sh_fill), a chain's start from C[] or from the corrector's prefix
//             table (search_init, ptab_start), one backward-search step (search_step), interval_valid
//   chains    a wave's reservation of chain numbers from a global counter (ChainGrab, grab_chains)
//   launch    the grid of a persistent kernel (persistent_cap, launch_persistent; host)
// Every translation unit gets its own copy.
#ifndef SIGA_AMD_SIGAX_RANK_H_
#define SIGA_AMD_SIGAX_RANK_H_

#include <hip/hip_runtime.h>

#include "fm_layout.h"
#include "sigax_fm.h"

namespace {

// ---- one-step granule (fm_layout.h): A, C, G, T among BWT[0, p) ---------------------------------------------------
struct Gran1 {
  uint4 k0, k1, k2, k3;
};
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

// ---- backward search: constants, start, step ---------------------------------------------------------------------------
template <typename P>
__device__ __forceinline__ bool interval_valid(P lo, P hi) { return hi != (P)~(P)0 && hi >= lo; }

template <bool WIDE>
struct SearchSh {  // a workgroup's copy in LDS
  typedef typename PosOf<WIDE>::type P;
  u64 C[5], T[5];  // FMIndex::_pred and the symbol totals
  P Cc[4][4];      // Cc[c][e] = Occ(e, C[c]): the constants of a double step
};
// by the first 16 threads of the workgroup, before its __syncthreads()
template <bool WIDE>
__device__ __forceinline__ void search_sh_fill(SearchSh<WIDE>& sh, const FmStrand& S) {
  typedef typename PosOf<WIDE>::type P;
  if (threadIdx.x < 5) {
    sh.C[threadIdx.x] = S.C[threadIdx.x];
    sh.T[threadIdx.x] = S.total[threadIdx.x];
  }
  if (threadIdx.x < 16) {
    const u32 c = threadIdx.x >> 2, e = threadIdx.x & 3u;
    u64 pc = S.C[c + 1];
    pc = pc > S.n ? S.n : pc;
    sh.Cc[c][e] = (P)gran_rank<WIDE>(S, gran_load(S, pc), pc, e + 1u);
  }
}
// the strand carries what a double step reads
template <bool WIDE>
__device__ __forceinline__ bool have_two_step(const FmStrand& S) { return S.gran2 != nullptr && (!WIDE || S.super2 != nullptr); }

// Interval::init (src/fmindex.h:90-93): the rows whose suffix begins with the symbol of rank r0
template <bool WIDE, typename P>
__device__ __forceinline__ void search_init(const SearchSh<WIDE>& sh, u32 r0, P& lo, P& hi) {
  lo = (P)sh.C[r0];
  hi = lo + (P)sh.T[r0] - 1;
}
// A chain's start from the prefix table (k_prefix_build): sym(j), j = 0 .. pk - 1, are the ranks of the first pk symbols it
// consumes; the first one goes to the lowest two bits of the entry's number.  -> false, nothing set, when one of them is not
// ACGT; else the entry's interval -- empty (lo > hi) for an entry without rows: the reference stopped somewhere in these
// symbols, after one at the least.
template <bool WIDE, typename P, typename Sym>
__device__ __forceinline__ bool ptab_start(const void* ptab, u32 pk, Sym sym, P& lo, P& hi) {
  u32 code = 0;
  bool acgt = true;
  for (u32 j = 0; j < pk; ++j) {
    const u32 r = sym(j);
    acgt = acgt && r != 0u;
    code |= ((r - 1u) & 3u) << (2u * j);
  }
  if (!acgt) return false;
  u64 cnt;
  if (WIDE) {
    const ulonglong2 e = reinterpret_cast<const ulonglong2*>(ptab)[code];
    lo = (P)e.x;
    cnt = e.y;
  } else {
    const uint2 e = reinterpret_cast<const uint2*>(ptab)[code];
    lo = (P)e.x;
    cnt = e.y;
  }
  hi = lo + (P)cnt - 1;
  if (cnt == 0) {
    lo = 1;
    hi = 0;
  }
  return true;
}

// One step of a live chain whose next symbol has rank r.  e != 0 (the caller has looked: the strand has two-step lines, r and
// the symbol after it are ACGT): both symbols off a pair of two-step lines, Occ(e, C[r] + Occ(r, p)) = Cc[r][e] + R2(e, r, p)
// (fm_layout.h); an interval that symbol r emptied comes out empty after the pair (R2 over no rows).  e == 0: r alone off
// one-step granules.  -> symbols consumed; n_sec += the 64-byte sectors asked for; *first_left: rows were left after r (where
// the reference stops counting symbols) -- a caller that does not read it does not pay for it.
template <bool WIDE, typename P>
__device__ __forceinline__ u32 search_step(const FmStrand& S, const SearchSh<WIDE>& sh, u32 r, u32 e, P& lo, P& hi, u32& n_sec,
                                           bool* first_left) {
  const u64 pl = (u64)lo > S.n ? S.n : (u64)lo, pu0 = (u64)hi + 1ull, pu = pu0 > S.n ? S.n : pu0;
  if (e != 0u) {
    const bool two = (pl >> 6) != (pu >> 6);
    const Gran2 ga = gran2_load(S.gran2, pl, r);
    Gran2 gb = ga;
    if (two) gb = gran2_load(S.gran2, pu, r);
    n_sec += two ? 4u : 2u;
    u32 l1, l2, u1, u2;
    rank2(ga, (u32)pl & 63u, r, e, l1, l2);
    rank2(gb, (u32)pu & 63u, r, e, u1, u2);
    P L1 = (P)l1, L2 = (P)l2, U1 = (P)u1, U2 = (P)u2;
    if (WIDE) {
      const u64* sl = S.super2 + (pl >> SIGAX_SUPER_SHIFT) * 20;
      const u64* su = S.super2 + (pu >> SIGAX_SUPER_SHIFT) * 20;
      const u32 col = 4u + (r - 1u) * 4u + (e - 1u);
      L1 += (P)sl[r - 1u]; U1 += (P)su[r - 1u];
      L2 += (P)sl[col]; U2 += (P)su[col];
    }
    const P pb = (P)sh.C[e] + sh.Cc[r - 1u][e - 1u];
    lo = pb + L2;
    hi = pb + U2 - 1;
    *first_left = U1 > L1;
    return 2u;
  }
  const bool two = (pl >> 7) != (pu >> 7);
  const Gran1 qa = gran_load(S, pl);
  Gran1 qb = qa;
  if (two) qb = gran_load(S, pu);
  n_sec += two ? 2u : 1u;
  const P pb = (P)sh.C[r];
  lo = pb + (P)gran_rank<WIDE>(S, qa, pl, r);      // getOcc(c, lower - 1)
  hi = pb + (P)gran_rank<WIDE>(S, qb, pu, r) - 1;  // getOcc(c, upper)
  *first_left = true;
  return 1u;
}
template <bool WIDE, typename P>
__device__ __forceinline__ u32 search_step(const FmStrand& S, const SearchSh<WIDE>& sh, u32 r, u32 e, P& lo, P& hi, u32& n_sec) {
  bool first_left;
  return search_step<WIDE>(S, sh, r, e, lo, hi, n_sec, &first_left);
}

// ---- chain numbers for the lanes of a persistent grid ---------------------------------------------------------------
#define GRAB 64u  // chain numbers a wave reserves at a time: one atomic per 64 chains, and the last waves of a launch are never
                  // more than 64 chains apart
struct ChainGrab {         // wave-uniform
  u64 next = 0, end = 0;   // the wave's reserved numbers
  bool drained = false;    // the global counter has run out
};
// One round of handing the wave's reserved numbers (more reserved from *counter when they are used up) to its idle lanes.
// -> false: no lane is idle, or no number is left for those that are.  Else *chain is this lane's number when `got`; a lane
// may stay idle with it (an empty pattern), so the caller asks again until false.
__device__ __forceinline__ bool grab_chains(ChainGrab& g, u64* counter, u64 n_chains, bool idle, bool& got, u64& chain) {
  const u32 lane = threadIdx.x & 63u;
  const u64 need = __ballot(idle);
  got = false;
  if (need == 0ull) return false;
  if (g.next >= g.end) {
    if (g.drained) return false;
    u64 b = 0;
    if (lane == 0) b = atomicAdd(counter, (u64)GRAB);
    b = first_lane64(b);
    if (b >= n_chains) {
      g.drained = true;
      return false;
    }
    g.next = b;
    g.end = b + GRAB < n_chains ? b + GRAB : n_chains;
  }
  // mine: the idle lanes below this one
  const u32 avail = (u32)(g.end - g.next), wanted = (u32)__popcll(need);
  const u32 mine = __builtin_amdgcn_mbcnt_hi((u32)(need >> 32), __builtin_amdgcn_mbcnt_lo((u32)need, 0u));
  got = idle && mine < avail;
  chain = g.next + mine;
  g.next += wanted < avail ? wanted : avail;
  return true;
}

// ---- the grid of a persistent kernel (host) -------------------------------------------------------------------------
// as many 256-lane workgroups as the device holds at once
template <typename K>
unsigned persistent_cap(K kernel, int n_cu) {
  int per_cu = 0;
  const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 256, 0);
  if (e != hipSuccess || per_cu < 1) {
    (void)hipGetLastError();
    per_cu = 2;
  }
  return (unsigned)(n_cu > 0 ? n_cu : 256) * (unsigned)per_cu;
}
// ... and no more of them than `want`, what the work can keep busy
template <typename K, typename Args>
void launch_persistent(K kernel, const Args& a, unsigned long long want, int n_cu, hipStream_t st) {
  const unsigned long long cap = persistent_cap(kernel, n_cu);
  hipLaunchKernelGGL(kernel, dim3((unsigned)(want < cap ? want : cap)), dim3(256), 0, st, a);
}

}  // namespace

#endif
