// siga_amd/csrc/sigax_consensus.hip -- the consensus pass of `siga unitig -e` on the device (gfx950 / CDNA4, wave64): every column
// of every unitig rewritten by majority vote over the reads the layout lays over it.  The reference has nothing like it
// (Vertex::merge, src/bigraph.cpp:131-202, appends label bytes); the rules are in include/sigax.h and DESIGN.md 9r, and the
// restatement the tests hold this against is tests/consensus_cases.py::expected_consensus.
//   k_cons_prep    one lane per read and per placement: the longest read (one wave maximum, one atomicMax), and the placements
//                  that are invalid in their unitig (one ballot, one add per wave)
//   k_cons_vote    a wave takes 64 consecutive bytes of useqs, on the output's own 64-byte grid, lane l the column at byte g0 + l:
//                  its unitig by bisection in seq_offs, so that a tile over several short unitigs is as good as one inside a long
//                  one.  Within a unitig the offsets ascend, so a lane bisects for the first placement of its unitig that can
//                  reach its column -- offset + longest read > column -- and the wave walks the placements from the smallest such
//                  first to the first placement every lane is done with.  Placements are loaded 64 at a time, lane l the record
//                  first + l with that read's lengths[] and offs[] entry, and handed round by v_readlane: per placement one byte
//                  load per covered lane, forward or backward along the read, and no chain of dependent loads.  The four counts
//                  live in registers.  A lane reads nothing of useqs but its own byte and writes it only when the vote replaces
//                  it; changed[u] takes one add per tile (per lane where a tile spans several unitigs), the status counts one add
//                  per wave, after its last tile.  The grid is CONS_GRID workgroups that stride over the tiles.
//   k_cons_status  status8 from the counters
// Every loop has a bound the host knows (the tiles: the bytes of the reads / 64; the walk: n_reads) and every load and store is
// bounds-checked.  Plain vector loads and stores and atomics on counters only; integer work; no LDS.
#include <hip/hip_runtime.h>

#include "sigax_consensus.h"
#include "sigax_device.h"

namespace {

// what can be read: the unitigs, the placements, the bytes of the reads and of the unitigs
struct ConsBounds {
  u64 nu, P, src_end, T;
};
__device__ __forceinline__ ConsBounds cons_bounds(const ConsArgs& A) {
  ConsBounds c;
  const u64 n = A.n_reads;
  c.nu = *A.n_unitigs;
  c.nu = c.nu < n ? c.nu : n;
  c.nu = c.nu < A.max_unitigs ? c.nu : A.max_unitigs;
  c.P = c.nu ? A.lay_offs[c.nu] : 0ull;
  c.P = c.P < n ? c.P : n;
  const u64 src0 = A.offs[0];
  c.src_end = A.offs[n];
  const u64 cap = c.src_end > src0 ? c.src_end - src0 : 0ull;  // useqs holds as many bytes as the reads
  c.T = c.nu ? A.seq_offs[c.nu] : 0ull;
  c.T = c.T < cap ? c.T : cap;
  return c;
}

// A, C, G, T -> 0 .. 3, every other byte 4
__device__ __forceinline__ u32 letter_of(u32 b) { return b == 'A' ? 0u : b == 'C' ? 1u : b == 'G' ? 2u : b == 'T' ? 3u : 4u; }

__device__ __forceinline__ u32 lane_u32(u32 v, u32 j) { return (u32)__builtin_amdgcn_readlane((int)v, (int)j); }
__device__ __forceinline__ u64 lane_u64(u64 v, u32 j) { return (u64)lane_u32((u32)v, j) | ((u64)lane_u32((u32)(v >> 32), j) << 32); }

__global__ __launch_bounds__(256) void k_cons_prep(ConsArgs A) {
  const u64 i = (u64)blockIdx.x * 256u + threadIdx.x, n = A.n_reads;
  const ConsBounds B = cons_bounds(A);
  const u32 lane = threadIdx.x & 63u;
  const u32 longest = wave_max32(i < n ? A.lengths[i] : 0u);
  if (lane == 0u && longest) atomicMax(A.cnt + CONS_MAX_LEN, (u64)longest);
  bool invalid = false;
  if (i < B.P) {
    const u64 u = last_at_most(A.lay_offs, B.nu, i);
    if (A.lay_offs[u] <= i && i < A.lay_offs[u + 1]) {
      const u64 s0 = A.seq_offs[u], s1 = A.seq_offs[u + 1], U = s1 > s0 ? s1 - s0 : 0ull;
      const uint4 rec = reinterpret_cast<const uint4*>(A.layout)[i];
      const u64 o = (u64)rec.z | ((u64)rec.w << 32);
      invalid = !((u64)rec.x < n && o <= U && (u64)A.lengths[rec.x < n ? rec.x : 0u] <= U - o);
    }
  }
  const u32 tot = (u32)__popcll(__ballot(invalid));
  if (lane == 0u && tot) atomicAdd(counter_slot(A.cnt, CONS_C_INVALID), (u64)tot);
}

__global__ __launch_bounds__(256) void k_cons_vote(ConsArgs A) {
  const ConsBounds B = cons_bounds(A);
  const u64 n = A.n_reads;
  const u32 lane = threadIdx.x & 63u;
  const u64 waves = (u64)gridDim.x * 4u, tiles = (B.T + 63u) >> 6;
  const u64 longest = A.cnt[CONS_MAX_LEN];
  const uint4* lay = reinterpret_cast<const uint4*>(A.layout);
  u32 n_col = 0, n_chg = 0, n_shallow = 0, n_tie = 0, n_held = 0, deepest = 0;
  for (u64 t = (u64)blockIdx.x * 4u + (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); t < tiles; t += waves) {
    const u64 g = t * 64u + lane;
    bool active = g < B.T;
    const u64 u = active ? last_at_most(A.seq_offs, B.nu, g) : 0ull;
    const u64 s0 = A.seq_offs[u], s1 = A.seq_offs[u + 1];  // (tiles > 0: nu >= 1)
    active = active && s0 <= g && g < s1;
    const u64 U = s1 - s0, x = g - s0;
    u32 lo = 0, hi = 0;  // the placements of this lane's unitig
    if (active) {
      const u64 l0 = A.lay_offs[u], l1 = A.lay_offs[u + 1];
      lo = (u32)(l0 < n ? l0 : n);
      hi = (u32)(l1 < n ? l1 : n);
      if (lo > hi) lo = hi;
    }
    // the first placement of [lo, hi) with offset + longest > x
    u32 a = lo, b = hi;
    if (x >= longest) {
      const u64 below = x - longest;
      for (int step = 0; step < 32 && a < b; ++step) {
        const u32 mid = (a + b) >> 1;
        if (placement_offset(A.layout, mid) > below)
          b = mid;
        else
          a = mid + 1u;
      }
    }
    // (the same in every lane: readfirstlane tells the compiler so, and the walk below runs on scalars)
    const u32 pa = (u32)__builtin_amdgcn_readfirstlane((int)wave_min32(active ? a : 0xFFFFFFFFu));
    const u32 pb = (u32)__builtin_amdgcn_readfirstlane((int)wave_max32(hi));
    u32 cA = 0, cC = 0, cG = 0, cT = 0;
    bool finished = false;
    for (u32 base = pa; base < pb && !finished; base += 64u) {
      const u32 p = base + lane;
      uint4 rec = make_uint4(0xFFFFFFFFu, 0u, 0u, 0u);
      u32 len = 0;
      u64 from = 0;
      if (p < pb) {
        rec = lay[p];
        if ((u64)rec.x < n) {
          len = A.lengths[rec.x];
          from = A.offs[rec.x];
        }
      }
      const u32 held = pb - base < 64u ? pb - base : 64u;
      for (u32 j = 0; j < held; ++j) {
        const u32 pj = base + j;
        const u32 r = lane_u32(rec.x, j), fl = lane_u32(rec.y, j), L = lane_u32(len, j);
        const u64 o = (u64)lane_u32(rec.z, j) | ((u64)lane_u32(rec.w, j) << 32), src = lane_u64(from, j);
        const bool mine = pj >= lo && pj < hi;
        if (__all(pj >= hi || (mine && o > x))) {  // (a lane that is not active has hi = 0)
          finished = true;
          break;
        }
        const bool valid = (u64)r < n && o <= U && (u64)L <= U - o;
        if (mine && valid && x >= o && x - o < (u64)L) {
          const u64 rel = x - o;
          const bool rev = (fl & SIGAX_PLACED_REV) != 0u;
          const u64 at = src + (rev ? (u64)L - 1ull - rel : rel);
          u32 k = at < B.src_end ? letter_of(A.seqs[at]) : 4u;
          if (rev && k < 4u) k = 3u - k;
          cA += k == 0u;
          cC += k == 1u;
          cG += k == 2u;
          cT += k == 3u;
        }
      }
    }
    // the winner: the most votes, a tie to the earliest of A, C, G, T
    u32 w = 0, cw = cA;
    if (cC > cw) { w = 1u; cw = cC; }
    if (cG > cw) { w = 2u; cw = cG; }
    if (cT > cw) { w = 3u; cw = cT; }
    const u32 own = active ? A.useqs[g] : 0u, ko = letter_of(own);
    const u32 c_own = ko == 0u ? cA : ko == 1u ? cC : ko == 2u ? cG : ko == 3u ? cT : 0u;
    const u32 firsts = (cA == cw) + (cC == cw) + (cG == cw) + (cT == cw), depth = cA + cC + cG + cT;
    const bool more = active && cw > c_own, replace = more && cw >= A.min_votes;
    if (replace) A.useqs[g] = (unsigned char)(w == 0u ? 'A' : w == 1u ? 'C' : w == 2u ? 'G' : 'T');
    if (active && A.support) {
      const u32 s = replace ? cw : c_own;
      A.support[g] = (unsigned char)(s < 255u ? s : 255u);
    }
    n_col += active;
    n_chg += replace;
    n_shallow += active && depth < 2u;
    n_tie += active && ko < 4u && cw >= 1u && c_own == cw && firsts >= 2u;
    n_held += more && !replace;
    deepest = active && depth > deepest ? depth : deepest;
    // changed[u]: one add per tile where the tile lies in one unitig
    const u64 actives = __ballot(active), changes = __ballot(replace);
    if (changes) {
      const u64 u_first = shfl64(u, (u32)__ffsll((long long)actives) - 1u);
      if (__all(!active || u == u_first)) {
        if (lane == 0u) atomicAdd(&A.changed[u_first], (u32)__popcll(changes));
      } else if (replace) {
        atomicAdd(&A.changed[u], 1u);
      }
    }
  }
  wave_add(counter_slot(A.cnt, CONS_C_COLUMNS), n_col);
  wave_add(counter_slot(A.cnt, CONS_C_CHANGED), n_chg);
  wave_add(counter_slot(A.cnt, CONS_C_SHALLOW), n_shallow);
  wave_add(counter_slot(A.cnt, CONS_C_TIES), n_tie);
  wave_add(counter_slot(A.cnt, CONS_C_HELD), n_held);
  deepest = wave_max32(deepest);
  if (lane == 0u && deepest) atomicMax(A.cnt + CONS_MAX_DEPTH, (u64)deepest);
}

__global__ void k_cons_status(ConsArgs A) {
  if (threadIdx.x != 0u || blockIdx.x != 0u) return;
  const ConsBounds B = cons_bounds(A);
  A.status[0] = B.nu;
  A.status[1] = counter_total(A.cnt, CONS_C_COLUMNS);
  A.status[2] = counter_total(A.cnt, CONS_C_CHANGED);
  A.status[3] = counter_total(A.cnt, CONS_C_SHALLOW);
  A.status[4] = counter_total(A.cnt, CONS_C_TIES);
  A.status[5] = counter_total(A.cnt, CONS_C_HELD);
  A.status[6] = A.cnt[CONS_MAX_DEPTH];
  A.status[7] = counter_total(A.cnt, CONS_C_INVALID);
}

}  // namespace

hipError_t launch_consensus(const ConsArgs& a, hipStream_t st) {
  hipLaunchKernelGGL(k_cons_prep, dim3(blocks_of(a.n_reads)), dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_cons_vote, dim3(CONS_GRID), dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_cons_status, dim3(1), dim3(64), 0, st, a);
  return hipGetLastError();
}
