// siga_amd/csrc/sigax_pairs.hip -- `siga unitig --pairs` on the device (gfx950 / CDNA4, wave64): mate-pair statistics and the
// links between unitig ends, over the layout a unitig call left on the device.  It restates the reference's
// InsertSizeEstimateVisitor (src/bigraph_visitors.cpp:517-663) as a pass over placements: the visitor's chains are the unitigs,
// its distance along a chain is sigax_placement.offset.  The rules are in include/sigax.h and DESIGN.md 9h; the restatement the
// tests hold this against is tests/pair_cases.py::expected_pairs.
//   k_pair_where     one lane per placement: its unitig by bisection in lay_offs (at most 32 steps), where[read] = (unitig << 32)
//                    | (placement + 1).  `where` is zeroed first; an entry is only ever written from a placement inside the
//                    layout, so whatever it holds names a readable placement and a readable unitig.
//   k_pair_classify  1024 reads per workgroup, four per lane.  The smaller id of a pair classifies it.  Counts are taken with one
//                    ballot per class and read, after the loop; the sums are per-lane, then per-wave; lane 0 adds what is not zero to
//                    the wave's slot of each counter (counter_slot, sigax_device.h: 32 slots 256 bytes apart).  The 128-bit sums of
//                    squares add their low word and carry from the value that add returns.  The histogram is an LDS
//                    sub-histogram per workgroup, flushed with one global add per non-zero bin: spans of one library pile into a
//                    handful of bins.  A pair that joins a link appends (key, s) to a list -- one counter add per wave -- whose
//                    order the sort and the commutative reduction make irrelevant.
//   (device radix sort of the cap = n_reads / 2 list entries by key; empty entries are all ones and sort last)
//   k_pair_heads     one lane per sorted entry: it begins a run of equal keys; launch_scan numbers the runs
//   k_pair_init      a head writes its record {a, b, 0, 2^32 - 1, 0}
//   k_pair_reduce    one lane per sorted entry: count, minimum and sum into its run's record; a wave whose 64 entries are of one
//                    run reduces in registers and adds once
//   k_pair_status    status24 from the slots
// Every loop has a bound the host knows and every store is bounds-checked.  Plain vector stores and atomics only; integer work.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>

#include "sigax_device.h"
#include "sigax_kernels.h"

namespace {
constexpr u64 EMPTY = ~0ull;
// status entries that are counts of reads or pairs (one ballot each); 21 is the appended entries, 22 the scan's total
enum { ST_ENTRY = 0, ST_BAD = 1, ST_PAIRS = 2, ST_UNPLACED = 3, ST_SAME = 4, ST_INWARD = 5, ST_OUTWARD = 6, ST_TANDEM = 7, ST_RING = 8,
       ST_FAR = 9, ST_ND = 10, ST_SD = 11, ST_SD2 = 12, ST_NS = 14, ST_SS = 15, ST_SS2 = 16, ST_ACROSS = 18, ST_RINGDROP = 19, ST_OVER = 20,
       ST_LINKED = 21, ST_RECORDS = 22 };
constexpr u32 BALLOTED = 0x1C47FFu;  // bits 0-10, 14, 18-20

// the unitigs and the placements that can be read
__device__ __forceinline__ void pair_bounds(const PairArgs& A, u64& nu, u64& P) {
  nu = *A.n_unitigs;
  if (nu > A.n_reads) nu = A.n_reads;
  P = nu ? A.lay_offs[nu] : 0ull;
  if (P > A.n_reads) P = A.n_reads;
}

__global__ __launch_bounds__(256) void k_pair_where(PairArgs A) {
  const u64 p = (u64)blockIdx.x * 256u + threadIdx.x;
  u64 nu, P;
  pair_bounds(A, nu, P);
  if (p >= P) return;
  u64 lo = 0, hi = nu;  // (last_at_most, written out: through the helper the kernel's one 64-bit add swaps its operands)
  for (int step = 0; step < 32 && hi - lo > 1; ++step) {
    const u64 mid = (lo + hi) >> 1;
    if (A.lay_offs[mid] <= p)
      lo = mid;
    else
      hi = mid;
  }
  const u32 read = A.layout[p].read;
  if ((u64)read < A.n_reads) A.where[read] = (lo << 32) | (p + 1);
}

// a 128-bit sum of this wave's squares, given as the totals of their low and high 32-bit halves, into slots c (low) and c + 1
__device__ __forceinline__ void add_squares(const PairArgs& A, u32 c, u64 L, u64 H) {
  u64 hi = H >> 32;
  const u64 part = (H & 0xFFFFFFFFull) << 32, lo = L + part;
  hi += lo < L;
  if (lo) {
    const u64 old = atomicAdd(counter_slot(A.cnt, c), lo);
    hi += old + lo < old;
  }
  if (hi) atomicAdd(counter_slot(A.cnt, c + 1u), hi);
}

__global__ __launch_bounds__(256) void k_pair_classify(PairArgs A) {
  __shared__ u32 sub[PAIR_HIST_MAX];
  const u32 bins = A.hist_bins < (u32)PAIR_HIST_MAX ? A.hist_bins : (u32)PAIR_HIST_MAX;
  for (u32 b = threadIdx.x; b < bins; b += 256u) sub[b] = 0u;
  __syncthreads();
  const u64 n = A.n_reads;
  u64 nu, P;
  pair_bounds(A, nu, P);
  const bool outward = (A.flags & SIGAX_PAIRS_OUTWARD) != 0u;
  const u32 lane = threadIdx.x & 63u;
  u32 fs[PAIR_READS_PER_BLOCK / 256u];  // the classes of this lane's reads, one bit per counter
  u64 sd = 0, sd2l = 0, sd2h = 0, ss = 0, ss2l = 0, ss2h = 0;
#pragma unroll
  for (u32 it = 0; it < PAIR_READS_PER_BLOCK / 256u; ++it) {
    const u64 i = (u64)blockIdx.x * PAIR_READS_PER_BLOCK + it * 256u + threadIdx.x;
    u32 f = 0;
    u64 key = EMPTY, s = 0;
    const u32 m = i < n ? A.mate[i] : SIGAX_NO_MATE;
    if (m != SIGAX_NO_MATE) {
      f |= 1u << ST_ENTRY;
      const bool paired = (u64)m < n && m != (u32)i && A.mate[m] == (u32)i;
      if (!paired) {
        f |= 1u << ST_BAD;
      } else if ((u32)i < m) {
        f |= 1u << ST_PAIRS;
        const u64 wi = A.where[i], wj = A.where[m];
        const u64 pi = wi & 0xFFFFFFFFull, pj = wj & 0xFFFFFFFFull;
        const u64 ui = wi >> 32, uj = wj >> 32;
        if (pi == 0 || pj == 0 || pi > P || pj > P || ui >= nu || uj >= nu) {  // (the last four cannot be: k_pair_where)
          f |= 1u << ST_UNPLACED;
        } else {
          const uint4 ri = reinterpret_cast<const uint4*>(A.layout)[pi - 1], rj = reinterpret_cast<const uint4*>(A.layout)[pj - 1];
          const u64 li = (u64)ri.z | ((u64)ri.w << 32), lj = (u64)rj.z | ((u64)rj.w << 32);
          const u64 ei = li + A.lengths[i], ej = lj + A.lengths[m];
          const bool vi = (ri.y & SIGAX_PLACED_REV) != 0u, vj = (rj.y & SIGAX_PLACED_REV) != 0u;
          const bool ci = (A.uflags[ui] & SIGAX_UNITIG_CIRCULAR) != 0u;
          if (ui == uj) {
            if (ci) {
              f |= 1u << ST_RING;
            } else {
              f |= 1u << ST_SAME;
              const bool first = li <= lj;  // (i < m: the tie goes to i)
              const bool va = first ? vi : vj, vb = first ? vj : vi;
              const bool in = !va && vb, out = va && !vb;
              f |= 1u << (in ? ST_INWARD : out ? ST_OUTWARD : ST_TANDEM);
              const u64 d = first ? lj - li : li - lj;
              const u64 span = (ei > ej ? ei : ej) - (first ? li : lj);
              if (span >> 32) {
                f |= 1u << ST_FAR;
              } else {
                f |= 1u << ST_ND;
                const u64 d2 = d * d;
                sd += d;
                sd2l += d2 & 0xFFFFFFFFull;
                sd2h += d2 >> 32;
                if (outward ? out : in) {
                  f |= 1u << ST_NS;
                  const u64 s2 = span * span;
                  ss += span;
                  ss2l += s2 & 0xFFFFFFFFull;
                  ss2h += s2 >> 32;
                  const u64 bin = span >> A.hist_shift;
                  atomicAdd(&sub[bin < bins - 1u ? (u32)bin : bins - 1u], 1u);
                }
              }
            }
          } else {
            f |= 1u << ST_ACROSS;
            const bool cj = (A.uflags[uj] & SIGAX_UNITIG_CIRCULAR) != 0u;
            const bool fi = vi == outward, fj = vj == outward;  // the read faces end E
            const u64 gi = fi ? A.seq_offs[ui + 1] - A.seq_offs[ui] - li : ei;
            const u64 gj = fj ? A.seq_offs[uj + 1] - A.seq_offs[uj] - lj : ej;
            s = gi + gj;
            if (ci || cj) {
              f |= 1u << ST_RINGDROP;
            } else if (A.max_span != 0ull && s > A.max_span) {
              f |= 1u << ST_OVER;
            } else {
              const u64 a = 2ull * ui + (fi ? 1u : 0u), b = 2ull * uj + (fj ? 1u : 0u);
              key = a < b ? (a << 32) | b : (b << 32) | a;
            }
          }
        }
      }
    }
    fs[it] = f;
    // the wave's link entries, appended behind one add
    const u64 linkers = __ballot(key != EMPTY);
    if (linkers) {
      u64 base = 0;
      if (lane == 0u) base = atomicAdd(A.cnt + PAIR_APPENDED, (u64)__popcll(linkers));
      base = __shfl(base, 0, 64);
      const u64 at = base + (u64)__popcll(linkers & ((1ull << lane) - 1ull));
      if (key != EMPTY && at < A.cap) {
        A.keys[0][at] = key;
        A.vals[0][at] = s;
      }
    }
  }
  const u64 t_sd = wave_sum(sd), t_sd2l = wave_sum(sd2l), t_sd2h = wave_sum(sd2h);
  const u64 t_ss = wave_sum(ss), t_ss2l = wave_sum(ss2l), t_ss2h = wave_sum(ss2h);
#pragma unroll
  for (int c = 0; c < 21; ++c)
    if ((BALLOTED >> c) & 1u) {  // one ballot per class and read: the wave's count, one add when it is not zero
      u32 tot = 0;
#pragma unroll
      for (u32 it = 0; it < PAIR_READS_PER_BLOCK / 256u; ++it) tot += (u32)__popcll(__ballot((fs[it] >> c) & 1u));
      if (lane == 0u && tot) atomicAdd(counter_slot(A.cnt, (u32)c), (u64)tot);
    }
  if (lane == 0u) {
    if (t_sd) atomicAdd(counter_slot(A.cnt, ST_SD), t_sd);
    if (t_ss) atomicAdd(counter_slot(A.cnt, ST_SS), t_ss);
    if (t_sd2l | t_sd2h) add_squares(A, ST_SD2, t_sd2l, t_sd2h);
    if (t_ss2l | t_ss2h) add_squares(A, ST_SS2, t_ss2l, t_ss2h);
  }
  __syncthreads();
  for (u32 b = threadIdx.x; b < bins; b += 256u) {
    const u32 v = sub[b];
    if (v) atomicAdd(&A.hist[b], (u64)v);
  }
}

__global__ __launch_bounds__(256) void k_pair_heads(PairArgs A, const u64* __restrict__ ks) {
  const u64 t = (u64)blockIdx.x * 256u + threadIdx.x;
  if (t >= A.cap) return;
  const u64 key = ks[t];
  A.head[t] = key != EMPTY && (t == 0 || ks[t - 1] != key) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_pair_init(PairArgs A, const u64* __restrict__ ks) {
  const u64 t = (u64)blockIdx.x * 256u + threadIdx.x;
  if (t >= A.cap || A.head[t] == 0u) return;
  const u64 r = A.scan[t];
  if (r >= A.cap) return;
  const u64 key = ks[t];
  sigax_pair_link rec;
  rec.a = (u32)(key >> 32);
  rec.b = (u32)key;
  rec.count = 0u;
  rec.min_span = 0xFFFFFFFFu;
  rec.sum_span = 0ull;
  A.links[r] = rec;
}

__global__ __launch_bounds__(256) void k_pair_reduce(PairArgs A, const u64* __restrict__ ks, const u64* __restrict__ vs) {
  const u64 t = (u64)blockIdx.x * 256u + threadIdx.x;
  const bool valid = t < A.cap && ks[t] != EMPTY;
  u64 r = EMPTY, s = 0;
  if (valid) {
    r = A.scan[t] + A.head[t] - 1ull;  // (an entry that is no head has its head before it)
    s = vs[t];
  }
  u32 mn = s > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)s;
  const u64 r0 = __shfl(r, 0, 64);
  if (__all(valid && r == r0)) {  // the whole wave in one run
    const u64 sum = wave_sum(s);
    for (int o = 32; o > 0; o >>= 1) {  // (not wave_min32: its shuffle of an int compiles to other code here)
      const u32 other = __shfl_xor(mn, o, 64);
      mn = other < mn ? other : mn;
    }
    if ((threadIdx.x & 63u) == 0u && r < A.cap) {
      atomicAdd(&A.links[r].count, 64u);
      atomicMin(&A.links[r].min_span, mn);
      atomicAdd((u64*)&A.links[r].sum_span, sum);
    }
  } else if (valid && r < A.cap) {
    atomicAdd(&A.links[r].count, 1u);
    atomicMin(&A.links[r].min_span, mn);
    atomicAdd((u64*)&A.links[r].sum_span, s);
  }
}

__global__ void k_pair_status(PairArgs A) {
  if (threadIdx.x != 0u || blockIdx.x != 0u) return;
  auto slot = [&](u32 c, u32 s) { return A.cnt[((u64)c * TRIM_SLOTS + s) * TRIM_STRIDE]; };
  for (u32 c = 0; c < PAIR_COUNTERS; ++c) {
    if (c == ST_SD2 || c == ST_SS2) {  // 128 bits over slots c and c + 1
      u64 lo = 0, hi = 0;
      for (u32 s = 0; s < TRIM_SLOTS; ++s) {
        const u64 v = slot(c, s);
        lo += v;
        hi += (lo < v) + slot(c + 1u, s);
      }
      A.status[c] = lo;
      A.status[c + 1u] = hi;
      ++c;
      continue;
    }
    u64 v = 0;  // (counter_total, through the lambda the 128-bit sums need)
    for (u32 s = 0; s < TRIM_SLOTS; ++s) v += slot(c, s);
    A.status[c] = v;
  }
  const u64 appended = A.cnt[PAIR_APPENDED];
  A.status[ST_LINKED] = appended < A.cap ? appended : A.cap;
  A.status[ST_RECORDS] = *A.scan_total;
  A.status[23] = 0ull;
}

}  // namespace

hipError_t pairs_sort_bytes(u64 cap, u64* bytes) {
  size_t tb = 0;
  *bytes = 0;
  if (cap == 0) return hipSuccess;
  const hipError_t e = rocprim::radix_sort_pairs(nullptr, tb, (const u64*)nullptr, (u64*)nullptr, (const u64*)nullptr, (u64*)nullptr, (size_t)cap, 0u, 64u);
  *bytes = tb;
  return e;
}

hipError_t launch_pairs(const PairArgs& a, hipStream_t st) {
  const u64 n = a.n_reads;
  const unsigned per_read = blocks_of(n), per_block = (unsigned)((n + PAIR_READS_PER_BLOCK - 1) / PAIR_READS_PER_BLOCK);
  hipLaunchKernelGGL(k_pair_where, dim3(per_read), dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_pair_classify, dim3(per_block), dim3(256), 0, st, a);
  if (a.cap) {
    size_t tb = (size_t)a.sort_tmp_bytes;
    const hipError_t e = rocprim::radix_sort_pairs(a.sort_tmp, tb, (const u64*)a.keys[0], a.keys[1], (const u64*)a.vals[0], a.vals[1], (size_t)a.cap, 0u, 64u, st);
    if (e != hipSuccess) return e;
    const unsigned per_entry = blocks_of(a.cap);
    hipLaunchKernelGGL(k_pair_heads, dim3(per_entry), dim3(256), 0, st, a, (const u64*)a.keys[1]);
    launch_scan(a.head, a.cap, a.partial, a.scan, a.scan_total, st);
    hipLaunchKernelGGL(k_pair_init, dim3(per_entry), dim3(256), 0, st, a, (const u64*)a.keys[1]);
    hipLaunchKernelGGL(k_pair_reduce, dim3(per_entry), dim3(256), 0, st, a, (const u64*)a.keys[1], (const u64*)a.vals[1]);
  }
  hipLaunchKernelGGL(k_pair_status, dim3(1), dim3(64), 0, st, a);
  return hipGetLastError();
}
