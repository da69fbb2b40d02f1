// siga_amd/csrc/sigax_scaffold.hip -- `siga unitig --scaffold` on the device (gfx950 / CDNA4, wave64): unitigs joined through the
// link records the pairs call left, with a run of N for every gap.  A scaffold is the unitig of sigax_unitig.hip with unitig
// for read, unitig end for read end and a gap for an overlap; the kernels below follow k_uni_* step by step over an argument
// block of their own.  The rules are in include/sigax.h and DESIGN.md 9i; the restatement the tests hold this against is
// tests/scaffold_cases.py::expected_scaffolds.
//
// A unitig has two ends, B = 0 and E = 1; state 2u + e = "unitig u, left through end e".
//   k_scaf_clear     the call's scratch emptied: counters, best, deg, link (NIL), closing
//   k_scaf_classify  one lane per link: its class; a candidate raises best[a] and best[b] to its count (atomicMax behind a
//                    plain compare)
//   k_scaf_degree    one lane per link: a candidate is weak or strong; a strong one adds to deg[a] and deg[b] (atomicAdd behind
//                    a plain compare: a degree of 2 says all that is ever asked of it)
//   k_scaf_joins     one lane per link, after the degrees are final: a strong candidate with deg 1 at both ends is a join and
//                    writes link[a] = {b, gap}, link[b] = {a, gap}.  deg[e] == 1 means one strong candidate touches e, so one
//                    lane writes link[e]; the rest are ambiguous
//   k_scaf_init / k_scaf_jump   list ranking by pointer jumping over the 2 max_unitigs states, `rounds` = ceil(log2
//                    max_unitigs) + 1 launches the host counts; a hop into unitig y over a gap adds gap + bases(y)
//   k_scaf_cut       the lane of a cycle's smallest unitig takes the join into its B end out and notes its gap; ranking runs
//                    once more (its launches leave at once when nothing was cut)
//   k_scaf_heads     one lane per unitig: a head gives its scaffold's unitigs and bases; launch_scan numbers and places them
//   k_scaf_place     one lane per unitig: its placement record, for a head the scaffold's table entries, and for the bases pass
//                    where the unitig goes, where it comes from and how long it is
//   k_scaf_status    status16 from the slots and the scans
//   k_scaf_bases     one lane per 16-byte piece of the output.  A wave finds the placement of its first byte by one bisection over
//                    pdst and keeps the 64 descriptors from there on in LDS; a lane finds its own among them in at most 6 LDS
//                    steps (beyond them: the bisection again).  Then a run of N, one 16-byte load and store (forward), the
//                    mirrored 16 bytes complemented in registers (reverse), or bytes where the piece crosses a boundary
// Counters are per-wave sums into 32 slots 256 bytes apart (counter_slot, sigax_device.h).  Every loop has a bound the host knows and
// every access is bounds-checked.  Plain vector stores and atomics only; integer work, no LDS beyond those descriptors.
#include <hip/hip_runtime.h>

#include "sigax_device.h"
#include "sigax_kernels.h"

namespace {
constexpr u32 NIL = 0xFFFFFFFFu;
// status entries
enum { ST_SCAFFOLDS = 0, ST_BASES = 1, ST_LINKS = 2, ST_MALFORMED = 3, ST_SELF = 4, ST_CIRCULAR = 5, ST_SHORT = 6, ST_THIN = 7, ST_WEAK = 8,
       ST_AMBIGUOUS = 9, ST_JOINS = 10, ST_CYCLES = 11, ST_GAP_BASES = 12, ST_BELOW = 13, ST_CLAMPED = 14, ST_NO_ROOM = 15 };
constexpr u32 CANDIDATE = 0u;  // a class that is no status entry

// this wave's lanes with `on` set, added once to counter c
__device__ __forceinline__ void count_lanes(const ScaffoldArgs& A, u32 c, bool on) {
  const u64 m = __ballot(on);
  if (m && (threadIdx.x & 63u) == 0u) atomicAdd(counter_slot(A.cnt, c), (u64)__popcll(m));
}
__device__ __forceinline__ u64 n_unitigs(const ScaffoldArgs& A) {
  const u64 nu = *A.n_unitigs;
  return nu < A.max_unitigs ? nu : A.max_unitigs;
}
__device__ __forceinline__ u64 n_links(const ScaffoldArgs& A) {
  if (A.max_links == 0) return 0ull;  // (no table, and no count of it either)
  const u64 nl = *A.n_links;
  return nl < A.max_links ? nl : A.max_links;
}
__device__ __forceinline__ u64 unitig_bases(const ScaffoldArgs& A, u64 u) { return A.seq_offs[u + 1] - A.seq_offs[u]; }
__device__ __forceinline__ u64 insert_size(const ScaffoldArgs& A) {
  if (A.flags & SIGAX_SCAFFOLD_INSERT_FROM_STATUS) {
    const u64 n = A.status24[14];
    return n ? A.status24[15] / n : 0ull;
  }
  return A.insert_size;
}
__device__ __forceinline__ sigax_pair_link load_link(const ScaffoldArgs& A, u64 i) {
  const u64* p = reinterpret_cast<const u64*>(A.links + i);  // 24 bytes, 8-byte aligned
  const u64 x = p[0], y = p[1];
  sigax_pair_link r;
  r.a = (u32)x;
  r.b = (u32)(x >> 32);
  r.count = (u32)y;
  r.min_span = (u32)(y >> 32);
  r.sum_span = p[2];
  return r;
}
__device__ __forceinline__ u32 link_class(const ScaffoldArgs& A, u64 nu, const sigax_pair_link& r) {
  if ((u64)r.a >= 2 * nu || (u64)r.b >= 2 * nu || r.a >= r.b || r.count == 0u) return ST_MALFORMED;
  const u32 ua = r.a >> 1, ub = r.b >> 1;
  if (ua == ub) return ST_SELF;
  if ((A.uflags[ua] | A.uflags[ub]) & SIGAX_UNITIG_CIRCULAR) return ST_CIRCULAR;
  const u64 mb = A.min_unitig_bases;
  if (unitig_bases(A, ua) < mb || unitig_bases(A, ub) < mb) return ST_SHORT;
  if (r.count < A.min_pairs) return ST_THIN;
  return CANDIDATE;
}
// over final best[]
__device__ __forceinline__ bool is_weak(const ScaffoldArgs& A, const sigax_pair_link& r) {
  if (A.link_ratio == 0u) return false;
  const u64 v = (u64)r.count * A.link_ratio;
  return v <= (u64)A.best[r.a] || v <= (u64)A.best[r.b];
}

__global__ __launch_bounds__(256) void k_scaf_clear(ScaffoldArgs A) {
  const u64 t = (u64)blockIdx.x * 256u + threadIdx.x;
  if (t < SCAF_WORDS) A.cnt[t] = 0ull;
  if (t < 2 * A.max_unitigs) {
    A.best[t] = 0u;
    A.deg[t] = 0u;
    A.link[t] = make_uint2(NIL, 0u);
  }
  if (t < A.max_unitigs) A.closing[t] = 0u;
}

__global__ __launch_bounds__(256) void k_scaf_classify(ScaffoldArgs A) {
  const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
  const u64 nu = n_unitigs(A), nl = n_links(A);
  u32 cls = NIL;
  if (i < nl) {
    const sigax_pair_link r = load_link(A, i);
    cls = link_class(A, nu, r);
    if (cls == CANDIDATE) {  // best[] only grows: a stale value is smaller, and then the atomic decides
      if (A.best[r.a] < r.count) atomicMax(&A.best[r.a], r.count);
      if (A.best[r.b] < r.count) atomicMax(&A.best[r.b], r.count);
    }
  }
#pragma unroll
  for (u32 c = ST_MALFORMED; c <= ST_THIN; ++c) count_lanes(A, c, cls == c);
}

__global__ __launch_bounds__(256) void k_scaf_degree(ScaffoldArgs A) {
  const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
  const u64 nu = n_unitigs(A), nl = n_links(A);
  bool weak = false;
  if (i < nl) {
    const sigax_pair_link r = load_link(A, i);
    if (link_class(A, nu, r) == CANDIDATE) {
      weak = is_weak(A, r);
      if (!weak) {  // deg[] only grows and is asked for 1 or not 1: at 2 it says all it ever will
        if (A.deg[r.a] < 2u) atomicAdd(&A.deg[r.a], 1u);
        if (A.deg[r.b] < 2u) atomicAdd(&A.deg[r.b], 1u);
      }
    }
  }
  count_lanes(A, ST_WEAK, weak);
}

__global__ __launch_bounds__(256) void k_scaf_joins(ScaffoldArgs A) {
  const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
  const u64 nu = n_unitigs(A), nl = n_links(A);
  bool join = false, ambiguous = false, below = false, clamped = false;
  u64 gap = 0;
  if (i < nl) {
    const sigax_pair_link r = load_link(A, i);
    if (link_class(A, nu, r) == CANDIDATE && !is_weak(A, r)) {
      if (A.deg[r.a] == 1u && A.deg[r.b] == 1u) {
        join = true;
        const u64 ins = insert_size(A), m = r.sum_span / r.count;
        if (m >= ins) {
          gap = A.min_gap;
          below = true;
        } else {
          gap = ins - m;
          if (gap < A.min_gap) {
            gap = A.min_gap;
            below = true;
          } else if (gap > A.max_gap) {
            gap = A.max_gap;
            clamped = true;
          }
        }
        A.link[r.a] = make_uint2(r.b, (u32)gap);
        A.link[r.b] = make_uint2(r.a, (u32)gap);
      } else {
        ambiguous = true;
      }
    }
  }
  count_lanes(A, ST_AMBIGUOUS, ambiguous);
  count_lanes(A, ST_JOINS, join);
  count_lanes(A, ST_BELOW, below);
  count_lanes(A, ST_CLAMPED, clamped);
  wave_add(counter_slot(A.cnt, ST_GAP_BASES), gap);
}

// rk[s] = {successor or NIL, state reached so far, hops so far, smallest unitig id so far}; dist[s] = bases so far: a hop into
// unitig y over a gap adds gap + bases(y).  second: the ranking after the cut, which has nothing to do when nothing was cut.
__global__ __launch_bounds__(256) void k_scaf_init(ScaffoldArgs A, uint4* __restrict__ rk, u64* __restrict__ dist, int second) {
  if (second && A.cnt[SCAF_ANY_CUT] == 0ull) return;
  const u64 s = (u64)blockIdx.x * 256u + threadIdx.x;
  if (s >= 2 * A.max_unitigs) return;
  const u64 nu = n_unitigs(A);
  const uint2 lk = A.link[s];
  const u32 u = (u32)(s >> 1);
  if (s >= 2 * nu || lk.x == NIL || (u64)lk.x >= 2 * nu) {
    rk[s] = make_uint4(NIL, (u32)s, 0u, u);
    dist[s] = 0;
  } else {
    const u32 y = lk.x >> 1, nx = lk.x ^ 1u;
    rk[s] = make_uint4(nx, nx, 1u, u < y ? u : y);
    dist[s] = unitig_bases(A, y) + lk.y;
  }
}

__global__ __launch_bounds__(256) void k_scaf_jump(ScaffoldArgs A, const uint4* __restrict__ in, const u64* __restrict__ din,
                                                   uint4* __restrict__ out, u64* __restrict__ dout, int second) {
  if (second && A.cnt[SCAF_ANY_CUT] == 0ull) return;
  const u64 s = (u64)blockIdx.x * 256u + threadIdx.x;
  if (s >= 2 * A.max_unitigs) return;
  uint4 a = in[s];
  u64 d = din[s];
  if (a.x != NIL && (u64)a.x < 2 * A.max_unitigs) {
    const uint4 b = in[a.x];
    d += din[a.x];
    a = make_uint4(b.x, b.y, a.z + b.z, a.w < b.w ? a.w : b.w);
  }
  out[s] = a;
  dout[s] = d;
}

__global__ __launch_bounds__(256) void k_scaf_cut(ScaffoldArgs A, const uint4* __restrict__ rk) {
  const u64 m = (u64)blockIdx.x * 256u + threadIdx.x;
  const u64 nu = n_unitigs(A);
  bool cut = false;
  u64 gap = 0;
  if (m < nu) {
    const uint4 a = rk[2 * m];
    if (a.x != NIL && a.w == (u32)m) {  // on a cycle, and its smallest unitig: the one lane of the cycle that acts
      const uint2 lk = A.link[2 * m];
      if (lk.x != NIL && (u64)lk.x < 2 * nu) {
        A.link[2 * m] = make_uint2(NIL, 0u);
        A.link[lk.x] = make_uint2(NIL, 0u);
        A.closing[m] = 1u | (lk.y << 1);
        A.cnt[SCAF_ANY_CUT] = 1ull;  // (every writer writes the same word)
        gap = lk.y;
        cut = true;
      }
    }
  }
  count_lanes(A, ST_CYCLES, cut);
  wave_add(counter_slot(A.cnt, SCAF_C_CLOSING_GAPS), gap);
}

__global__ __launch_bounds__(256) void k_scaf_heads(ScaffoldArgs A, const uint4* __restrict__ rk, const u64* __restrict__ dist) {
  const u64 r = (u64)blockIdx.x * 256u + threadIdx.x;
  const u64 n = A.max_unitigs;
  if (r >= n) return;
  u32 one = 0, units = 0;
  u64 bases = 0;
  if (r < n_unitigs(A)) {
    const uint4 a0 = rk[2 * r], a1 = rk[2 * r + 1];
    const u32 d = head_dir(a0, a1);
    const uint4 to = d ? a1 : a0, away = d ? a0 : a1;
    if (to.z == 0u && to.x == NIL) {  // nothing between r and the head: r is it
      one = 1;
      units = away.z + 1u;
      bases = unitig_bases(A, r) + dist[2 * r + (d ^ 1u)];
    }
  }
  A.hcnt[r] = one;
  A.hcnt[(n + 1) + r] = units;
  A.hcnt[2 * (n + 1) + r] = (u32)bases;
  A.hcnt[3 * (n + 1) + r] = (u32)(bases >> 32);
}

__global__ __launch_bounds__(256) void k_scaf_place(ScaffoldArgs A, const uint4* __restrict__ rk, const u64* __restrict__ dist) {
  const u64 r = (u64)blockIdx.x * 256u + threadIdx.x;
  const u64 n = A.max_unitigs;
  if (r >= n) return;
  const u64 *snum = A.scan, *layr = A.scan + (n + 1), *lo = A.scan + 2 * (n + 1), *hi = A.scan + 3 * (n + 1);
  if (r < n_unitigs(A)) {
    const uint4 a0 = rk[2 * r], a1 = rk[2 * r + 1];
    const u32 d = head_dir(a0, a1);
    const uint4 to = d ? a1 : a0;
    const u64 h = to.y >> 1;  // the head
    if (h < n) {
      const u64 off = dist[2 * r + d], slot = layr[h] + to.z, seq0 = lo[h] + (hi[h] << 32);
      if (slot < n) {
        // entered through the end it is left through on the way to the head: through B = forward
        reinterpret_cast<uint4*>(A.sc_layout)[slot] = make_uint4((u32)r, d ? SIGAX_PLACED_REV : 0u, (u32)off, (u32)(off >> 32));
        A.pdst[slot] = seq0 + off;
        A.psrc[slot] = A.seq_offs[r] | ((u64)d << 63);
        A.plen[slot] = unitig_bases(A, r);
      }
      if (to.z == 0u && to.x == NIL) {  // the head writes its scaffold's entries
        const u64 s = snum[r];
        if (s < n) {
          A.sc_offs[s] = seq0;
          A.sc_lay_offs[s] = layr[r];
          A.sc_flags[s] = A.closing[r];
        }
      }
    }
  }
  if (r == 0) {
    const u64 S = snum[n], bases = lo[n] + (hi[n] << 32), placed = layr[n];
    if (S <= n) {
      A.sc_offs[S] = bases;
      A.sc_lay_offs[S] = placed;
    }
    if (placed <= n) A.pdst[placed] = bases;
  }
}

// one wave: lane c < 16 sums the 32 slots of counter c and writes status entry c
__global__ __launch_bounds__(64) void k_scaf_status(ScaffoldArgs A) {
  const u32 c = threadIdx.x;
  if (blockIdx.x != 0u) return;
  const u64 n = A.max_unitigs;
  const u64 v = c < SCAF_COUNTERS ? counter_total(A.cnt, c) : 0ull;
  const u64 closing_gaps = __shfl(v, SCAF_C_CLOSING_GAPS, 64), joins = __shfl(v, ST_JOINS, 64), cycles = __shfl(v, ST_CYCLES, 64);
  const u64 bases = A.scan[2 * (n + 1) + n] + (A.scan[3 * (n + 1) + n] << 32);
  u64 out = v;
  if (c == ST_SCAFFOLDS) out = A.scan[n];
  if (c == ST_BASES) out = bases;
  if (c == ST_LINKS) out = n_links(A);
  if (c == ST_JOINS) out = joins - (cycles < joins ? cycles : joins);  // a cycle's closing join is not merged
  if (c == ST_GAP_BASES) out = v - closing_gaps;
  if (c == ST_NO_ROOM) out = bases > A.sseqs_capacity ? 1ull : 0ull;
  if (c < 16u) A.status[c] = out;
}

// what a wave keeps in LDS of the placements its 1024 output bytes begin in: 64 descriptors from the first byte's placement on
struct ScafSh {
  u64 dst[4][65];
  u64 src[4][64];
  u64 len[4][64];
};
struct ScafDesc {
  u64 d0, len, src, next;  // where the unitig begins in the output, its bases, psrc, where the next placement begins
};

__global__ __launch_bounds__(256) void k_scaf_bases(ScaffoldArgs A) {
  __shared__ ScafSh sh;
  const u32 wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63u;
  const u64 n = A.max_unitigs;
  const u64 total = A.scan[2 * (n + 1) + n] + (A.scan[3 * (n + 1) + n] << 32);
  u64 P = A.scan[(n + 1) + n];  // the placements
  if (P > n) P = n;
  const bool live = total <= A.sseqs_capacity && P != 0;
  const u64 wb = ((u64)blockIdx.x * 4u + wave) * 1024ull;  // the wave's first output byte
  const u64 b = wb + 16ull * lane;
  const u64* __restrict__ D = A.pdst;
  // the placement of output byte p: the last k with D[k] <= p
  auto find = [&](u64 p) -> u64 { return last_at_most(D, P, p); };
  // one bisection per wave (its operands are the wave's alone), then 64 descriptors side by side
  u64 k0 = 0;
  u32 cnt = 0;
  if (live && wb < total) {
    k0 = find(wb);
    cnt = (u32)(P - k0 < 64 ? P - k0 : 64);
  }
  if (lane < cnt) {
    sh.dst[wave][lane] = D[k0 + lane];
    sh.src[wave][lane] = A.psrc[k0 + lane];
    sh.len[wave][lane] = A.plen[k0 + lane];
  }
  if (lane == 0u && cnt) sh.dst[wave][cnt] = D[k0 + cnt];
  __syncthreads();
  if (!live || b >= total) return;
  const u64* Dw = sh.dst[wave];
  // the placement of byte p >= wb: in the window by at most 6 LDS steps, beyond it by the bisection over the whole table.  (Not
  // last_at_most: the window is in LDS, indexed in 32 bits, and its search ends with the test whether p lies beyond it.)
  auto locate = [&](u64 p) -> u64 {
    u32 lo = 0, hi = cnt;
    while (hi - lo > 1u) {
      const u32 mid = (lo + hi) >> 1;
      if (Dw[mid] <= p)
        lo = mid;
      else
        hi = mid;
    }
    if (lo + 1u == cnt && k0 + cnt < P && Dw[cnt] <= p) return find(p);
    return k0 + lo;
  };
  auto desc = [&](u64 k) -> ScafDesc {
    ScafDesc d;
    if (k >= k0 && k - k0 < cnt) {
      const u32 j = (u32)(k - k0);
      d.d0 = Dw[j];
      d.len = sh.len[wave][j];
      d.src = sh.src[wave][j];
      d.next = Dw[j + 1];
    } else {
      d.d0 = D[k];
      d.len = A.plen[k];
      d.src = A.psrc[k];
      d.next = D[k + 1];
    }
    return d;
  };
  // output byte p, which lies in the placement of d or in the gap behind it
  auto fetch = [&](u64 p, const ScafDesc& d) -> u32 {
    const u64 rel = p - d.d0;
    if (rel >= d.len) return 'N';
    const bool rev = (d.src >> 63) != 0ull;
    const u64 s0 = d.src & ~(1ull << 63);
    const u64 at = rev ? s0 + (d.len - 1ull - rel) : s0 + rel;
    if (at >= A.useqs_bytes) return 'N';  // (no consistent input comes here)
    const u32 c = A.useqs[at];
    return rev ? comp_byte(c) : c;
  };
  unsigned char* out = A.sseqs;
  ScafDesc d = desc(locate(b));
  const u64 end = d.d0 + d.len;
  const bool whole = b + 16 <= total && b >= d.d0 && end >= d.d0;
  if (whole && b + 16 <= end) {  // inside one unitig
    const u64 rel = b - d.d0;
    const bool rev = (d.src >> 63) != 0ull;
    const u64 s0 = d.src & ~(1ull << 63);
    const u64 from = rev ? s0 + (d.len - rel - 16ull) : s0 + rel;  // a reverse stretch reads the mirrored 16 bytes
    uint4 v;
    if (from + 16 > A.useqs_bytes || from + 16 < from) {
      unsigned char t[16];
      for (u32 j = 0; j < 16; ++j) t[j] = (unsigned char)fetch(b + j, d);
      __builtin_memcpy(&v, t, 16);
    } else {
      uint4 w;
      if ((from & 15ull) == 0ull)
        w = *reinterpret_cast<const uint4*>(A.useqs + from);
      else
        __builtin_memcpy(&w, A.useqs + from, 16);  // (no alignment: the compiler picks the access)
      if (rev) {
        // byte j of the piece = complement of byte 15 - j of the load (written out in each bases kernel: as a shared
        // function it compiles to other code, and these kernels stay as they are)
        const u32 x[4] = {w.w, w.z, w.y, w.x};
        u32 y[4];
#pragma unroll
        for (u32 q = 0; q < 4; ++q) {
          const u32 e = x[q];
          y[q] = comp_byte(e >> 24) | (comp_byte((e >> 16) & 255u) << 8) | (comp_byte((e >> 8) & 255u) << 16) | (comp_byte(e & 255u) << 24);
        }
        v = make_uint4(y[0], y[1], y[2], y[3]);
      } else {
        v = w;
      }
    }
    *reinterpret_cast<uint4*>(out + b) = v;
  } else if (whole && b >= end && b + 16 <= d.next) {  // inside one gap
    *reinterpret_cast<uint4*>(out + b) = make_uint4(0x4E4E4E4Eu, 0x4E4E4E4Eu, 0x4E4E4E4Eu, 0x4E4E4E4Eu);
  } else {  // a piece over a boundary: bytes; a byte beyond the placement at hand finds its own
    const u64 to = b + 16 < total ? b + 16 : total;
    for (u64 p = b; p < to; ++p) {
      if (p < d.d0 || p >= d.next) d = desc(locate(p));
      out[p] = (unsigned char)fetch(p, d);
    }
  }
}

}  // namespace

void launch_scaffold_bases(const ScaffoldArgs& a, hipStream_t st) {
  if (a.max_unitigs == 0 || !a.sseqs || a.sseqs_capacity == 0) return;
  hipLaunchKernelGGL(k_scaf_bases, dim3(blocks_of((a.sseqs_capacity + 15) / 16)), dim3(256), 0, st, a);
}

hipError_t launch_scaffold(const ScaffoldArgs& a, hipStream_t st) {
  const u64 n = a.max_unitigs, ns = 2 * n, nl = a.max_links;
  if (n == 0) return hipSuccess;
  const u64 clear = ns > (u64)SCAF_WORDS ? ns : (u64)SCAF_WORDS;
  hipLaunchKernelGGL(k_scaf_clear, dim3(blocks_of(clear)), dim3(256), 0, st, a);
  if (nl) {
    hipLaunchKernelGGL(k_scaf_classify, dim3(blocks_of(nl)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_scaf_degree, dim3(blocks_of(nl)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_scaf_joins, dim3(blocks_of(nl)), dim3(256), 0, st, a);
  }
  const unsigned rounds = unitig_rounds(n);
  uint4* rk[2] = {reinterpret_cast<uint4*>(a.rank[0]), reinterpret_cast<uint4*>(a.rank[1])};
  for (int pass = 0; pass < 2; ++pass) {
    hipLaunchKernelGGL(k_scaf_init, dim3(blocks_of(ns)), dim3(256), 0, st, a, rk[0], a.dist[0], pass);
    for (unsigned r = 0; r < rounds; ++r)
      hipLaunchKernelGGL(k_scaf_jump, dim3(blocks_of(ns)), dim3(256), 0, st, a, (const uint4*)rk[r & 1], (const u64*)a.dist[r & 1], rk[(r & 1) ^ 1],
                         a.dist[(r & 1) ^ 1], pass);
    if (pass == 0) hipLaunchKernelGGL(k_scaf_cut, dim3(blocks_of(n)), dim3(256), 0, st, a, (const uint4*)rk[rounds & 1]);
  }
  const uint4* fin = rk[rounds & 1];
  const u64* fdist = a.dist[rounds & 1];
  hipLaunchKernelGGL(k_scaf_heads, dim3(blocks_of(n)), dim3(256), 0, st, a, fin, fdist);
  for (int k = 0; k < 4; ++k) launch_scan(a.hcnt + (u64)k * (n + 1), n, a.partial, a.scan + (u64)k * (n + 1), a.scan_total, st);
  hipLaunchKernelGGL(k_scaf_place, dim3(blocks_of(n)), dim3(256), 0, st, a, fin, fdist);
  hipLaunchKernelGGL(k_scaf_status, dim3(1), dim3(64), 0, st, a);
  launch_scaffold_bases(a, st);
  return hipGetLastError();
}
