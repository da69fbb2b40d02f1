// siga_amd/csrc/sigax_gapfill.hip -- `siga unitig --scaffold --gapfill` on the device (gfx950 / CDNA4, wave64): the gaps of the
// scaffolds closed by k-mer walks over the FM-index of the reads.  The rules are in include/sigax.h and DESIGN.md 9k; the
// restatement the tests hold this against is tests/gapfill_cases.py::expected_gapfill.
//
//   k_gap_classify  one lane per placement: its scaffold (one bisection), its unitig's place in useqs, whether it and the next
//                   placement are a gap, G, the classes that need no walk, the bytes of walk scratch the gap needs, and the
//                   four windows of its two walks as 2-bit codes
//   launch_scan     the gaps' numbers and where each gap's walk scratch begins
//   k_gap_walk      the walks.  A persistent grid; a GROUP of 8 lanes takes a gap from one global counter (grab_chains,
//                   sigax_rank.h) and keeps it until both walks are done.  One extension is the unit of work: count(w[1:] + b) for
//                   the four b is eight backward searches of k symbols on the forward strand, one per lane -- lanes 0-3 the
//                   candidate as it stands (it ends in b, so the four chains differ from their first symbol on), lanes 4-7 its
//                   reverse complement (the four share k - 1 symbols and so every granule but the last: their loads fall on
//                   the same lines).  Two shuffles and a ballot give the group its candidates.  The window lives in registers,
//                   four 64-bit words; a wave carries 8 walks in lockstep, and a group whose gap is done takes the next number
//                   in the same iteration.  Latency-bound gathers, integer work, no MFMA: the speed comes from the walks in
//                   flight, not from one walk.
//   launch_scan     the fill and the N it replaces, summed over the placements before each one
//   k_gap_lengths   one lane per scaffold: its new bases; launch_scan gives sc_offs'
//   k_gap_place     one lane per placement: its new offset, where it goes in sseqs, the gap's record, the counters
//   k_gap_status    status24
//   k_gap_bases     one lane per 16-byte piece of the output, as k_scaf_bases: the piece's placement by bisection, then a unitig's
//                   16 bytes (mirrored and complemented when it lies reversed) or bytes where the piece meets a gap or a boundary
// Every loop has a bound the host knows and every access is bounds-checked.  Plain vector stores and atomics only.
#include <hip/hip_runtime.h>

#include "sigax_device.h"
#include "sigax_kernels.h"
#include "sigax_rank.h"

namespace {

// ---- tables ---------------------------------------------------------------------------------------------------------------------
// (the tables' bounds, scaffold_of and placement_offset are sigax_device.h's)
// this wave's sum of v, added once to counter c
__device__ __forceinline__ void count_sum(const GapfillArgs& A, u32 c, u64 v) { wave_add(&A.cnt[c], v); }

// window w of placement p from k rank codes: base i (rank r(i), 1 .. 4) goes to bits 2 i of its four words; unused bits are 0
template <typename R>
__device__ __forceinline__ void window_write(u64* win, u32 k, R rank_of) {
  u64 acc = 0;
  for (u32 i = 0; i < k; ++i) {
    acc |= (u64)((rank_of(i) - 1u) & 3u) << (2u * (i & 31u));
    if ((i & 31u) == 31u || i + 1u == k) {
      win[i >> 5] = acc;
      acc = 0;
    }
  }
  for (u32 w = (k + 31u) >> 5; w < 4u; ++w) win[w] = 0ull;
}

__global__ __launch_bounds__(256) void k_gap_classify(GapfillArgs A) {
  const u64 p = (u64)blockIdx.x * 256u + threadIdx.x;
  if (p >= A.max_unitigs) return;
  const ScafBounds c = scaffold_bounds(A);
  const u32 k = A.k;
  u32 cls = GAP_NONE, gap = 0, need = 0, s = 0;
  u64 len = 0, src = 0, G = 0;
  if (p < c.P) {
    s = (u32)scaffold_of(A, c.S, p);
    // a placement's unitig: where it lies and how long it is; a bad one has no bases
    auto unitig = [&](u64 q, u64& at, u64& bases, bool& rev) {
      const uint4 v = reinterpret_cast<const uint4*>(A.sc_layout)[q];
      rev = (v.y & SIGAX_PLACED_REV) != 0u;
      at = bases = 0;
      if ((u64)v.x >= c.nu) return false;
      const u64 a = A.seq_offs[v.x], b = A.seq_offs[(u64)v.x + 1];
      if (b < a || b > A.useqs_bytes) return false;
      at = a;
      bases = b - a;
      return true;
    };
    u64 atL, lenL, atR = 0, lenR = 0;
    bool revL, revR = false;
    const bool okL = unitig(p, atL, lenL, revL);
    len = lenL;
    src = atL | ((u64)revL << 63);
    gap = (p + 1 < c.P && scaffold_of(A, c.S, p + 1) == s) ? 1u : 0u;
    if (gap) {
      const bool okR = unitig(p + 1, atR, lenR, revR);
      G = placement_offset(A.sc_layout, p + 1) - placement_offset(A.sc_layout, p) - lenL;
      // byte i of the last k of L and of the first k of R, as placed, as ranks (0: not ACGT)
      auto rank_l = [&](u32 i) {
        const u32 r = base_rank(A.useqs[revL ? atL + (k - 1u - i) : atL + lenL - k + i]);
        return revL ? comp_rank(r) : r;
      };
      auto rank_r = [&](u32 i) {
        const u32 r = base_rank(A.useqs[revR ? atR + lenR - 1u - i : atR + i]);
        return revR ? comp_rank(r) : r;
      };
      if (!okL || !okR) {
        cls = SIGAX_GAP_MALFORMED;
      } else if (lenL < k || lenR < k) {
        cls = SIGAX_GAP_SHORT;
      } else {
        bool acgt = true;
        for (u32 i = 0; i < k; ++i) acgt = acgt && rank_l(i) != 0u && rank_r(i) != 0u;
        if (!acgt) {
          cls = SIGAX_GAP_NON_ACGT;
        } else if (G > (u64)A.max_fill) {
          cls = SIGAX_GAP_FAR;
        } else {
          cls = GAP_WALK;
          need = (u32)G + A.slack;  // below 2^32: both are below 2^31
          u64* w = A.win + p * 16;
          window_write(w, k, rank_l);
          window_write(w + 4, k, rank_r);
          window_write(w + 8, k, [&](u32 i) { return comp_rank(rank_r(k - 1u - i)); });
          window_write(w + 12, k, [&](u32 i) { return comp_rank(rank_l(k - 1u - i)); });
        }
      }
    }
  }
  A.sof[p] = s;
  A.isgap[p] = gap;
  A.need[p] = need;
  A.fillc[p] = 0u;
  A.remc[p] = 0u;
  A.gres[p] = make_uint2(cls | (SIGAX_GAP_NOT_RUN << 8) | (SIGAX_GAP_NOT_RUN << 16), 0u);
  A.gap_g[p] = G;
  A.plen[p] = len;
  A.psrc[p] = src;
}

// ---- the walks --------------------------------------------------------------------------------------------------------------------
struct Win4 {
  u64 a, b, c, d;  // bases 0-31, 32-63, 64-95, 96-127
};
__device__ __forceinline__ bool same(const Win4& x, const Win4& y) { return x.a == y.a && x.b == y.b && x.c == y.c && x.d == y.d; }
__device__ __forceinline__ Win4 win_load(const u64* p) {
  const ulonglong2 lo = reinterpret_cast<const ulonglong2*>(p)[0], hi = reinterpret_cast<const ulonglong2*>(p)[1];
  Win4 w = {lo.x, lo.y, hi.x, hi.y};
  return w;
}
// w[1:] + b for a window of k bases (k wave-uniform)
__device__ __forceinline__ Win4 win_shift(const Win4& w, u32 k, u32 b) {
  Win4 x = {(w.a >> 2) | (w.b << 62), (w.b >> 2) | (w.c << 62), (w.c >> 2) | (w.d << 62), w.d >> 2};
  const u32 word = (k - 1u) >> 5;
  const u64 v = (u64)b << (2u * ((k - 1u) & 31u));
  if (word == 0u) x.a |= v;
  else if (word == 1u) x.b |= v;
  else if (word == 2u) x.c |= v;
  else x.d |= v;
  return x;
}
__device__ __forceinline__ u32 win_code(const Win4& w, u32 i) { return (u32)(sel4<u64>(i >> 5, w.a, w.b, w.c, w.d) >> (2u * (i & 31u))) & 3u; }

template <bool WIDE>
__global__ __launch_bounds__(256) void k_gap_walk(GapfillArgs A) {
  typedef typename PosOf<WIDE>::type P;
  __shared__ SearchSh<WIDE> sh;
  const FmStrand& S = A.fwd;
  const bool have2 = have_two_step<WIDE>(S);
  search_sh_fill(sh, S);
  __syncthreads();

  const u32 lane = threadIdx.x & 63u, role = lane & 7u, lead = lane & ~7u;
  const u32 mine = role & 3u;      // the base this lane tries
  const bool rcv = role >= 4u;     // ... as the candidate's reverse complement
  const u32 k = A.k;
  const u64 n = A.max_unitigs;

  ChainGrab grab;
  // a group's gap: the same in its eight lanes
  bool active = false;
  u32 phase = 0, fwd_out = SIGAX_GAP_NOT_RUN, need = 0;
  u64 gp = 0, t = 0, limit = 0, G = 0, scr = 0;
  Win4 w = {0, 0, 0, 0}, dst = {0, 0, 0, 0};
  u64 n_steps = 0;
  u32 n_sec = 0;

  // the gap is done: its result, by the group's first lane
  auto finish = [&](u32 cls, u32 fo, u32 ro, u32 dir, u32 fill) {
    if (role == 0u) {
      A.gres[gp] = make_uint2(cls | (fo << 8) | (ro << 16) | (dir << 24), fill);
      if (cls == SIGAX_GAP_FILLED) {
        A.fillc[gp] = fill;
        A.remc[gp] = (u32)G;
      }
    }
    active = false;
  };

  for (;;) {
    // ---- groups without a gap take the wave's next numbers ----
    for (;;) {
      bool got;
      u64 chain;
      if (!grab_chains(grab, &A.cnt[GAP_CHAIN], n, !active && role == 0u, got, chain)) break;
      got = __shfl((int)got, (int)lead, 64) != 0;
      chain = shfl64(chain, lead);
      if (got && chain < n && (A.gres[chain].x & 0xFFu) == GAP_WALK) {
        gp = chain;
        G = A.gap_g[gp];
        need = A.need[gp];
        scr = A.soff[gp];
        if (scr + (u64)need > A.max_walk_bases) {
          finish(SIGAX_GAP_NO_ROOM, SIGAX_GAP_NOT_RUN, SIGAX_GAP_NOT_RUN, 0u, 0u);
        } else {
          active = true;
          phase = 0;
          t = 0;
          limit = (u64)k + G + A.slack;
          w = win_load(A.win + gp * 16);
          dst = win_load(A.win + gp * 16 + 4);
        }
      }
    }
    if (__ballot(active) == 0ull) break;

    // ---- one extension of every walk of the wave: this lane's chain over the k symbols of its candidate ----
    const Win4 x = win_shift(w, k, mine);
    // symbol j of the chain: the candidate from its end (as it stands), its complement from its start (reverse complement)
    auto sym = [&](u32 j) {
      const u32 code = win_code(x, rcv ? j : k - 1u - j);
      return rcv ? 4u - code : code + 1u;
    };
    P lo = 0, hi = 0;
    search_init(sh, sym(0), lo, hi);
    for (u32 j = 1; j < k;) {  // k and have2 are the wave's: every lane takes the same steps
      const bool two = have2 && k - j >= 2u;
      if (active && interval_valid(lo, hi)) search_step<WIDE>(S, sh, sym(j), two ? sym(j + 1u) : 0u, lo, hi, n_sec);
      j += two ? 2u : 1u;
    }
    const u64 occ = active && interval_valid(lo, hi) ? (u64)(hi - lo) + 1ull : 0ull;
    const u64 both = occ + __shfl_xor(occ, 4, 64);  // count(w[1:] + mine), in lanes `mine` and `mine + 4`
    const u32 cand = (u32)(__ballot(active && both >= (u64)A.min_count) >> lead) & 0xFu;

    if (active) {
      ++t;
      if (role == 0u) ++n_steps;
      u32 out = SIGAX_GAP_NOT_RUN, fill = 0;  // NOT_RUN: the walk goes on
      if (cand == 0u) {
        out = SIGAX_GAP_DEAD_END;
      } else if (cand & (cand - 1u)) {
        out = SIGAX_GAP_BRANCH;
      } else {
        const u32 b = (u32)__builtin_ctz(cand);
        const u64 at = scr + (t - 1u);
        if (role == 0u && t <= (u64)need && at < A.max_walk_bases) A.walk[at] = (unsigned char)((0x54474341u >> (8u * b)) & 0xFFu);  // "ACGT"
        w = win_shift(w, k, b);
        if (same(w, dst)) {
          if (t < (u64)k) {
            out = SIGAX_GAP_OVERLAP;
          } else if (t - k + A.slack < G) {
            out = SIGAX_GAP_OFF_ESTIMATE;
          } else {
            out = SIGAX_GAP_FILLED;
            fill = (u32)(t - k);
          }
        } else if (t >= limit) {
          out = SIGAX_GAP_TOO_LONG;
        }
      }
      if (out != SIGAX_GAP_NOT_RUN) {
        if (phase == 0u) {
          if (out == SIGAX_GAP_DEAD_END || out == SIGAX_GAP_BRANCH || out == SIGAX_GAP_TOO_LONG) {
            fwd_out = out;
            phase = 1;
            t = 0;
            w = win_load(A.win + gp * 16 + 8);
            dst = win_load(A.win + gp * 16 + 12);
          } else {
            finish(out, out, SIGAX_GAP_NOT_RUN, 0u, fill);
          }
        } else {
          const bool filled = out == SIGAX_GAP_FILLED;
          finish(filled ? out : fwd_out, fwd_out, out, filled ? 1u : 0u, fill);
        }
      }
    }
  }

  const u64 t_steps = wave_sum(n_steps), t_sec = wave_sum((u64)n_sec);
  if (lane == 0u) {
    if (t_steps) atomicAdd(&A.cnt[GAP_C_STEPS], t_steps);
    if (t_sec) atomicAdd(&A.cnt[GAP_C_SECTORS], t_sec);
  }
}

// ---- the new tables ---------------------------------------------------------------------------------------------------------------
// D(p): the bases the filled gaps before placement p add (modulo 2^64)
__device__ __forceinline__ u64 shift_before(const GapfillArgs& A, u64 p) { return A.fsum[p] - A.rsum[p]; }

__global__ __launch_bounds__(256) void k_gap_lengths(GapfillArgs A) {
  const u64 s = (u64)blockIdx.x * 256u + threadIdx.x;
  if (s >= A.max_unitigs) return;
  const ScafBounds c = scaffold_bounds(A);
  u64 bases = 0;
  if (s < c.S) {
    u64 h = A.sc_lay_offs[s], e = A.sc_lay_offs[s + 1];
    h = h < c.P ? h : c.P;
    e = e < c.P ? e : c.P;
    if (e > h) bases = placement_offset(A.sc_layout, e - 1) + shift_before(A, e - 1) - shift_before(A, h) + A.plen[e - 1];
  }
  A.lenlo[s] = (u32)bases;
  A.lenhi[s] = (u32)(bases >> 32);
}

__global__ __launch_bounds__(256) void k_gap_place(GapfillArgs A) {
  const u64 p = (u64)blockIdx.x * 256u + threadIdx.x;
  const u64 n = A.max_unitigs;
  const ScafBounds c = scaffold_bounds(A);
  u32 cls = GAP_NONE, dir = 0;
  u64 fill = 0, left = 0;
  if (p <= c.S && p <= n) A.sc_offs[p] = A.slo[p] + (A.shi[p] << 32);
  if (p == 0) A.pdst[c.P] = A.slo[c.S] + (A.shi[c.S] << 32);
  if (p < c.P) {
    const u64 s = A.sof[p];
    u64 h = s < c.S ? A.sc_lay_offs[s] : 0ull;
    h = h < c.P ? h : c.P;
    const uint4 v = reinterpret_cast<const uint4*>(A.sc_layout)[p];
    const u64 off = ((u64)v.z | ((u64)v.w << 32)) + shift_before(A, p) - shift_before(A, h);
    reinterpret_cast<uint4*>(A.sc_layout_out)[p] = make_uint4(v.x, v.y, (u32)off, (u32)(off >> 32));
    A.pdst[p] = A.slo[s] + (A.shi[s] << 32) + off;
    if (A.isgap[p]) {
      const uint2 r = A.gres[p];
      const u64 G = A.gap_g[p], g = A.gnum[p];
      cls = r.x & 0xFFu;
      dir = r.x >> 24;
      if (cls == SIGAX_GAP_FILLED) fill = r.y;
      else left = G;
      if (g < n) {
        const u32 right = reinterpret_cast<const uint4*>(A.sc_layout)[p + 1].x;  // (a gap: p + 1 < P)
        const u64 at = off + A.plen[p];
        uint4* rec = reinterpret_cast<uint4*>(A.gaps + g);
        rec[0] = make_uint4((u32)s, v.x, right, G > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)G);
        rec[1] = make_uint4(r.y, r.x, (u32)at, (u32)(at >> 32));
      }
    }
  }
  // the wave's gaps per class, its fills per direction, its bases
#pragma unroll
  for (u32 k = 0; k <= SIGAX_GAP_MALFORMED; ++k) count_sum(A, k, cls == k ? 1ull : 0ull);
  count_sum(A, GAP_C_GAPS, cls != GAP_NONE ? 1ull : 0ull);
  count_sum(A, GAP_C_FWD, cls == SIGAX_GAP_FILLED && dir == 0u ? 1ull : 0ull);
  count_sum(A, GAP_C_REV, cls == SIGAX_GAP_FILLED && dir != 0u ? 1ull : 0ull);
  count_sum(A, GAP_C_FILL, fill);
  count_sum(A, GAP_C_NLEFT, left);
}

// one wave: lane c < 24 writes status entry c
__global__ __launch_bounds__(64) void k_gap_status(GapfillArgs A) {
  const u32 c = threadIdx.x;
  if (blockIdx.x != 0u || c >= 24u) return;
  const ScafBounds g = scaffold_bounds(A);
  const u64 bases = A.slo[g.S] + (A.shi[g.S] << 32);
  u64 out = 0;
  if (c == 0u) out = A.cnt[GAP_C_GAPS];
  else if (c <= 11u) out = A.cnt[c - 1u];
  else if (c <= 15u) out = A.cnt[GAP_C_FWD + (c - 12u)];
  else if (c == 16u) out = bases;
  else if (c == 17u) out = A.cnt[GAP_C_STEPS];
  else if (c == 18u) out = A.cnt[GAP_C_STEPS] * 8ull;
  else if (c == 19u) out = A.cnt[GAP_C_SECTORS];
  else if (c == 20u) out = bases > A.sseqs_capacity ? 1ull : 0ull;
  else if (c == 21u) out = A.cnt[SIGAX_GAP_NO_ROOM] ? 1ull : 0ull;
  else if (c == 22u) out = g.S;
  A.status[c] = out;
}

// ---- the bases --------------------------------------------------------------------------------------------------------------------
struct GapDesc {
  u64 d0, len, src, next, scr;  // where the unitig begins in the output, its bases, psrc, where the next placement begins, its gap's
  u32 fill, rev;                // walk scratch; the gap's fill (0: N) and whether it is read backwards and complemented
};

__global__ __launch_bounds__(256) void k_gap_bases(GapfillArgs A) {
  const ScafBounds c = scaffold_bounds(A);
  const u64 total = A.slo[c.S] + (A.shi[c.S] << 32);
  const u64 P = c.P;
  const u64 b = ((u64)blockIdx.x * 256u + threadIdx.x) * 16ull;
  if (total > A.sseqs_capacity || P == 0 || b >= total) return;
  const u64* __restrict__ D = A.pdst;
  // the placement of output byte p: the last k with D[k] <= p
  auto find = [&](u64 p) -> u64 { return last_at_most(D, P, p); };
  auto desc = [&](u64 k) -> GapDesc {
    GapDesc d;
    d.d0 = D[k];
    d.len = A.plen[k];
    d.src = A.psrc[k];
    d.next = D[k + 1];
    const uint2 r = A.gres[k];
    const bool filled = A.isgap[k] != 0u && (r.x & 0xFFu) == SIGAX_GAP_FILLED;
    d.fill = filled ? r.y : 0u;
    d.rev = r.x >> 24;
    d.scr = A.soff[k];
    return d;
  };
  // output byte p, which lies in the placement of d or in the gap behind it
  auto fetch = [&](u64 p, const GapDesc& d) -> u32 {
    const u64 rel = p - d.d0;
    if (rel < d.len) {
      const bool rev = (d.src >> 63) != 0ull;
      const u64 s0 = d.src & ~(1ull << 63);
      const u64 at = rev ? s0 + (d.len - 1ull - rel) : s0 + rel;
      if (at >= A.useqs_bytes) return 'N';  // (no consistent input comes here)
      const u32 ch = A.useqs[at];
      return rev ? comp_byte(ch) : ch;
    }
    const u64 grel = rel - d.len;
    if (grel >= (u64)d.fill) return 'N';
    const u64 at = d.rev ? d.scr + ((u64)d.fill - 1ull - grel) : d.scr + grel;
    if (at >= A.max_walk_bases) return 'N';
    const u32 ch = A.walk[at];
    return d.rev ? comp_byte(ch) : ch;
  };
  unsigned char* out = A.sseqs;
  GapDesc d = desc(find(b));
  const u64 end = d.d0 + d.len;
  if (b + 16 <= total && b >= d.d0 && end >= d.d0 && b + 16 <= end) {  // inside one unitig
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
      uint4 x;
      __builtin_memcpy(&x, A.useqs + from, 16);  // (no alignment: the compiler picks the access)
      if (rev) {
        // byte j of the piece = complement of byte 15 - j of the load (written out in each bases kernel: as a shared
        // function it compiles to other code, and these kernels stay as they are)
        const u32 m[4] = {x.w, x.z, x.y, x.x};
        u32 y[4];
#pragma unroll
        for (u32 q = 0; q < 4; ++q) {
          const u32 e = m[q];
          y[q] = comp_byte(e >> 24) | (comp_byte((e >> 16) & 255u) << 8) | (comp_byte((e >> 8) & 255u) << 16) | (comp_byte(e & 255u) << 24);
        }
        v = make_uint4(y[0], y[1], y[2], y[3]);
      } else {
        v = x;
      }
    }
    *reinterpret_cast<uint4*>(out + b) = v;
  } else {  // a piece that meets a gap or a boundary: bytes; a byte beyond the placement at hand finds its own
    const u64 to = b + 16 < total ? b + 16 : total;
    for (u64 p = b; p < to; ++p) {
      if (p < d.d0 || p >= d.next) d = desc(find(p));
      out[p] = (unsigned char)fetch(p, d);
    }
  }
}

}  // namespace

void launch_gapfill_bases(const GapfillArgs& a, hipStream_t st) {
  if (a.max_unitigs == 0 || !a.sseqs || a.sseqs_capacity == 0) return;
  hipLaunchKernelGGL(k_gap_bases, dim3(blocks_of((a.sseqs_capacity + 15) / 16)), dim3(256), 0, st, a);
}

hipError_t launch_gapfill(const GapfillArgs& a, bool wide, int n_cu, hipStream_t st) {
  const u64 n = a.max_unitigs;
  if (n == 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(a.cnt, 0, GAP_WORDS * 8, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_gap_classify, dim3(blocks_of(n)), dim3(256), 0, st, a);
  launch_scan(a.isgap, n, a.partial, a.gnum, a.scan_total, st);
  launch_scan(a.need, n, a.partial, a.soff, a.scan_total, st);
  const unsigned long long want = (n * 8ull + 255) / 256;  // eight lanes a gap
  if (wide) launch_persistent(k_gap_walk<true>, a, want, n_cu, st);
  else launch_persistent(k_gap_walk<false>, a, want, n_cu, st);
  launch_scan(a.fillc, n, a.partial, a.fsum, a.scan_total, st);
  launch_scan(a.remc, n, a.partial, a.rsum, a.scan_total, st);
  hipLaunchKernelGGL(k_gap_lengths, dim3(blocks_of(n)), dim3(256), 0, st, a);
  launch_scan(a.lenlo, n, a.partial, a.slo, a.scan_total, st);
  launch_scan(a.lenhi, n, a.partial, a.shi, a.scan_total, st);
  hipLaunchKernelGGL(k_gap_place, dim3(blocks_of(n + 1)), dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_gap_status, dim3(1), dim3(64), 0, st, a);
  launch_gapfill_bases(a, st);
  return hipGetLastError();
}
