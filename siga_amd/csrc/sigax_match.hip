// siga_amd/csrc/sigax_match.hip -- `siga match` on the device (gfx950 / CDNA4): how often a read, or its first and last
// --max-length bases, occurs in the indexed set, on both strands (src/match.cpp:38-63, FMIndex::Interval::occurrences,
// src/fmindex.h:67-98).
//
//   k_match_init  counts[2r] = 0, counts[2r+1] = 0 for a read that is split (len > max_length), SIGAX_MATCH_NONE otherwise
//   k_match       whole-pattern backward search on the forward strand for up to four CHAINS per read:
//                 {head, tail} x {as read, reverse complement}; every chain adds its occurrences to its read's count
//
// Shape.  Chains differ in length by orders of magnitude (a read with an error dies a few symbols past the point where its
// suffix becomes unique, a read of the index walks to its end, a contig walks 100 000 symbols), so lanes are not tied to
// chains: the grid is persistent, a wave reserves MATCH_GRAB chain numbers at a time from one global counter, and a lane
// whose interval emptied or whose pattern ended adds its count and takes the wave's next chain number in the same loop
// iteration -- every lane of a wave has a live chain until the counter runs out.
// The pattern is read in place, through a two-word (16-byte) window per lane that slides in the direction the chain
// consumes: backwards through the read for the pattern as read, FORWARDS for its reverse complement -- backward search
// of revcomp(w) consumes comp(w[0]), comp(w[1]), ... -- so no reversed copy exists anywhere, and no pattern length is too
// long.  The window's next word is asked for when the previous one is entered, eight symbols before it is needed.
// With the two-step table (fm_layout.h) two symbols go per pair of gathers; a pair with a symbol of rank 0, an odd last
// symbol, and indexes without the table take one-step granules.  When the corrector's prefix table is resident a chain of
// at least that many symbols, all of them ACGT, starts from its entry.  Counts are the same whichever tables exist.
// Integer work only, bound by gather latency; no MFMA.
#include <hip/hip_runtime.h>

#include "sigax_kernels.h"
#include "sigax_rank.h"

namespace {

#define MATCH_GRAB 64u  // chain numbers a wave reserves at a time: one atomic per 64 chains, and the last waves of a launch
                        // are never more than 64 chains apart

template <bool WIDE>
struct MatchSh {
  typedef typename PosOf<WIDE>::type P;
  u64 C[5], T[5];  // FMIndex::_pred and the symbol totals
  P Cc[4][4];      // Cc[c][e] = Occ(e, C[c]): the constants of a double step
};

// ---- the pattern, read in place -------------------------------------------------------------------------------------
// Positions are VIRTUAL byte offsets: offset in seqs + (address of seqs & 7), so that word w of the window is the aligned
// 8 bytes at base + 8 w (base = seqs rounded down).  A word that does not touch the chain's segment [lo, hi) is never
// loaded; one that sticks out of the batch's bytes [a + offs[0], a + offs[n]) is put together from its bytes inside.
struct Win {
  u64 w0, w1;  // word i0 and the next one in the chain's direction
  u64 i0;
};
__device__ __forceinline__ u64 win_word(const unsigned char* base, u64 wi, u64 seg_lo, u64 seg_hi, u64 buf_lo, u64 buf_hi) {
  if (wi < (seg_lo >> 3) || wi > ((seg_hi - 1u) >> 3)) return 0ull;
  const u64 o = wi << 3;
  if (o >= buf_lo && o + 8u <= buf_hi) return *reinterpret_cast<const u64*>(base + o);
  u64 v = 0;
  for (u32 b = 0; b < 8u; ++b)
    if (o + b >= buf_lo && o + b < buf_hi) v |= (u64)base[o + b] << (8u * b);
  return v;
}
__device__ __forceinline__ u32 win_byte(const Win& w, u64 p) {
  const u64 v = (p >> 3) == w.i0 ? w.w0 : w.w1;
  return (u32)(v >> (((u32)p & 7u) * 8u)) & 0xFFu;
}

__global__ __launch_bounds__(256) void k_match_init(const u64* offs, u64 n_reads, u64 max_length, u64* counts) {
  const u64 r = (u64)blockIdx.x * 256 + threadIdx.x;
  if (r >= n_reads) return;
  const u64 len = offs[r + 1] - offs[r];
  counts[2 * r] = 0;
  counts[2 * r + 1] = len > max_length ? 0ull : SIGAX_MATCH_NONE;
}

template <bool WIDE>
__global__ __launch_bounds__(256) void k_match(MatchArgs A) {
  typedef typename PosOf<WIDE>::type P;
  __shared__ MatchSh<WIDE> sh;
  const FmStrand& S = A.fwd;
  const bool have2 = S.gran2 != nullptr && (!WIDE || S.super2 != nullptr);
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
  __syncthreads();

  const u32 lane = threadIdx.x & 63u;
  const u64 lt = (1ull << lane) - 1ull;
  const u32 nvar = (A.rc ? 2u : 1u) * (A.max_length == ~0ull ? 1u : 2u);  // chains per read: chain = read * nvar + variant
  const u64 n_chains = A.n_reads * nvar;
  const u64 align = (u64)(uintptr_t)A.seqs & 7ull;
  const unsigned char* base = A.seqs - align;
  const u64 buf_lo = align + A.offs[0], buf_hi = align + A.offs[A.n_reads];

  u64 wnext = 0, wend = 0;  // the wave's reserved chain numbers (wave-uniform)
  bool drained = false;     // the global counter has run out
  // a lane's chain
  bool active = false;
  bool rcv = false;
  u64 pos = 0, seg_lo = 0, seg_hi = 0, out = 0;
  u32 rem = 0;
  P lo = 0, hi = 0;
  Win win = {0, 0, 0};
  u32 n_run = 0, n_sym = 0, n_sec = 0;

  auto valid = [&]() { return hi != (P)~(P)0 && hi >= lo; };
  // the chain has consumed k symbols: move on, sliding the window when its first word has been left
  auto advance = [&](u32 k) {
    pos = rcv ? pos + k : pos - k;
    rem -= k;
    if ((pos >> 3) != win.i0) {
      win.w0 = win.w1;
      win.i0 = pos >> 3;
      win.w1 = win_word(base, rcv ? win.i0 + 1u : win.i0 - 1u, seg_lo, seg_hi, buf_lo, buf_hi);
    }
  };
  auto rank_at = [&](u64 p) {
    const u32 r = base_rank(win_byte(win, p));
    return rcv ? comp_rank(r) : r;
  };

  for (;;) {
    // ---- lanes without a chain take the wave's next chain numbers ----
    for (;;) {
      const u64 need = __ballot(!active);
      if (need == 0ull) break;
      if (wnext >= wend) {
        if (drained) break;
        u64 b = 0;
        if (lane == 0) b = atomicAdd(&A.dstat[3], (u64)MATCH_GRAB);
        b = first_lane64(b);
        if (b >= n_chains) {
          drained = true;
          break;
        }
        wnext = b;
        wend = b + MATCH_GRAB < n_chains ? b + MATCH_GRAB : n_chains;
      }
      const u32 avail = (u32)(wend - wnext), wanted = (u32)__popcll(need), mine = (u32)__popcll(need & lt);
      if (!active && mine < avail) {
        const u64 chain = wnext + mine;
        const u64 rd = chain / nvar;
        const u32 var = (u32)(chain - rd * nvar);
        rcv = A.rc && (var & 1u);
        const bool tail = (A.rc ? (var >> 1) : var) != 0u;
        const u64 b0 = A.offs[rd], b1 = A.offs[rd + 1], len = b1 - b0;
        const bool split = len > A.max_length;
        const u64 plen = split ? A.max_length : len;
        // match.cpp:54-62: one number for a read of up to max_length bases, two for a longer one; an empty pattern has no
        // occurrence (Interval::occurrences of "")
        if ((!tail || split) && plen != 0) {
          active = true;
          ++n_run;
          out = 2 * rd + (tail ? 1u : 0u);
          seg_lo = align + (tail ? b1 - plen : b0);
          seg_hi = seg_lo + plen;
          // segments of 2^32 symbols and more are beyond what a batch holds (offs are bytes of one device buffer)
          rem = (u32)plen;
          pos = rcv ? seg_lo : seg_hi - 1u;
          win.i0 = pos >> 3;
          win.w0 = win_word(base, win.i0, seg_lo, seg_hi, buf_lo, buf_hi);
          win.w1 = win_word(base, rcv ? win.i0 + 1u : win.i0 - 1u, seg_lo, seg_hi, buf_lo, buf_hi);
          bool started = false;
          if (A.ptab != nullptr && rem >= A.pk) {
            // the prefix table's entry of the first pk symbols, the first one consumed in the lowest two bits (k_prefix_build)
            const Win w_save = win;
            const u64 pos_save = pos;
            const u32 rem_save = rem;
            u32 code = 0;
            bool acgt = true;
            for (u32 i = 0; i < A.pk; ++i) {
              const u32 r = rank_at(pos);
              acgt = acgt && r != 0u;
              code |= ((r - 1u) & 3u) << (2u * i);
              advance(1);
            }
            if (acgt) {
              u64 cnt;
              if (WIDE) {
                const ulonglong2 e = reinterpret_cast<const ulonglong2*>(A.ptab)[code];
                lo = (P)e.x;
                cnt = e.y;
              } else {
                const uint2 e = reinterpret_cast<const uint2*>(A.ptab)[code];
                lo = (P)e.x;
                cnt = e.y;
              }
              n_sec += 1u;
              hi = lo + (P)cnt - 1;
              if (cnt == 0) {  // the reference stopped somewhere in these symbols, after one at the least
                lo = 1;
                hi = 0;
                n_sym += 1u;
              } else {
                n_sym += A.pk;
              }
              started = true;
            } else {
              win = w_save;
              pos = pos_save;
              rem = rem_save;
            }
          }
          if (!started) {  // Interval::init (src/fmindex.h:90-93)
            const u32 r0 = rank_at(pos);
            lo = (P)sh.C[r0];
            hi = lo + (P)sh.T[r0] - 1;
            n_sym += 1u;
            advance(1);
          }
        }
      }
      wnext += wanted < avail ? wanted : avail;
    }
    if (__ballot(active) == 0ull) break;

    if (active) {
      if (rem == 0 || !valid()) {
        // the chain is done (fmindex.h:80-86): its occurrences go to its read's number; the lane is free
        if (valid()) atomicAdd(&A.counts[out], (u64)(hi - lo) + 1ull);
        active = false;
      } else {
        const u32 r = rank_at(pos);
        const u64 pl = (u64)lo > S.n ? S.n : (u64)lo, pu0 = (u64)hi + 1ull, pu = pu0 > S.n ? S.n : pu0;
        u32 e = 0;
        if (have2 && rem >= 2u && r != 0u) e = rank_at(rcv ? pos + 1u : pos - 1u);
        if (e != 0u) {
          // two symbols from the two positions of the first step (fm_layout.h): Occ(e, C[r] + Occ(r, p)) = Cc[r][e] + R2(e, r, p)
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
          // an interval that symbol r emptied comes out empty after the pair (R2 over no rows); the reference stopped there
          n_sym += U1 > L1 ? 2u : 1u;
          advance(2);
        } else {
          const bool two = (pl >> 7) != (pu >> 7);
          const Gran1 qa = gran_load(S, pl);
          Gran1 qb = qa;
          if (two) qb = gran_load(S, pu);
          n_sec += two ? 2u : 1u;
          const P pb = (P)sh.C[r];
          lo = pb + (P)gran_rank<WIDE>(S, qa, pl, r);       // getOcc(c, lower - 1)
          hi = pb + (P)gran_rank<WIDE>(S, qb, pu, r) - 1;   // getOcc(c, upper)
          n_sym += 1u;
          advance(1);
        }
      }
    }
  }

  const u64 t_run = wave_sum(n_run), t_sym = wave_sum(n_sym), t_sec = wave_sum(n_sec);
  if (lane == 0) {
    atomicAdd(&A.dstat[0], t_run);
    atomicAdd(&A.dstat[1], t_sym);
    atomicAdd(&A.dstat[2], t_sec);
  }
}

}  // namespace

void launch_match(const MatchArgs& a, bool wide, int n_cu, hipStream_t st) {
  if (a.n_reads == 0) return;
  hipLaunchKernelGGL(k_match_init, dim3((unsigned)((a.n_reads + 255) / 256)), dim3(256), 0, st, a.offs, a.n_reads, a.max_length, a.counts);
  // persistent grid: as many workgroups as the device holds at once, no more than the chains can keep busy
  int per_cu = 0;
  const hipError_t e = wide ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_match<true>, 256, 0)
                            : hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_match<false>, 256, 0);
  if (e != hipSuccess || per_cu < 1) {
    (void)hipGetLastError();
    per_cu = 2;
  }
  const unsigned long long chains = a.n_reads * 4ull;
  const unsigned long long want = (chains + 255) / 256, cap = (unsigned long long)(n_cu > 0 ? n_cu : 256) * (unsigned)per_cu;
  const unsigned grid = (unsigned)(want < cap ? want : cap);
  if (wide) hipLaunchKernelGGL(k_match<true>, dim3(grid), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(k_match<false>, dim3(grid), dim3(256), 0, st, a);
}
