// siga_amd/csrc/sigax_join.hip -- `siga unitig --scaffold --join-overlaps` on the device (gfx950 / CDNA4, wave64): scaffold
// neighbours that overlap written as one sequence.  The rules are in include/sigax.h and DESIGN.md 9l; the restatement the tests
// hold this against is tests/join_cases.py::expected_join.
//
//   k_join_classify  one lane per placement: its scaffold (one bisection), where its bases lie in the input sseqs, whether it and
//                    the next placement are a gap, G, and the classes that need no match (the fill test reads the gap's bytes)
//   launch_scan      the gaps' numbers; the numbers of the gaps that come to the match
//   k_join_list      the placements of those gaps, in order
//   k_join_match     a wave per open gap, taken in strides of the grid.  It packs L's last hi and R's first hi bases into 2-bit
//                    codes in LDS, 32 bases a word (2 KB at the limit), and the run of ACGT at L's end and R's start bounds the
//                    candidates, so no validity bit is kept.  Lane i tests v = lo + i, lo + i + 64, ...: R's head word by word
//                    against L's tail funnel-shifted into place, leaving at the first word that differs.  The lanes' counts
//                    summed give |M|, the largest matching v the one v: neither depends on lane order.  <true> (`--join-mismatches`)
//                    goes on where |M| = 0: over the words still in LDS, v up to hi' = min(hi, |L| / 2, |R| / 2), the differing
//                    bases counted word by word (popcount of the XOR folded to one bit a base) until they pass B(v); the lane
//                    that owns the one v writes its columns
//   k_join_choose    a wave per gap with one approximate v: lanes 0-31 are column i x {J^L, J^R} as the window stands, lanes
//                    32-63 the reverse complements; the column takes R's base iff count over J^R > count over J^L
//   k_join_support   a wave per gap with one v and windows across its junction: 32 windows a turn, lanes 0-31 the windows as they
//                    stand, lanes 32-63 their reverse complements, one backward search of k symbols a lane (search_step,
//                    sigax_rank.h), forward strand only.  <.., true>: an approximate v has every window that touches the overlap,
//                    over J* (L's bases but for the columns that took R's)
//   launch_scan      G + v of the joined gaps, summed over the placements before each one
//   k_join_lengths   one lane per scaffold: its new bases; launch_scan gives sc_offs'
//   k_join_place     one lane per placement: its new offset, the stretch of the output it governs, the gap's record, the counters
//   k_join_status    status16
//   k_join_bases     one lane per 16-byte piece of the output: the piece's stretch by bisection, then 16 bytes of the input from a
//                    source that is in general not aligned, or bytes where the piece meets a junction or the end
//   k_join_patch     one lane per (gap, column): R's base where an approximately joined gap's column took it
// Every loop has a bound the host knows and every access is bounds-checked.  Plain vector stores and atomics only.
#include <hip/hip_runtime.h>

#include "sigax_device.h"
#include "sigax_kernels.h"
#include "sigax_rank.h"

namespace {

// (the tables' bounds, scaffold_of, placement_offset and the wave reductions are sigax_device.h's)
// this wave's sum of v, added once to counter c
__device__ __forceinline__ void count_sum(const JoinArgs& A, u32 c, u64 v) { wave_add(&A.cnt[c], v); }
// the first placement of scaffold s, and the one behind its last: sc_lay_offs taken as P when above it
__device__ __forceinline__ u64 head_of(const JoinArgs& A, const ScafBounds& c, u64 s) {
  const u64 h = A.sc_lay_offs[s];
  return h < c.P ? h : c.P;
}

__global__ __launch_bounds__(256) void k_join_classify(JoinArgs A) {
  const u64 p = (u64)blockIdx.x * 256u + threadIdx.x;
  if (p >= A.max_unitigs) return;
  const ScafBounds c = scaffold_bounds(A);
  u32 cls = JOIN_NO_GAP, gap = 0, open = 0, s = 0, hi = 0;
  u64 len = 0, src = 0, G = 0;
  if (p < c.P) {
    s = (u32)scaffold_of(A, c.S, p);
    const u64 base = A.sc_offs_in[s], top = A.sc_offs_in[(u64)s + 1];
    const bool sc_ok = top >= base && top <= A.sseqs_bytes;
    const u64 sc_len = top - base;
    // a placement of scaffold s: where its bases lie in the input and how many they are; a bad one has none
    auto placed = [&](u64 q, u64& at, u64& bases) {
      const uint4 v = reinterpret_cast<const uint4*>(A.sc_layout)[q];
      at = bases = 0;
      if ((u64)v.x >= c.nu || !sc_ok) return false;
      const u64 a = A.seq_offs[v.x], b = A.seq_offs[(u64)v.x + 1];
      const u64 off = (u64)v.z | ((u64)v.w << 32);
      if (b < a || off > sc_len || b - a > sc_len - off) return false;
      at = base + off;
      bases = b - a;
      return true;
    };
    u64 atL, lenL, atR = 0, lenR = 0;
    const bool okL = placed(p, atL, lenL);
    len = lenL;
    src = atL;
    gap = (p + 1 < c.P && scaffold_of(A, c.S, p + 1) == s) ? 1u : 0u;
    if (gap) {
      const bool okR = placed(p + 1, atR, lenR);
      G = placement_offset(A.sc_layout, p + 1) - placement_offset(A.sc_layout, p) - lenL;
      if (!okL || !okR) {
        cls = SIGAX_JOIN_MALFORMED;
      } else if (G == 0) {
        cls = SIGAX_JOIN_CLOSED;
      } else if (G > (u64)A.slack) {
        cls = SIGAX_JOIN_FAR;
      } else {
        // the gap's bytes lie between two good placements of one scaffold: inside the input (the test is never false)
        bool all_n = true;
        for (u64 i = 0; i < G && all_n; ++i) {
          const u64 at = atL + lenL + i;
          all_n = at < A.sseqs_bytes && A.sseqs_in[at] == (unsigned char)'N';
        }
        u64 h = A.max_overlap;
        h = lenL == 0 || lenR == 0 ? 0ull : h;
        h = lenL && lenL - 1 < h ? lenL - 1 : h;
        h = lenR && lenR - 1 < h ? lenR - 1 : h;
        hi = (u32)h;
        if (!all_n) {
          cls = SIGAX_JOIN_CLOSED;
        } else if (hi < A.min_overlap) {
          cls = SIGAX_JOIN_SHORT;
        } else {
          cls = JOIN_OPEN;
          open = 1;
        }
      }
    }
  }
  A.sof[p] = s;
  A.isgap[p] = gap;
  A.open[p] = open;
  A.rem[p] = 0u;
  if (A.ainfo) A.ainfo[p] = 0u;
  A.gres[p] = make_uint4(cls, 0u, G > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)G, hi);
  A.plen[p] = len;
  A.psrc[p] = src;
}

__global__ __launch_bounds__(256) void k_join_list(JoinArgs A) {
  const u64 p = (u64)blockIdx.x * 256u + threadIdx.x;
  if (p >= A.max_unitigs || !A.open[p]) return;
  const u64 at = A.onum[p];
  if (at < A.max_unitigs) A.list[at] = (u32)p;
}

// ---- the match --------------------------------------------------------------------------------------------------------------------
enum { JOIN_MAX_WORDS = 128 };  // 4096 bases, 32 a word

// L's tail from base `from` on against R's head, word w of v bases: the XOR of the 2-bit codes, bits beyond base v cleared
__device__ __forceinline__ u64 match_word(const u64* T, const u64* H, u32 from, u32 v, u32 w) {
  const u32 fw = from >> 5, sh = 2u * (from & 31u);
  const u64 a = T[fw + w], b = T[fw + w + 1u];
  u64 x = ((a >> sh) | (sh ? b << (64u - sh) : 0ull)) ^ H[w];
  const u32 left = v - 32u * w;
  if (left < 32u) x &= (1ull << (2u * left)) - 1ull;
  return x;
}
// one bit a base (the low bit of its code's place) where the two codes differ
__device__ __forceinline__ u64 differing(u64 x) { return (x | (x >> 1)) & 0x5555555555555555ull; }

// One wave a workgroup, so that the workgroup's barrier is the wave's: T and H are written by some lanes and read by others.
template <bool APPROX>
__global__ __launch_bounds__(64) void k_join_match(JoinArgs A) {
  __shared__ u64 T[JOIN_MAX_WORDS + 2], H[JOIN_MAX_WORDS + 2];  // L's last hi bases and R's first hi, base j at bits 2 (j & 31) of word j >> 5
  const u32 lane = threadIdx.x;
  const u64 n = A.max_unitigs;
  u64 n_open = A.onum[n];
  n_open = n_open < n ? n_open : n;
  u64 t_cand = 0, a_cand = 0;
  for (u64 g = blockIdx.x; g < n_open; g += gridDim.x) {
    const u64 p = A.list[g];
    if (p + 1 >= n) continue;  // (a listed placement has one behind it)
    const uint4 r = A.gres[p];
    u32 hi = r.w;
    hi = hi > 32u * JOIN_MAX_WORDS ? 32u * JOIN_MAX_WORDS : hi;  // (max_overlap <= 4096)
    const u32 lo = A.min_overlap;
    if ((r.x & 0xFFu) != JOIN_OPEN || hi < lo) continue;
    const u64 tail = A.psrc[p] + A.plen[p] - hi, head = A.psrc[p + 1];
    const u32 words = (hi + 31u) >> 5;
    // pack, two words a lane at the most; the ACGT run at L's end and at R's start
    u32 bad_t = 0, bad_h = hi;  // one past the last base of the tail that is not ACGT; the first such base of the head
    for (u32 w = lane; w <= words; w += 64u) {
      u64 tw = 0, hw = 0;
      for (u32 j = 32u * w; j < 32u * w + 32u && j < hi; ++j) {
        const u64 ta = tail + j, ha = head + j;
        const u32 rt = ta < A.sseqs_bytes ? base_rank(A.sseqs_in[ta]) : 0u, rh = ha < A.sseqs_bytes ? base_rank(A.sseqs_in[ha]) : 0u;
        if (rt == 0u) bad_t = j + 1u;
        if (rh == 0u && j < bad_h) bad_h = j;
        tw |= (u64)((rt - 1u) & 3u) << (2u * (j & 31u));
        hw |= (u64)((rh - 1u) & 3u) << (2u * (j & 31u));
      }
      T[w] = tw;  // word `words` is zero: the funnel shift reads one word beyond the last base
      H[w] = hw;
    }
    bad_t = wave_max32(bad_t);
    bad_h = wave_min32(bad_h);
    const u32 run = hi - bad_t < bad_h ? hi - bad_t : bad_h;  // no v above it matches
    __syncthreads();
    u32 mine = 0, best = 0;
    for (u32 v = lo + lane; v <= hi && v <= run; v += 64u) {
      const u32 from = hi - v, fw = from >> 5, sh = 2u * (from & 31u), vw = (v + 31u) >> 5;
      bool same = true;
      for (u32 w = 0; w < vw && same; ++w) {
        const u64 a = T[fw + w], b = T[fw + w + 1u];
        u64 x = ((a >> sh) | (sh ? b << (64u - sh) : 0ull)) ^ H[w];
        const u32 left = v - 32u * w;
        if (left < 32u) x &= (1ull << (2u * left)) - 1ull;
        same = x == 0ull;
      }
      if (same) {
        ++mine;
        best = v;
      }
    }
    const u32 m = (u32)wave_sum((u64)mine);
    best = wave_max32(best);
    // the second match: no exact v (m is the wave's, so the whole wave comes here or none of it)
    u32 m1 = 0, v1 = 0, d1 = 0;
    if (APPROX && m == 0u) {
      u64 half = A.plen[p] >> 1;
      half = (A.plen[p + 1] >> 1) < half ? A.plen[p + 1] >> 1 : half;
      const u32 hi2 = (u64)hi < half ? hi : (u32)half;  // hi'
      u32 mine2 = 0, best2 = 0, dist2 = 0;
      for (u32 v = lo + lane; v <= hi2 && v <= run; v += 64u) {
        u64 bud = (u64)v * A.mismatch_permille / 1000ull;
        bud = bud < (u64)A.max_mismatches ? bud : (u64)A.max_mismatches;
        const u32 budget = (u32)bud, vw = (v + 31u) >> 5;
        u32 d = 0;
        for (u32 w = 0; w < vw && d <= budget; ++w) d += (u32)__popcll(differing(match_word(T, H, hi - v, v, w)));
        if (d <= budget) {
          ++mine2;
          best2 = v;
          dist2 = d;
        }
      }
      m1 = (u32)wave_sum((u64)mine2);
      v1 = wave_max32(best2);
      d1 = wave_max32(mine2 ? dist2 : 0u);  // (read only when m1 == 1: the one lane's)
      if (m1 == 1u && mine2 == 1u) {  // the one lane that owns the one v: its columns, ascending (d1 <= 16 of them)
        const u32 vw = (v1 + 31u) >> 5;
        u32 c = 0;
        for (u32 w = 0; w < vw; ++w) {
          u64 x = differing(match_word(T, H, hi - v1, v1, w));
          for (u32 b = 0; b < 32u && x; ++b) {
            const u32 j = 32u * w + (((u32)__ffsll((unsigned long long)x) - 1u) >> 1);
            if (c < (u32)JOIN_MAX_COLUMNS) A.cols[p * JOIN_MAX_COLUMNS + c] = (uint16_t)j;
            ++c;
            x &= x - 1ull;
          }
        }
      }
      a_cand += hi2 >= lo ? (u64)(hi2 - lo) + 1ull : 0ull;
    }
    __syncthreads();  // T and H are packed again for the wave's next gap
    t_cand += (u64)(hi - lo) + 1ull;
    if (lane == 0u) {
      const u32 matches = m > 255u ? 255u : m;
      if (APPROX && m == 0u && m1 >= 1u) {
        if (m1 >= 2u) {
          A.gres[p] = make_uint4(SIGAX_JOIN_AMBIGUOUS | ((m1 > 255u ? 255u : m1) << 8), 0u, r.z, r.w);
        } else {
          // every window of J that touches the overlap or crosses the junction: starts |L| - v - k + 1 .. |L| - 1, clipped to 0 .. |J| - k
          const u64 lenL = A.plen[p], lenJ = lenL + A.plen[p + 1] - v1, k = A.k;
          A.ainfo[p] = d1 | (1u << 16);
          if (lenJ < k) {
            A.gres[p] = make_uint4(SIGAX_JOIN_UNSUPPORTED | (1u << 8), v1, r.z, r.w);
          } else {
            const u64 first = lenL + 1ull > (u64)v1 + k ? lenL + 1ull - v1 - k : 0ull;
            const u64 last = lenL - 1ull < lenJ - k ? lenL - 1ull : lenJ - k;  // (>= first: |R| >= 1)
            A.gres[p] = make_uint4(JOIN_APPROX | (1u << 8) | ((u32)(last - first + 1ull) << 16), v1, r.z, r.w);
          }
        }
      } else if (m == 0u) {
        A.gres[p] = make_uint4(SIGAX_JOIN_NONE, 0u, r.z, r.w);
      } else if (m >= 2u) {
        A.gres[p] = make_uint4(SIGAX_JOIN_AMBIGUOUS | (matches << 8), 0u, r.z, r.w);
      } else {
        // the windows across the junction of J = L ++ R[v:], |J| = |L| + |R| - v: starts |L| - k + 1 .. |L| - v - 1, clipped to 0 .. |J| - k
        const u64 lenL = A.plen[p], lenJ = lenL + A.plen[p + 1] - best, k = A.k;
        u64 win = 0;
        if ((u64)best + 1ull < k && lenJ >= k) {
          const u64 first = lenL + 1ull > k ? lenL + 1ull - k : 0ull;
          u64 last = lenL - best - 1ull;  // (|L| > v)
          last = last < lenJ - k ? last : lenJ - k;
          win = last >= first ? last - first + 1ull : 0ull;
        }
        if (win == 0) {
          A.gres[p] = make_uint4(SIGAX_JOIN_JOINED | (1u << 8), best, r.z, r.w);
          A.rem[p] = r.z + best;  // (G <= slack < 2^31)
        } else {
          A.gres[p] = make_uint4(JOIN_UNIQUE | (1u << 8) | ((u32)win << 16), best, r.z, r.w);
        }
      }
    }
  }
  if (lane == 0u && t_cand) atomicAdd(&A.cnt[JOIN_C_CAND], t_cand);
  if (APPROX && lane == 0u && a_cand) atomicAdd(&A.acnt[JOIN_A_CAND], a_cand);
}

// ---- the choice and the support test --------------------------------------------------------------------------------------------------
// count(window) of the k bytes that rank(at), rank(at + 1) .. give, for the lane pair (slot, slot + 32): lanes below 32 search the
// window as it stands, the others its reverse complement.  k and have2 are the wave's: every lane takes the same steps
template <bool WIDE, class Rank>
__device__ __forceinline__ u64 window_count(const FmStrand& S, const SearchSh<WIDE>& sh, bool have2, u32 k, bool active, bool rcv, u64 at, Rank rank,
                                            u32& n_sec) {
  typedef typename PosOf<WIDE>::type P;
  // symbol j of the chain: the window from its end (as it stands), its complement from its start (reverse complement)
  auto sym = [&](u32 j) {
    const u32 rk = rank(at + (rcv ? j : k - 1u - j));
    return rcv ? comp_rank(rk) : rk;
  };
  bool acgt = active;
  for (u32 j = 0; j < k && acgt; ++j) acgt = rank(at + j) != 0u;
  P lo = 0, hi = 0;
  if (acgt) search_init(sh, sym(0), lo, hi);
  for (u32 j = 1; j < k;) {
    const bool two = have2 && k - j >= 2u;
    if (acgt && interval_valid(lo, hi)) search_step<WIDE>(S, sh, sym(j), two ? sym(j + 1u) : 0u, lo, hi, n_sec);
    j += two ? 2u : 1u;
  }
  const u64 occ = acgt && interval_valid(lo, hi) ? (u64)(hi - lo) + 1ull : 0ull;
  return occ + __shfl_xor(occ, 32, 64);
}

// `win` windows from `first` on, 32 a turn: whether one of them has count < min_count
template <bool WIDE, class Rank>
__device__ __forceinline__ bool windows_fail(const JoinArgs& A, const SearchSh<WIDE>& sh, bool have2, u64 first, u32 win, Rank rank, u32& n_sec) {
  const u32 lane = threadIdx.x, slot = lane & 31u;
  bool failed = false;
  for (u32 w0 = 0; w0 < win; w0 += 32u) {  // at most four turns for an exact v, (v + k - 1 + 31) / 32 <= 132 for an approximate one
    const bool active = w0 + slot < win;
    const u64 both = window_count<WIDE>(A.fwd, sh, have2, A.k, active, lane >= 32u, first + w0 + slot, rank, n_sec);
    failed = failed || __ballot(active && both < (u64)A.min_count) != 0ull;
  }
  return failed;
}

template <bool WIDE>
__global__ __launch_bounds__(64) void k_join_choose(JoinArgs A) {
  __shared__ SearchSh<WIDE> sh;
  const FmStrand& S = A.fwd;
  const bool have2 = have_two_step<WIDE>(S);
  search_sh_fill(sh, S);
  __syncthreads();
  const u32 lane = threadIdx.x, col = (lane & 31u) >> 1;
  const bool right = (lane & 1u) != 0u;  // the window over J^R
  const u32 k = A.k;
  const u64 n = A.max_unitigs;
  u64 n_open = A.onum[n];
  n_open = n_open < n ? n_open : n;
  u32 n_sec = 0;
  u64 looked = 0;
  for (u64 g = blockIdx.x; g < n_open; g += gridDim.x) {
    const u64 p = A.list[g];
    if (p + 1 >= n) continue;
    const uint4 r = A.gres[p];
    if ((r.x & 0xFFu) != JOIN_APPROX) continue;
    const u32 v = r.y, info = A.ainfo[p];
    u32 m = info & 0xFFu;
    m = m < (u32)JOIN_MAX_COLUMNS ? m : (u32)JOIN_MAX_COLUMNS;
    const u64 lenL = A.plen[p], srcL = A.psrc[p], srcR = A.psrc[p + 1];
    const u64 lenJ = lenL + A.plen[p + 1] - v, cut = lenL - v;  // (the match: |J| >= k, v < |L|)
    const bool active = col < m;
    const u64 x = cut + (active ? (u64)A.cols[p * JOIN_MAX_COLUMNS + col] : 0ull);
    u64 at = (x > (u64)(k / 2u) ? x : (u64)(k / 2u)) - (u64)(k / 2u);
    at = at < lenJ - k ? at : lenJ - k;
    // byte y of J^L = L ++ R[v:] or of J^R = L[:|L| - v] ++ R as a rank (0: not ACGT)
    auto rank_j = [&](u64 y) {
      const u64 from = right ? (y < cut ? srcL + y : srcR + (y - cut)) : (y < lenL ? srcL + y : srcR + v + (y - lenL));
      return from < A.sseqs_bytes ? base_rank(A.sseqs_in[from]) : 0u;
    };
    const u64 mine = window_count<WIDE>(S, sh, have2, k, active, lane >= 32u, at, rank_j, n_sec);
    const u64 other = __shfl_xor(mine, 1, 64);  // J^R's count in the lanes of J^L
    const u64 took = __ballot(active && !right && lane < 32u && other > mine);  // bit 2 i: column i takes R's base
    u32 mask = 0;
    for (u32 i = 0; i < (u32)JOIN_MAX_COLUMNS; ++i) mask |= (u32)((took >> (2u * i)) & 1ull) << i;
    if (lane == 0u) {
      A.amask[p] = mask;
      A.ainfo[p] = info | ((u32)__popc(mask) << 8);
    }
    looked += 2ull * m;
  }
  if (lane == 0u && looked) atomicAdd(&A.acnt[JOIN_A_CHOICE], looked);
}

template <bool WIDE, bool APPROX>
__global__ __launch_bounds__(64) void k_join_support(JoinArgs A) {
  __shared__ SearchSh<WIDE> sh;
  const FmStrand& S = A.fwd;
  const bool have2 = have_two_step<WIDE>(S);
  search_sh_fill(sh, S);
  __syncthreads();
  const u32 lane = threadIdx.x;
  const u32 k = A.k;
  const u64 n = A.max_unitigs;
  u64 n_open = A.onum[n];
  n_open = n_open < n ? n_open : n;
  u32 n_sec = 0;
  for (u64 g = blockIdx.x; g < n_open; g += gridDim.x) {
    const u64 p = A.list[g];
    if (p + 1 >= n) continue;
    const uint4 r = A.gres[p];
    const u32 cls = r.x & 0xFFu;
    const bool approx = APPROX && cls == JOIN_APPROX;
    if (cls != JOIN_UNIQUE && !approx) continue;
    const u32 v = r.y, win = r.x >> 16;  // win <= k - 2, or <= v + k - 1 for an approximate v
    const u64 lenL = A.plen[p], srcL = A.psrc[p], srcR = A.psrc[p + 1];
    // byte x of J as a rank (0: not ACGT): L, then R from its base v on
    auto rank_j = [&](u64 x) {
      const u64 at = x < lenL ? srcL + x : srcR + v + (x - lenL);
      return at < A.sseqs_bytes ? base_rank(A.sseqs_in[at]) : 0u;
    };
    bool failed;
    if (approx) {
      const u32 mask = A.amask[p];
      u32 m = A.ainfo[p] & 0xFFu;
      m = m < (u32)JOIN_MAX_COLUMNS ? m : (u32)JOIN_MAX_COLUMNS;
      const u64 cut = lenL - v;
      // byte x of J*: J, but R's base at the columns that took it.  Only at a column do the two copies of the overlap differ
      auto rank_star = [&](u64 x) {
        u32 rk = rank_j(x);
        if (mask && x >= cut && x < lenL) {
          const u64 j = x - cut, at = srcR + j;
          const u32 rr = at < A.sseqs_bytes ? base_rank(A.sseqs_in[at]) : 0u;
          if (rr != rk)
            for (u32 i = 0; i < m; ++i)
              if ((mask >> i & 1u) && (u64)A.cols[p * JOIN_MAX_COLUMNS + i] == j) rk = rr;
        }
        return rk;
      };
      const u64 first = lenL + 1ull > (u64)v + k ? lenL + 1ull - v - k : 0ull;
      failed = windows_fail<WIDE>(A, sh, have2, first, win, rank_star, n_sec);
    } else {
      const u64 first = lenL + 1ull > (u64)k ? lenL + 1ull - k : 0ull;
      failed = windows_fail<WIDE>(A, sh, have2, first, win, rank_j, n_sec);
    }
    if (lane == 0u) {
      A.gres[p] = make_uint4((failed ? SIGAX_JOIN_UNSUPPORTED : SIGAX_JOIN_JOINED) | (r.x & 0xFFFFFF00u), v, r.z, r.w);
      if (!failed) A.rem[p] = r.z + v;
    }
  }
}

// ---- the new tables ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_join_lengths(JoinArgs A) {
  const u64 s = (u64)blockIdx.x * 256u + threadIdx.x;
  if (s >= A.max_unitigs) return;
  const ScafBounds c = scaffold_bounds(A);
  u64 bases = 0;
  if (s < c.S) {
    const u64 h = head_of(A, c, s), e = head_of(A, c, s + 1);
    bases = A.sc_offs_in[s + 1] - A.sc_offs_in[s];
    if (e > h) bases -= A.esum[e] - A.esum[h];
  }
  A.lenlo[s] = (u32)bases;
  A.lenhi[s] = (u32)(bases >> 32);
}

__global__ __launch_bounds__(256) void k_join_place(JoinArgs A) {
  const u64 p = (u64)blockIdx.x * 256u + threadIdx.x;
  const u64 n = A.max_unitigs;
  const ScafBounds c = scaffold_bounds(A);
  u32 cls = JOIN_NO_GAP;
  u64 ov = 0, gone = 0, win = 0, acols = 0, aright = 0, ajoined = 0;
  if (p <= c.S && p <= n) A.sc_offs[p] = A.slo[p] + (A.shi[p] << 32);
  if (p == 0) A.pkey[c.P] = A.slo[c.S] + (A.shi[c.S] << 32);
  if (p < c.P) {
    const u64 s = A.sof[p];
    const u64 h = s < c.S ? head_of(A, c, s) : 0ull;
    const u64 shift = A.esum[p] - A.esum[h];
    const uint4 v = reinterpret_cast<const uint4*>(A.sc_layout)[p];
    const u64 off = ((u64)v.z | ((u64)v.w << 32)) - shift;
    reinterpret_cast<uint4*>(A.sc_layout_out)[p] = make_uint4(v.x, v.y, (u32)off, (u32)(off >> 32));
    // from the first base that placement p alone has -- behind the overlap, where the gap before it is joined -- the output is
    // the input `shift` bytes on
    const u64 base_out = A.slo[s] + (A.shi[s] << 32), base_in = s < c.S ? A.sc_offs_in[s] : 0ull;
    u64 before = 0;
    if (p > 0 && A.isgap[p - 1]) {
      const uint4 q = A.gres[p - 1];
      if ((q.x & 0xFFu) == SIGAX_JOIN_JOINED) before = q.y;
    }
    A.pkey[p] = base_out + off + before;
    A.pshift[p] = base_in + shift - base_out;
    if (A.isgap[p]) {
      const uint4 r = A.gres[p];
      const u64 g = A.gnum[p];
      cls = r.x & 0xFFu;
      const bool tested = cls == SIGAX_JOIN_JOINED || cls == SIGAX_JOIN_UNSUPPORTED;
      win = tested ? r.x >> 16 : 0u;
      if (cls == SIGAX_JOIN_JOINED) {
        ov = r.y;
        gone = r.z;
      }
      if (g < n) {
        const u32 right = reinterpret_cast<const uint4*>(A.sc_layout)[p + 1].x;  // (a gap: p + 1 < P)
        const u64 at = cls == SIGAX_JOIN_JOINED ? off + A.plen[p] - r.y : off + A.plen[p];  // offset'[p + 1] of a joined gap
        uint4* rec = reinterpret_cast<uint4*>(A.joins + g);
        rec[0] = make_uint4((u32)s, v.x, right, r.z);
        rec[1] = make_uint4(tested ? r.y : 0u, cls | (r.x & 0xFF00u) | ((u32)win << 16), (u32)at, (u32)(at >> 32));
        const u32 info = tested && A.ainfo ? A.ainfo[p] : 0u;
        if (A.mm) A.mm[g] = info;
        if (cls == SIGAX_JOIN_JOINED && info) {
          ajoined = 1;
          acols = info & 0xFFu;
          aright = (info >> 8) & 0xFFu;
        }
      }
    }
  }
  // the wave's gaps per class, its bases
#pragma unroll
  for (u32 k = 0; k <= SIGAX_JOIN_MALFORMED; ++k) count_sum(A, k, cls == k ? 1ull : 0ull);
  count_sum(A, JOIN_C_GAPS, cls != JOIN_NO_GAP ? 1ull : 0ull);
  count_sum(A, JOIN_C_OVERLAP, ov);
  count_sum(A, JOIN_C_N, gone);
  count_sum(A, JOIN_C_WINDOWS, win);
  if (A.acnt) {
    const u64 sums[3] = {wave_sum(ajoined), wave_sum(acols), wave_sum(aright)};  // (all three sums before the first add)
    for (u32 k = 0; k < 3u; ++k)
      if (sums[k] && (threadIdx.x & 63u) == 0u) atomicAdd(&A.acnt[JOIN_A_JOINED + k], sums[k]);
  }
}

// one wave: lane c < 16 (24 with `--join-mismatches`) writes status entry c
__global__ __launch_bounds__(64) void k_join_status(JoinArgs A) {
  const u32 c = threadIdx.x;
  if (blockIdx.x != 0u || c >= A.n_status || c >= 24u) return;
  const ScafBounds g = scaffold_bounds(A);
  const u64 bases = A.slo[g.S] + (A.shi[g.S] << 32);
  u64 out = 0;
  if (c == 0u) out = A.cnt[JOIN_C_GAPS];
  else if (c <= 8u) out = A.cnt[c - 1u];
  else if (c == 9u) out = A.cnt[JOIN_C_OVERLAP];
  else if (c == 10u) out = A.cnt[JOIN_C_N];
  else if (c == 11u) out = bases;
  else if (c == 12u) out = A.cnt[JOIN_C_CAND];
  else if (c == 13u) out = A.cnt[JOIN_C_WINDOWS];
  else if (c == 14u) out = bases > A.sseqs_capacity ? 1ull : 0ull;
  else if (c == 15u) out = g.S;
  else out = c < 16u + 5u && A.acnt ? A.acnt[c - 16u] : 0ull;
  A.status[c] = out;
}

// ---- the bases --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_join_bases(JoinArgs A) {
  const ScafBounds c = scaffold_bounds(A);
  const u64 total = A.slo[c.S] + (A.shi[c.S] << 32);
  const u64 P = c.P;
  const u64 b = ((u64)blockIdx.x * 256u + threadIdx.x) * 16ull;
  if (total > A.sseqs_capacity || P == 0 || b >= total) return;
  const u64* __restrict__ D = A.pkey;
  // the stretch of output byte x: the last placement k with D[k] <= x
  auto find = [&](u64 x) -> u64 { return last_at_most(D, P, x); };
  auto fetch = [&](u64 x, u64 shift) -> u32 {
    const u64 at = x + shift;
    return at < A.sseqs_bytes ? A.sseqs_in[at] : (u32)'N';  // (no consistent input comes to the N)
  };
  unsigned char* out = A.sseqs;
  u64 k = find(b);
  u64 shift = A.pshift[k], next = D[k + 1];
  const u64 from = b + shift;
  if (b + 16 <= total && b >= D[k] && b + 16 <= next && from + 16 <= A.sseqs_bytes && from + 16 > from) {  // inside one stretch
    uint4 v;
    __builtin_memcpy(&v, A.sseqs_in + from, 16);  // (no alignment: the compiler picks the access)
    *reinterpret_cast<uint4*>(out + b) = v;
  } else {  // a piece that meets a junction or the end: bytes; a byte beyond the stretch at hand finds its own
    const u64 to = b + 16 < total ? b + 16 : total;
    for (u64 x = b; x < to; ++x) {
      if (x < D[k] || x >= next) {
        k = find(x);
        shift = A.pshift[k];
        next = D[k + 1];
      }
      out[x] = (unsigned char)fetch(x, shift);
    }
  }
}

// ---- the patches ------------------------------------------------------------------------------------------------------------------
// lane (p, i): column i of the gap behind placement p, where that gap is joined approximately and the column took R's base
__global__ __launch_bounds__(256) void k_join_patch(JoinArgs A) {
  const u64 t = (u64)blockIdx.x * 256u + threadIdx.x;
  const u64 p = t / JOIN_MAX_COLUMNS;
  const u32 i = (u32)(t % JOIN_MAX_COLUMNS);
  const ScafBounds c = scaffold_bounds(A);
  const u64 total = A.slo[c.S] + (A.shi[c.S] << 32);
  if (total > A.sseqs_capacity || p + 1 >= c.P || p + 1 >= A.max_unitigs || !A.isgap[p]) return;
  const uint4 r = A.gres[p];
  const u32 info = A.ainfo[p];
  if ((r.x & 0xFFu) != SIGAX_JOIN_JOINED || !(info >> 16) || i >= (info & 0xFFu) || !(A.amask[p] >> i & 1u)) return;
  const u64 s = A.sof[p];
  const u64 j = A.cols[p * JOIN_MAX_COLUMNS + i];
  const u64 to = A.slo[s] + (A.shi[s] << 32) + placement_offset(A.sc_layout_out, p + 1) + j, from = A.psrc[p + 1] + j;
  if (to < total && from < A.sseqs_bytes) A.sseqs[to] = A.sseqs_in[from];
}

// one-wave workgroups for the gaps that come to the match: no more than the device holds at a time, the rest in strides
unsigned gap_waves(u64 n, int n_cu) {
  const u64 cap = (u64)(n_cu > 0 ? n_cu : 256) * 16ull;
  return (unsigned)(n < cap ? n : cap);
}
}  // namespace

void launch_join_bases(const JoinArgs& a, hipStream_t st) {
  if (a.max_unitigs == 0 || !a.sseqs || a.sseqs_capacity == 0) return;
  hipLaunchKernelGGL(k_join_bases, dim3(blocks_of((a.sseqs_capacity + 15) / 16)), dim3(256), 0, st, a);
  if (a.max_mismatches) hipLaunchKernelGGL(k_join_patch, dim3(blocks_of(a.max_unitigs * JOIN_MAX_COLUMNS)), dim3(256), 0, st, a);
}

hipError_t launch_join(const JoinArgs& a, bool wide, int n_cu, hipStream_t st) {
  const u64 n = a.max_unitigs;
  if (n == 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(a.cnt, 0, JOIN_WORDS * 8, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_join_classify, dim3(blocks_of(n)), dim3(256), 0, st, a);
  launch_scan(a.isgap, n, a.partial, a.gnum, a.scan_total, st);
  launch_scan(a.open, n, a.partial, a.onum, a.scan_total, st);
  hipLaunchKernelGGL(k_join_list, dim3(blocks_of(n)), dim3(256), 0, st, a);
  const dim3 waves(gap_waves(n, n_cu));
  if (a.max_mismatches) {  // `--join-mismatches`: the second match, the choice, the wider support test
    e = hipMemsetAsync(a.acnt, 0, JOIN_AWORDS * 8, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_join_match<true>, waves, dim3(64), 0, st, a);
    if (wide) {
      hipLaunchKernelGGL(k_join_choose<true>, waves, dim3(64), 0, st, a);
      hipLaunchKernelGGL((k_join_support<true, true>), waves, dim3(64), 0, st, a);
    } else {
      hipLaunchKernelGGL(k_join_choose<false>, waves, dim3(64), 0, st, a);
      hipLaunchKernelGGL((k_join_support<false, true>), waves, dim3(64), 0, st, a);
    }
  } else {
    hipLaunchKernelGGL(k_join_match<false>, waves, dim3(64), 0, st, a);
    if (wide) hipLaunchKernelGGL((k_join_support<true, false>), waves, dim3(64), 0, st, a);
    else hipLaunchKernelGGL((k_join_support<false, false>), waves, dim3(64), 0, st, a);
  }
  launch_scan(a.rem, n, a.partial, a.esum, a.scan_total, st);
  hipLaunchKernelGGL(k_join_lengths, dim3(blocks_of(n)), dim3(256), 0, st, a);
  launch_scan(a.lenlo, n, a.partial, a.slo, a.scan_total, st);
  launch_scan(a.lenhi, n, a.partial, a.shi, a.scan_total, st);
  hipLaunchKernelGGL(k_join_place, dim3(blocks_of(n + 1)), dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_join_status, dim3(1), dim3(64), 0, st, a);
  launch_join_bases(a, st);
  return hipGetLastError();
}
