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
// chains: the grid is persistent, a wave reserves GRAB chain numbers at a time from one global counter (grab_chains,
// sigax_rank.h), and a lane whose interval emptied or whose pattern ended adds its count and takes the wave's next chain
// number in the same loop iteration -- every lane of a wave has a live chain until the counter runs out.
// The pattern is read in place, through a two-word (16-byte) window per lane that slides in the direction the chain
// consumes: backwards through the read for the pattern as read, FORWARDS for its reverse complement -- backward search
// of revcomp(w) consumes comp(w[0]), comp(w[1]), ... -- so no reversed copy exists anywhere, and no pattern length is too
// long.  The window's next word is asked for when the previous one is entered, eight symbols before it is needed.
// With the two-step table (fm_layout.h) two symbols go per pair of gathers; a pair with a symbol of rank 0, an odd last
// symbol, and indexes without the table take one-step granules.  When the corrector's prefix table is resident a chain of
// at least that many symbols, all of them ACGT, starts from its entry.  Counts are the same whichever tables exist.
// The step, the start from the table and the workgroup's constants are sigax_rank.h's, shared with sigax_spectrum.hip and
// sigax_locate.hip; what is this file's own is how a chain's symbols are fetched.  Integer work only, bound by gather
// latency; no MFMA.
#include <hip/hip_runtime.h>

#include "sigax_kernels.h"
#include "sigax_rank.h"

namespace {

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
  __shared__ SearchSh<WIDE> sh;
  const FmStrand& S = A.fwd;
  const bool have2 = have_two_step<WIDE>(S);
  search_sh_fill(sh, S);
  __syncthreads();

  const u32 nvar = (A.rc ? 2u : 1u) * (A.max_length == ~0ull ? 1u : 2u);  // chains per read: chain = read * nvar + variant
  const u64 n_chains = A.n_reads * nvar;
  const u64 align = (u64)(uintptr_t)A.seqs & 7ull;
  const unsigned char* base = A.seqs - align;
  const u64 buf_lo = align + A.offs[0], buf_hi = align + A.offs[A.n_reads];

  ChainGrab grab;
  // a lane's chain
  bool active = false;
  bool rcv = false;
  u64 pos = 0, seg_lo = 0, seg_hi = 0, out = 0;
  u32 rem = 0;
  P lo = 0, hi = 0;
  Win win = {0, 0, 0};
  u32 n_run = 0, n_sym = 0, n_sec = 0;

  auto valid = [&]() { return interval_valid(lo, hi); };
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
      bool got;
      u64 chain;
      if (!grab_chains(grab, &A.dstat[3], n_chains, !active, got, chain)) break;
      if (got) {
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
            // the attempt slides the window over the pk symbols; they are taken back when one of them is not ACGT
            const Win w_save = win;
            const u64 pos_save = pos;
            const u32 rem_save = rem;
            started = ptab_start<WIDE>(A.ptab, A.pk, [&](u32) {
              const u32 r = rank_at(pos);
              advance(1);
              return r;
            }, lo, hi);
            if (started) {
              n_sec += 1u;
              n_sym += valid() ? A.pk : 1u;
            } else {
              win = w_save;
              pos = pos_save;
              rem = rem_save;
            }
          }
          if (!started) {
            search_init(sh, rank_at(pos), lo, hi);
            n_sym += 1u;
            advance(1);
          }
        }
      }
    }
    if (__ballot(active) == 0ull) break;

    if (active) {
      if (rem == 0 || !valid()) {
        // the chain is done (fmindex.h:80-86): its occurrences go to its read's number; the lane is free
        if (valid()) atomicAdd(&A.counts[out], (u64)(hi - lo) + 1ull);
        active = false;
      } else {
        const u32 r = rank_at(pos);
        u32 e = 0;
        if (have2 && rem >= 2u && r != 0u) e = rank_at(rcv ? pos + 1u : pos - 1u);
        bool first_left;
        const u32 k = search_step<WIDE>(S, sh, r, e, lo, hi, n_sec, &first_left);
        n_sym += first_left ? k : 1u;  // the reference stopped at a symbol that emptied the interval
        advance(k);
      }
    }
  }

  const u64 t_run = wave_sum(n_run), t_sym = wave_sum(n_sym), t_sec = wave_sum(n_sec);
  if ((threadIdx.x & 63u) == 0) {
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
  const unsigned long long want = (a.n_reads * 4ull + 255) / 256;
  if (wide) launch_persistent(k_match<true>, a, want, n_cu, st);
  else launch_persistent(k_match<false>, a, want, n_cu, st);
}
