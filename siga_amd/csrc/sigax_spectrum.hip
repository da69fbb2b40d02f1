// siga_amd/csrc/sigax_spectrum.hip -- `siga preqc` on the device (gfx950 / CDNA4): index rows back to text
// (FMIndex::getString, src/fmindex.cpp:292-313) and the k-mer count distribution of a batch of strings
// (KmerDistribution::sample, src/kmerdistr.cpp:7-36).
//
//   k_walk      one lane per requested row: read the BWT symbol at the row out of its granule's bit planes, stop at the first
//               symbol of rank 0, else one LF step with the same granule (Occ(c, row - 1) is in it) -- one gather per symbol.
//               WRITE = false returns the length (and Occ('$', end row - 1), the stretch index: what the .sai table is
//               indexed by); WRITE = true walks once to check the caller's slot against the length and, when they agree,
//               a second time to put the bytes down in text order (the first symbol met is the text's last).
//               A walk is cut after max_len symbols, keeping those nearest the row, and where LF leaves the table (a
//               damaged index): no walk can spin.  One-step granules only, so the bytes do not depend on which of the
//               optional tables exist; plain launch, no lane refill (the walk is 1 / 2k of a spectrum's gathers).
//   k_spectrum  for every string s with len >= k and every j = k .. len - 1: w = s[j - k, j), count = occ(w) + occ(revcomp(w))
//               on the forward index, hist[min(count, n_bins - 1)] += 1.  NOTE j < len: the reference's loop never counts the
//               window that ends at the string's last base, and a string of exactly k bases contributes no window, though
//               its bases still count in L (the sum of the lengths of the strings with len >= k).  Kept as it is.
//               Bytes outside ACGT rank as '$' in w and in its complement, as in sigax_match.hip.
//
// Shape of k_spectrum.  Persistent grid; a wave takes one string at a time from a global counter and its lanes take the
// string's windows 64 at a time, so the lanes of a wave read neighbouring bytes of one string.  A lane runs BOTH chains of
// its window in one loop, a (double) step of each per iteration: the two gathers are independent and in flight together,
// and the window's bin is known in the lane without any per-window array or cross-lane traffic.  Chains start from the
// corrector's table of 13-mer intervals when it is resident, k >= 13 and the 13 symbols are ACGT; two symbols go per pair
// of gathers where the two-step lines exist (the start and the step of sigax_rank.h, as k_match).  Bins below SPEC_LOW
// are counted in LDS (u64, 8 KB per workgroup) and flushed once when the workgroup ends; the rare higher ones go to global
// memory directly.  Bins are ADDED to.
// Integer work only, bound by gather latency; no MFMA.
#include <hip/hip_runtime.h>

#include "sigax_kernels.h"
#include "sigax_rank.h"

namespace {

#define SPEC_LOW 1024u  // bins kept in LDS

// ---- rows to text ---------------------------------------------------------------------------------------------------
// -> symbols walked; *cut: stopped by max_len or by a row outside the table; *stretch: Occ('$', end row - 1), ~0 when cut.
// WRITE: the symbols go down backwards from `end`.
// (k_locate_walk of sigax_locate.hip spells the same step out around its hit record -- it tests p >= S.n at the top of the
// loop, which is this loop's test after the step plus one for the first row: a change to the step or to the cut conditions
// here is a change there)
template <bool WIDE, bool WRITE>
__device__ __forceinline__ u32 walk_row(const FmStrand& S, const u64* C, u64 row, u32 max_len, unsigned char* end, bool* cut,
                                        u64* stretch, u32* n_sec) {
  u64 p = row;
  u32 cnt = 0;
  *cut = false;
  *stretch = ~0ull;
  for (;;) {
    const Gran1 q = gran_load(S, p);
    *n_sec += 1u;
    const u32 j = (u32)p & 127u, bit = j & 31u;
    const uint4 ch = sel4<uint4>(j >> 5, q.k0, q.k1, q.k2, q.k3);
    const u32 code = ((ch.y >> bit) & 1u) | (((ch.z >> bit) & 1u) << 1) | (((ch.w >> bit) & 1u) << 2);
    if (code == 0u) {
      *stretch = gran_rank<WIDE>(S, q, p, 0u);
      break;
    }
    if (code > 4u || cnt == max_len) {  // (no such code in a table the decoder wrote)
      *cut = true;
      break;
    }
    if (WRITE) *--end = (unsigned char)((0x5447434124ull >> (8u * code)) & 0xFFu);  // "$ACGT"
    ++cnt;
    p = C[code] + gran_rank<WIDE>(S, q, p, code);
    if (p >= S.n) {
      *cut = true;
      break;
    }
  }
  return cnt;
}

template <bool WIDE, bool WRITE>
__global__ __launch_bounds__(256) void k_walk(WalkArgs A) {
  __shared__ u64 C[5];
  if (threadIdx.x < 5) C[threadIdx.x] = A.s.C[threadIdx.x];
  __syncthreads();
  const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
  u64 n_range = 0, n_cut = 0, n_slot = 0;
  if (i < A.n) {
    const u64 row = A.rows[i];
    bool cut = false;
    u64 stretch = ~0ull;
    u32 len = 0, n_sec = 0;
    if (row >= A.s.n) n_range = 1;
    else len = walk_row<WIDE, false>(A.s, C, row, A.max_len, nullptr, &cut, &stretch, &n_sec);
    n_cut = cut ? 1 : 0;
    if (!WRITE) {
      A.lens[i] = len;
      if (A.stretch) A.stretch[i] = stretch;
    } else {
      const u64 b0 = A.offs[i], b1 = A.offs[i + 1];
      if (b1 < b0 || b1 - b0 != (u64)len) n_slot = 1;
      else if (len != 0) (void)walk_row<WIDE, true>(A.s, C, row, A.max_len, A.out + b1, &cut, &stretch, &n_sec);
    }
  }
  n_range = wave_sum(n_range);
  n_cut = wave_sum(n_cut);
  n_slot = wave_sum(n_slot);
  if ((threadIdx.x & 63u) == 0) {
    if (n_range) atomicAdd(&A.status[0], n_range);
    if (n_cut) atomicAdd(&A.status[1], n_cut);
    if (WRITE && n_slot) atomicAdd(&A.status[2], n_slot);
  }
}

// ---- k-mer spectrum -------------------------------------------------------------------------------------------------
template <bool WIDE>
struct SpecSh {
  SearchSh<WIDE> s;
  u64 low[SPEC_LOW];
};

// symbol i, in the order its chain consumes them, of the window w[0, k): the window backwards as it is read, forwards and
// complemented for its reverse complement
template <bool RC>
__device__ __forceinline__ u32 win_rank(const unsigned char* w, u32 k, u32 i) {
  const u32 r = base_rank(RC ? w[i] : w[k - 1u - i]);
  return RC ? comp_rank(r) : r;
}

template <bool WIDE>
struct SpecChain {
  typename PosOf<WIDE>::type lo, hi;
  u32 i;  // symbols consumed
  __device__ __forceinline__ bool valid() const { return interval_valid(lo, hi); }
  __device__ __forceinline__ bool live(u32 k) const { return i < k && valid(); }
  __device__ __forceinline__ u64 count() const { return valid() ? (u64)(hi - lo) + 1ull : 0ull; }
};

template <bool WIDE, bool RC>
__device__ __forceinline__ void chain_start(const SpectrumArgs& A, const SearchSh<WIDE>& sh, const unsigned char* w, SpecChain<WIDE>& c,
                                            u32* n_sec) {
  auto sym = [&](u32 i) { return win_rank<RC>(w, A.k, i); };
  if (A.ptab != nullptr && A.k >= A.pk && ptab_start<WIDE>(A.ptab, A.pk, sym, c.lo, c.hi)) {
    *n_sec += 1u;
    c.i = A.pk;
  } else {
    search_init(sh, sym(0), c.lo, c.hi);
    c.i = 1;
  }
}

// one step of a live chain: two symbols off a pair of two-step lines where they exist and both are ACGT, else one symbol
// off one-step granules (as k_match)
template <bool WIDE, bool RC>
__device__ __forceinline__ void chain_step(const SpectrumArgs& A, const SearchSh<WIDE>& sh, bool have2, const unsigned char* w,
                                           SpecChain<WIDE>& c, u32* n_sec) {
  const u32 r = win_rank<RC>(w, A.k, c.i);
  u32 e = 0;
  if (have2 && A.k - c.i >= 2u && r != 0u) e = win_rank<RC>(w, A.k, c.i + 1u);
  c.i += search_step<WIDE>(A.fwd, sh, r, e, c.lo, c.hi, *n_sec);
}

template <bool WIDE>
__global__ __launch_bounds__(256) void k_spectrum(SpectrumArgs A) {
  __shared__ SpecSh<WIDE> sh;
  const FmStrand& S = A.fwd;
  const bool have2 = have_two_step<WIDE>(S);
  search_sh_fill(sh.s, S);
  for (u32 b = threadIdx.x; b < SPEC_LOW; b += 256) sh.low[b] = 0;
  __syncthreads();

  const u32 lane = threadIdx.x & 63u;
  const u64 top = A.n_bins - 1ull;
  u64 n_str = 0, n_len = 0, n_win = 0;
  u32 n_sec = 0;
  for (;;) {
    u64 s = 0;
    if (lane == 0) s = atomicAdd(A.counter, 1ull);
    s = first_lane64(s);
    if (s >= A.n_reads) break;
    const u64 b0 = A.offs[s], b1 = A.offs[s + 1];
    if (b1 < b0 || b1 - b0 < (u64)A.k) continue;
    const u64 len = b1 - b0, nwin = len - A.k;
    if (lane == 0) {
      n_str += 1;
      n_len += len;
    }
    for (u64 x = lane; x < nwin; x += 64) {
      const unsigned char* w = A.seqs + b0 + x;
      SpecChain<WIDE> f, r;
      chain_start<WIDE, false>(A, sh.s, w, f, &n_sec);
      chain_start<WIDE, true>(A, sh.s, w, r, &n_sec);
      for (;;) {
        const bool lf = f.live(A.k), lr = r.live(A.k);
        if (!lf && !lr) break;
        if (lf) chain_step<WIDE, false>(A, sh.s, have2, w, f, &n_sec);
        if (lr) chain_step<WIDE, true>(A, sh.s, have2, w, r, &n_sec);
      }
      const u64 cnt = f.count() + r.count();
      const u64 bin = cnt < top ? cnt : top;
      if (bin < SPEC_LOW) atomicAdd(&sh.low[bin], 1ull);
      else atomicAdd(&A.hist[bin], 1ull);
      n_win += 1;
    }
  }
  __syncthreads();
  for (u32 b = threadIdx.x; b < SPEC_LOW && b < A.n_bins; b += 256) {
    const u64 v = sh.low[b];
    if (v) atomicAdd(&A.hist[b], v);
  }
  const u64 t_str = wave_sum(n_str), t_len = wave_sum(n_len), t_win = wave_sum(n_win), t_sec = wave_sum((u64)n_sec);
  if (lane == 0) {
    if (t_str) atomicAdd(&A.dstat[0], t_str);
    if (t_len) atomicAdd(&A.dstat[1], t_len);
    if (t_win) atomicAdd(&A.dstat[2], t_win);
    if (t_sec) atomicAdd(&A.dstat[3], t_sec);
  }
}

}  // namespace

void launch_walk(const WalkArgs& a, bool wide, hipStream_t st) {
  if (a.n == 0) return;
  const dim3 grid((unsigned)((a.n + 255) / 256)), block(256);
  const bool write = a.out != nullptr;
  if (wide) {
    if (write) hipLaunchKernelGGL((k_walk<true, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_walk<true, false>), grid, block, 0, st, a);
  } else {
    if (write) hipLaunchKernelGGL((k_walk<false, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((k_walk<false, false>), grid, block, 0, st, a);
  }
}

void launch_spectrum(const SpectrumArgs& a, bool wide, int n_cu, hipStream_t st) {
  if (a.n_reads == 0) return;
  // persistent grid: as many workgroups as the device holds at once, no more than one wave per string
  const unsigned long long want = (a.n_reads + 3) / 4;
  if (wide) launch_persistent(k_spectrum<true>, a, want, n_cu, st);
  else launch_persistent(k_spectrum<false>, a, want, n_cu, st);
}
