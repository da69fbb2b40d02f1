// siga_amd/csrc/sigax_locate.hip -- `siga locate` on the device (gfx950 / CDNA4): where every query occurs in the indexed
// reads -- read, offset, strand.  The other half of the FM-index beside counting (sigax_match.hip); no counterpart in the
// reference.
//
//   k_locate_search  whole-pattern backward search on the forward strand for the two CHAINS of a query, {as given, reverse
//                    complement}, as k_match runs them; a chain that ends with rows left writes {lower row, width} instead
//                    of adding its width to a count
//   k_locate_finish  one lane per query: total = the two widths, the per-query flags (a byte outside ACGT, more than max_hits)
//                    and cnt = the hits that are listed; launch_scan turns cnt into hit_offs
//   k_locate_walk    one LF walk per listed row p: the steps from p back to the first symbol of rank 0 are the occurrence's
//                    offset in its read, Occ('$') before that row indexes the .sai table, whose entry is the read
//
// Shape of the search: k_match's.  Chains die at very different depths, so lanes are not tied to chains: persistent grid, a
// wave reserves GRAB chain numbers at a time from one global counter, a lane whose chain ended takes the wave's next one
// in the same loop iteration.  The pattern's bytes are read in place.  Two symbols per pair of gathers where the two-step
// lines exist, one-step granules otherwise, a start from the corrector's table of 13-mer intervals when it is resident and
// the chain has that many ACGT symbols: the intervals are the same whichever tables exist.  The step, the start, the
// constants and the reservation are sigax_rank.h's, the ones k_match and k_spectrum run.
//
// Shape of the walk.  One lane per hit slot, plain launch: the lane finds its (query, strand, row) by binary search in
// hit_offs, walks one 64-byte granule gather per LF step (one-step granules only, the step of k_walk) and writes its record
// with one 16-byte store.  A hit's offset is uniform over its read, so the walks of a wave differ in length as much as walks
// can; a persistent grid whose lanes take the next slot when their walk ends was built and measured against this launch and
// was the slower of the two, so the simpler one stayed.  Integer work only, bound by gather throughput; no
// MFMA, no LDS beyond C[].
#include <hip/hip_runtime.h>

#include "sigax_kernels.h"
#include "sigax_rank.h"

static_assert(sizeof(sigax_hit) == 16, "sigax_hit must be 16 bytes");

namespace {

template <bool WIDE>
__global__ __launch_bounds__(256) void k_locate_search(LocateArgs A) {
  typedef typename PosOf<WIDE>::type P;
  __shared__ SearchSh<WIDE> sh;
  const FmStrand& S = A.fwd;
  const bool have2 = have_two_step<WIDE>(S);
  search_sh_fill(sh, S);
  __syncthreads();

  const u32 nvar = A.rc ? 2u : 1u;  // chains per query: chain = query * nvar + strand
  const u64 n_chains = A.n_queries * nvar;

  ChainGrab grab;
  // a lane's chain: pattern w[0, len), i symbols consumed
  bool active = false, rcv = false;
  const unsigned char* w = nullptr;
  u32 len = 0, i = 0;
  u64 out = 0;
  P lo = 0, hi = 0;
  u32 n_sec = 0;

  auto valid = [&]() { return interval_valid(lo, hi); };
  // symbol j in the order the chain consumes them: the pattern backwards as given, forwards and complemented for its
  // reverse complement
  auto sym = [&](u32 j) {
    const u32 r = base_rank(rcv ? w[j] : w[len - 1u - j]);
    return rcv ? comp_rank(r) : r;
  };

  for (;;) {
    // ---- lanes without a chain take the wave's next chain numbers ----
    for (;;) {
      bool got;
      u64 chain;
      if (!grab_chains(grab, &A.counters[0], n_chains, !active, got, chain)) break;
      if (got) {
        const u64 q = chain / nvar;
        const u64 b0 = A.offs[q], b1 = A.offs[q + 1];
        if (b1 > b0) {  // an empty pattern has no occurrence (Interval::occurrences of "")
          active = true;
          rcv = (chain - q * nvar) != 0u;
          out = 2 * q + (rcv ? 1u : 0u);
          w = A.seqs + b0;
          len = (u32)(b1 - b0);
          if (A.ptab != nullptr && len >= A.pk && ptab_start<WIDE>(A.ptab, A.pk, sym, lo, hi)) {
            n_sec += 1u;
            i = A.pk;
          } else {
            search_init(sh, sym(0), lo, hi);
            i = 1;
          }
        }
      }
    }
    if (__ballot(active) == 0ull) break;

    // ---- one step of every live chain: two symbols off a pair of two-step lines where they exist and both are ACGT,
    //      else one symbol off one-step granules (as k_match) ----
    if (active && i < len && valid()) {
      const u32 r = sym(i);
      u32 e = 0;
      if (have2 && len - i >= 2u && r != 0u) e = sym(i + 1u);
      i += search_step<WIDE>(S, sh, r, e, lo, hi, n_sec);
    }
    // ---- a chain that is done leaves its interval, in the iteration of its last step; the lane is free ----
    if (active && (i >= len || !valid())) {
      if (valid()) A.chains[out] = make_ulonglong2((u64)lo, (u64)(hi - lo) + 1ull);
      active = false;
    }
  }

  const u64 t_sec = wave_sum((u64)n_sec);
  if ((threadIdx.x & 63u) == 0 && t_sec) atomicAdd(&A.status[2], t_sec);
}

__global__ __launch_bounds__(256) void k_locate_finish(LocateArgs A) {
  const u64 q = (u64)blockIdx.x * 256 + threadIdx.x;
  if (q >= A.n_queries) return;
  const u64 b0 = A.offs[q], b1 = A.offs[q + 1];
  bool acgt = b1 > b0;
  for (u64 j = b0; j < b1; ++j) acgt = acgt && base_rank(A.seqs[j]) != 0u;
  const ulonglong2 f = A.chains[2 * q], r = A.chains[2 * q + 1];
  const u64 total = f.y + r.y;
  const u32 flags = (acgt ? 0u : SIGAX_LOCATE_SKIPPED) | (total > (u64)A.max_hits ? SIGAX_LOCATE_OVER : 0u);
  A.totals[q] = total;
  A.qflags[q] = flags;
  A.cnt[q] = flags ? 0u : (u32)total;
}

template <bool WIDE>
__global__ __launch_bounds__(256) void k_locate_walk(LocateArgs A) {
  __shared__ u64 C[5];
  const FmStrand& S = A.fwd;
  if (threadIdx.x < 5) C[threadIdx.x] = S.C[threadIdx.x];
  __syncthreads();
  const u64 total = A.hit_offs[A.n_queries];
  const u64 slot = (u64)blockIdx.x * 256 + threadIdx.x;
  u32 n_sec = 0, n_cut = 0;
  // total > hits_cap: the caller's buffers are too small, nothing is written (sigax.h)
  if (total <= A.hits_cap && slot < total) {
    // the query whose hits hold this slot: hit_offs[lo_q] <= slot < hit_offs[hi_q] throughout (hit_offs[n] = total > slot)
    u64 lo_q = 0, hi_q = A.n_queries;
    while (hi_q - lo_q > 1ull) {
      const u64 m = (lo_q + hi_q) >> 1;
      if (A.hit_offs[m] <= slot) lo_q = m;
      else hi_q = m;
    }
    const u64 j = slot - A.hit_offs[lo_q];
    const ulonglong2 f = A.chains[2 * lo_q];
    const bool rev = j >= f.y;
    const u64 row = rev ? A.chains[2 * lo_q + 1].x + (j - f.y) : f.x + j;
    // the LF walk from the row to the first symbol of rank 0, one granule gather per step: the step and the cut conditions of
    // walk_row in sigax_spectrum.hip, kept in step with it by hand (k_walk's code generation stays what it was)
    u64 p = row, stretch = 0;
    u32 steps = 0;
    bool cut = false;
    for (;;) {
      if (p >= S.n) {  // LF left the table
        cut = true;
        break;
      }
      const Gran1 g = gran_load(S, p);
      n_sec += 1u;
      const u32 b = (u32)p & 127u, bit = b & 31u;
      const uint4 ch = sel4<uint4>(b >> 5, g.k0, g.k1, g.k2, g.k3);
      const u32 code = ((ch.y >> bit) & 1u) | (((ch.z >> bit) & 1u) << 1) | (((ch.w >> bit) & 1u) << 2);
      if (code == 0u) {
        stretch = gran_rank<WIDE>(S, g, p, 0u);
        break;
      }
      if (code > 4u || steps == A.max_len) {  // (no such code in a table the decoder wrote)
        cut = true;
        break;
      }
      ++steps;
      p = C[code] + gran_rank<WIDE>(S, g, p, code);
    }
    if (!cut && stretch >= A.n_sai) cut = true;
    const u32 fl = rev ? SIGAX_HIT_REV : 0u;
    uint4 rec;
    if (!cut) rec = make_uint4((u32)lo_q, A.sai[stretch], steps, fl);
    else rec = make_uint4((u32)lo_q, 0xFFFFFFFFu, 0xFFFFFFFFu, fl | SIGAX_HIT_CUT);
    reinterpret_cast<uint4*>(A.hits)[slot] = rec;  // one 16-byte store
    if (A.rows) A.rows[slot] = row;
    n_cut = cut ? 1u : 0u;
  }
  const u64 t_sec = wave_sum((u64)n_sec), t_cut = wave_sum((u64)n_cut);
  if ((threadIdx.x & 63u) == 0) {
    if (t_cut) atomicAdd(&A.status[1], t_cut);
    if (t_sec) atomicAdd(&A.status[2], t_sec);
  }
}

}  // namespace

void launch_locate_search(const LocateArgs& a, bool wide, int n_cu, hipStream_t st) {
  if (a.n_queries == 0) return;
  // persistent grid: as many workgroups as the device holds at once, no more than the chains can keep busy
  const unsigned long long want = (a.n_queries * 2ull + 255) / 256;
  if (wide) launch_persistent(k_locate_search<true>, a, want, n_cu, st);
  else launch_persistent(k_locate_search<false>, a, want, n_cu, st);
}

void launch_locate_finish(const LocateArgs& a, hipStream_t st) {
  if (a.n_queries == 0) return;
  hipLaunchKernelGGL(k_locate_finish, dim3((unsigned)((a.n_queries + 255) / 256)), dim3(256), 0, st, a);
}

unsigned long long locate_walk_slots(unsigned long long n_queries, uint32_t max_hits, unsigned long long hits_cap) {
  // n_queries < 2^32 (a hit names its query in 32 bits) and max_hits < 2^32: the product does not wrap
  const unsigned long long most = n_queries * (unsigned long long)max_hits;
  return hits_cap < most ? hits_cap : most;
}

void launch_locate_walk(const LocateArgs& a, bool wide, hipStream_t st) {
  // the hits are not known on the host here, but they are no more than hits_cap when anything is walked, and never more
  // than n_queries * max_hits (a caller may pass UINT64_MAX for "room enough"): one lane per such slot, lanes beyond the
  // hits listed leave at once.  The caller has checked the slots against LOCATE_MAX_SLOTS.
  const unsigned long long slots = locate_walk_slots(a.n_queries, a.max_hits, a.hits_cap);
  if (slots == 0) return;
  const dim3 grid((unsigned)(slots / 256 + (slots % 256 ? 1 : 0))), block(256);
  if (wide) hipLaunchKernelGGL(k_locate_walk<true>, grid, block, 0, st, a);
  else hipLaunchKernelGGL(k_locate_walk<false>, grid, block, 0, st, a);
}
