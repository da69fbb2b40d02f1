// siga_amd/csrc/sigax_pileup.hip -- `siga correct -a overlap` on the device (gfx950 / CDNA4, wave64): a read is lined up
// against the indexed reads that share a seed with it, and every column is put to the vote (rules: include/sigax.h).  No
// counterpart in the reference, whose OverlapCorrector::process is empty (src/correct_processor.cpp:231-240).
//
//   k_pile                   the pile-up: one wave per read
//   k_pile_status            the eight status words from the round's counters
//
// The reference text, the seed kernels and the pieces k_pile shares with k_mmo (the table of candidate keys: cand_collect,
// cand_slot, cand_decode, cand_code; seed_span, seed_flags) are sigax_seeded.h's and sigax_seeded.hip's.
//
// Shape of k_pile.  A workgroup is one wave and owns, in dynamic LDS, per column of the read one u64 of four u16 vote counters
// and one byte of the read's code, and a table of candidate keys.  (1) The read's hits are taken 64 at a time, one per lane: a
// hit becomes the key {read, diagonal, strand} and goes into the open-addressed table with a 64-bit compare-and-swap, which is
// what makes the triples distinct; the lanes that did insert are counted, and more than K ends the read.  (2) The table is
// swept 64 slots at a time; the lanes load the text offsets of their own slot's read, so the 64 loads are in flight together,
// and then every occupied slot is taken by the whole wave in turn: lane l faces column x0 + 64 c + l, so a candidate's bases
// are read as 64 neighbouring bytes per step, backwards for the reverse strand.  The candidate's codes stay in two u64 per lane
// (2 bits a column, 64 steps = SIGAX_PILE_MAX_LEN columns), the mismatches are summed over the wave, and an accepted candidate
// is voted from those registers: it is read once.  A lane owns its columns, so the votes are plain LDS read-modify-writes.
// (3) Lanes across columns again: the change rule, the depth rule, the output.  Integer work only, bound by the latency of
// one candidate's text after the other; several waves per SIMD hide it.
#include <hip/hip_runtime.h>

#include "sigax_rank.h"
#include "sigax_pileup.h"

namespace {

__global__ __launch_bounds__(64) void k_pile(PileArgs A) {
  extern __shared__ __align__(16) unsigned char pile_lds[];
  u64* cnt = reinterpret_cast<u64*>(pile_lds);               // [len_cap]: votes of a column, A C G T in 16 bits each
  u64* tab = cnt + A.len_cap;                                // [tab_cap]: candidate keys
  unsigned char* qs = reinterpret_cast<unsigned char*>(tab + A.tab_cap);  // [len_cap]: the read's codes, 4 = outside ACGT

  const u32 lane = threadIdx.x;
  const u64 r = blockIdx.x;
  const u64 total_hits = A.L.loc_status[0];
  if (total_hits > A.L.hits_cap) return;  // the caller's hits did not fit: nothing is written (sigax.h)

  const u32 S = A.p.seed_length, T = A.p.seed_stride;
  const u64 b0 = A.offs[r], n64 = A.offs[r + 1] - b0;
  const unsigned char* q = A.seqs + b0;
  unsigned char* out = A.out_seqs + b0;

  // ---- rule 1 ----
  if (n64 < S || n64 > A.p.max_read_len) {
    for (u64 x = lane; x < n64; x += 64) out[x] = q[x];
    if (lane == 0) {
      A.valid[r] = n64 < S ? 0 : 2;
      A.changed[r] = 0;
      if (n64 >= S) atomicAdd(&A.counters[PILE_C_LONG], 1ull);
    }
    return;
  }
  const u32 n = (u32)n64;  // <= max_read_len <= len_cap

  for (u32 x = lane; x < n; x += 64) {
    cnt[x] = 0;
    const u32 rk = base_rank(q[x]);
    qs[x] = (unsigned char)(rk ? rk - 1u : 4u);
  }
  for (u32 s = lane; s < A.tab_cap; s += 64) tab[s] = CAND_EMPTY;
  __syncthreads();

  // ---- rules 2-3: the seeds' flags, and the hits into the table of distinct triples ----
  const SeedSpan sp = seed_span(A.L, r, total_hits);
  u32 located, repeats;
  seed_flags(A.L, sp, lane, located, repeats);
  const bool over = cand_collect(tab, A.tab_cap, A.L, sp, A.R, n, S, T, A.p.max_candidates, lane);
  wave_add(&A.counters[PILE_C_LOCATED], (u64)located);
  wave_add(&A.counters[PILE_C_REPEATS], (u64)repeats);
  if (over) {
    for (u32 x = lane; x < n; x += 64) out[x] = q[x];
    if (lane == 0) {
      A.valid[r] = 0;
      A.changed[r] = 0;
      atomicAdd(&A.counters[PILE_C_OVER], 1ull);
    }
    return;
  }
  __syncthreads();

  // ---- rules 4-5: every candidate once, lanes across columns ----
  u32 tested = 0, taken = 0;
  for (u32 base = 0; base < A.tab_cap; base += 64) {
    u64 key, rb;
    u32 len_t;
    u64 mask = __ballot(cand_slot(tab, base + lane, A.R, key, rb, len_t, [](u64) {}));
    while (mask) {
      const int src = __ffsll((long long)mask) - 1;
      mask &= mask - 1ull;
      const SeedCand k = cand_decode(key, rb, len_t, src, n);
      const bool rev = k.rev;
      const long long d = k.d, x0 = k.x0, x1 = k.x1, clen = k.clen;
      if (x1 <= x0) continue;  // (a hit's window lies in both texts: there is an overlap)
      const u32 ell = (u32)(x1 - x0), steps = (ell + 63u) >> 6;  // <= 64: ell <= n <= 4096
      const unsigned char* text = A.R.ref_text + k.rb;
      u64 held0 = 0, held1 = 0;
      u32 mism = 0;
      for (u32 c = 0; c < steps; ++c) {
        const long long x = x0 + (long long)(c * 64u + lane);
        if (x < x1) {
          const long long pos = x + d;  // in [0, clen)
          const u32 code = cand_code(text, clen, pos, rev);
          mism += code != (u32)qs[x] ? 1u : 0u;
          if (c < 32u) held0 |= (u64)code << (2u * c);
          else held1 |= (u64)code << (2u * (c - 32u));
        }
      }
      const u32 m = (u32)wave_sum((u64)mism);
      tested += 1u;
      if (ell >= A.p.min_overlap && (u64)m <= ((u64)ell * A.p.error_permille) / 1000ull) {
        taken += 1u;
        for (u32 c = 0; c < steps; ++c) {
          const long long x = x0 + (long long)(c * 64u + lane);
          if (x < x1) {
            const u32 code = (u32)((c < 32u ? held0 >> (2u * c) : held1 >> (2u * (c - 32u))) & 3ull);
            cnt[x] += 1ull << (16u * code);
          }
        }
      }
    }
  }
  __syncthreads();

  // ---- rules 6-7: lanes across columns ----
  const u32 C = A.p.conflict, D = A.p.min_depth;
  bool ok = true;
  u32 n_chg = 0;
  for (u32 x = lane; x < n; x += 64) {
    const u64 c = cnt[x];
    const u32 b = qs[x];
    u32 top = 0, which = 0, n_top = 0;
    for (u32 e = 0; e < 4u; ++e) {
      const u32 v = (u32)(c >> (16u * e)) & 0xFFFFu;
      if (v > top) {
        top = v;
        which = e;
        n_top = 1;
      } else if (v == top) {
        n_top += 1u;
      }
    }
    const u32 cb = b < 4u ? (u32)(c >> (16u * b)) & 0xFFFFu : 0u;
    u32 nb = b;
    if (n_top == 1u && which != b && top >= C && cb < C) nb = which;
    const u32 depth = nb < 4u ? (u32)(c >> (16u * nb)) & 0xFFFFu : 0u;
    ok = ok && depth >= D;
    n_chg += nb != b ? 1u : 0u;
    qs[x] = (unsigned char)(b | (nb << 4));
  }
  const bool valid = __ballot(!ok) == 0ull;
  const u64 t_chg = wave_sum((u64)n_chg);
  for (u32 x = lane; x < n; x += 64) {
    const u32 v = qs[x], b = v & 15u, nb = v >> 4;
    out[x] = (valid && nb != b) ? (unsigned char)((0x54474341u >> (8u * nb)) & 0xFFu) : q[x];  // "ACGT"
  }
  if (lane == 0) {
    A.valid[r] = valid ? 1 : 0;
    A.changed[r] = (valid && t_chg) ? 1 : 0;
    if (tested) atomicAdd(&A.counters[PILE_C_TESTED], (u64)tested);
    if (taken) atomicAdd(&A.counters[PILE_C_ACCEPTED], (u64)taken);
    if (valid && t_chg) atomicAdd(&A.counters[PILE_C_CHANGED], t_chg);
  }
}

__global__ void k_pile_status(PileArgs A) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const u64 hits = A.L.loc_status[0];
  const bool fits = hits <= A.L.hits_cap;
  A.status[0] = hits;
  A.status[1] = fits ? A.counters[PILE_C_LONG] : 0ull;
  A.status[2] = fits ? A.counters[PILE_C_OVER] : 0ull;
  A.status[3] = fits ? A.counters[PILE_C_LOCATED] : 0ull;
  A.status[4] = fits ? A.counters[PILE_C_REPEATS] : 0ull;
  A.status[5] = fits ? A.counters[PILE_C_TESTED] : 0ull;
  A.status[6] = fits ? A.counters[PILE_C_ACCEPTED] : 0ull;
  A.status[7] = fits ? A.counters[PILE_C_CHANGED] : 0ull;
}

}  // namespace

uint32_t pile_lds_bytes(uint32_t len_cap, uint32_t tab_cap) { return len_cap * 8u + tab_cap * 8u + len_cap; }

int launch_pile(const PileArgs& a, hipStream_t st) { return launch_wave_lds(k_pile, a, a.n_reads, pile_lds_bytes(a.len_cap, a.tab_cap), st); }

void launch_pile_status(const PileArgs& a, hipStream_t st) { hipLaunchKernelGGL(k_pile_status, dim3(1), dim3(64), 0, st, a); }
