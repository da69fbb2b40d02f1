// siga_amd/csrc/sigax_pileup.hip -- `siga correct -a overlap` on the device (gfx950 / CDNA4, wave64): a read is lined up
// against the indexed reads that share a seed with it, and every column is put to the vote (rules: include/sigax.h).  No
// counterpart in the reference, whose OverlapCorrector::process is empty (src/correct_processor.cpp:231-240).
//
//   k_ref_iota, k_ref_order  the reference text by read id, around the row walk of sigax_spectrum.hip: rows 0 .. n_strings - 1
//                            are walked for their lengths and stretches, k_ref_order files row and length under the read id
//                            sai[stretch], the scan gives the offsets and the walk's write pass the bytes
//   k_pile_seed_count        one lane per read: the seeds it has (rule 2), none for a read the kernel does not take
//   k_pile_seed_fill         one lane per seed slot: the seed's bytes and its offset, as the query table of sigax_locate_device
//   k_pile                   the pile-up: one wave per read
//   k_pile_status            the eight status words from the round's counters
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

#include "sigax_pileup.h"
#include "sigax_rank.h"

namespace {

#define PILE_EMPTY (~0ull)
#define PILE_D_BIAS (1ll << 30)  // diagonals are kept as d + 2^30 in 31 bits: reference reads are shorter than 2^30 bases

__global__ __launch_bounds__(256) void k_ref_iota(u64* rows, u64 n) {
  const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
  if (i < n) rows[i] = i;
}

__global__ __launch_bounds__(256) void k_ref_order(RefOrderArgs A) {
  const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
  u32 bad = 0;
  if (i < A.n) {
    const u64 s = A.stretch[i];
    const u32 id = s < A.n ? A.sai[s] : 0xFFFFFFFFu;
    if ((u64)id < A.n) {
      A.rows_by_id[id] = i;
      A.lens_by_id[id] = A.lens[i];
    } else {
      bad = 1;
    }
  }
  wave_add(A.bad, (u64)bad);
}

// rule 2: the windows at 0, T, 2T, ... and the one that ends the read
__device__ __forceinline__ u32 seeds_regular(u32 n, u32 S, u32 T) { return (n - S) / T + 1u; }
__device__ __forceinline__ u32 seeds_of(u32 n, u32 S, u32 T) { return seeds_regular(n, S, T) + ((n - S) % T ? 1u : 0u); }

__global__ __launch_bounds__(256) void k_pile_seed_count(PileArgs A) {
  const u64 r = (u64)blockIdx.x * 256 + threadIdx.x;
  if (r >= A.n_reads) return;
  const u64 n = A.offs[r + 1] - A.offs[r];
  A.seed_cnt[r] = (n < A.p.seed_length || n > A.p.max_read_len) ? 0u : seeds_of((u32)n, A.p.seed_length, A.p.seed_stride);
}

__global__ __launch_bounds__(256) void k_pile_seed_fill(PileArgs A) {
  const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
  if (i >= A.seed_cap) return;
  const u32 S = A.p.seed_length;
  u64 total = *A.seed_total;
  total = total < A.seed_cap ? total : A.seed_cap;
  A.seed_offs[i] = (i < total ? i : total) * S;  // the slots behind the seeds are empty queries
  if (i == 0) A.seed_offs[A.seed_cap] = total * S;
  if (i >= total) return;
  const u64 r = last_at_most(A.seed_start, A.n_reads, i);  // the last read that starts at or before this seed: the one that has it
  const u64 b0 = A.offs[r];
  const u32 n = (u32)(A.offs[r + 1] - b0), j = (u32)(i - A.seed_start[r]);
  if (n < S || j >= seeds_of(n, S, A.p.seed_stride)) return;  // (not with a seed_start made from these reads)
  const u32 p = j < seeds_regular(n, S, A.p.seed_stride) ? j * A.p.seed_stride : n - S;
  const unsigned char* src = A.seqs + b0 + p;
  unsigned char* dst = A.seed_bytes + i * S;
  for (u32 k = 0; k < S; ++k) dst[k] = src[k];
}

__device__ __forceinline__ u64 shfl64(u64 v, int src) {
  return (u64)(u32)__shfl((int)(u32)v, src, 64) | ((u64)(u32)__shfl((int)(u32)(v >> 32), src, 64) << 32);
}

__device__ __forceinline__ u32 pile_hash(u64 k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 29;
  return (u32)k;
}

__global__ __launch_bounds__(64) void k_pile(PileArgs A) {
  extern __shared__ __align__(16) unsigned char pile_lds[];
  u64* cnt = reinterpret_cast<u64*>(pile_lds);               // [len_cap]: votes of a column, A C G T in 16 bits each
  u64* tab = cnt + A.len_cap;                                // [tab_cap]: candidate keys
  unsigned char* qs = reinterpret_cast<unsigned char*>(tab + A.tab_cap);  // [len_cap]: the read's codes, 4 = outside ACGT

  const u32 lane = threadIdx.x;
  const u64 r = blockIdx.x;
  const u64 total_hits = A.loc_status[0];
  if (total_hits > A.hits_cap) return;  // the caller's hits did not fit: nothing is written (sigax.h)

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
  for (u32 s = lane; s < A.tab_cap; s += 64) tab[s] = PILE_EMPTY;
  __syncthreads();

  // ---- rules 2-3: the seeds' flags, and the hits into the table of distinct triples ----
  u64 s0 = A.seed_start[r], s1 = A.seed_start[r + 1];
  s1 = s1 < A.seed_cap ? s1 : A.seed_cap;
  s0 = s0 < s1 ? s0 : s1;
  u32 located = 0, repeats = 0;
  for (u64 s = s0 + lane; s < s1; s += 64) {
    const u32 f = A.qflags[s];
    if (!(f & SIGAX_LOCATE_SKIPPED)) {
      located += 1u;
      if (f & SIGAX_LOCATE_OVER) repeats += 1u;
    }
  }
  u64 h0 = A.hit_offs[s0], h1 = A.hit_offs[s1];
  h1 = h1 < total_hits ? h1 : total_hits;
  h0 = h0 < h1 ? h0 : h1;
  const u32 n_reg = seeds_regular(n, S, T), n_seeds = (u32)(s1 - s0), tmask = A.tab_cap - 1u;
  u32 n_dist = 0;
  bool over = false;
  for (u64 base = h0; base < h1; base += 64) {
    const u64 i = base + lane;
    u32 ins = 0;
    if (i < h1) {
      const uint4 h = reinterpret_cast<const uint4*>(A.hits)[i];  // {seed, read, offset, flags}
      const u32 j = h.x - (u32)s0;
      if (!(h.w & SIGAX_HIT_CUT) && (u64)h.y < A.n_ref && j < n_seeds) {
        const long long p = j < n_reg ? (long long)j * T : (long long)(n - S);
        long long d;
        if (h.w & SIGAX_HIT_REV) {
          const long long len_t = (long long)(A.ref_offs[(u64)h.y + 1] - A.ref_offs[h.y]);
          d = len_t - (long long)h.z - (long long)S - p;
        } else {
          d = (long long)h.z - p;
        }
        if (d >= -PILE_D_BIAS && d < PILE_D_BIAS) {
          const u64 key = ((u64)h.y << 32) | ((u64)(u32)(d + PILE_D_BIAS) << 1) | ((h.w & SIGAX_HIT_REV) ? 1ull : 0ull);
          u32 slot = pile_hash(key) & tmask;
          for (u32 probe = 0; probe < A.tab_cap; ++probe) {  // the table is never full: at most K + 64 keys in (K + 64) 4/3 slots
            const u64 old = atomicCAS(reinterpret_cast<unsigned long long*>(&tab[slot]), PILE_EMPTY, key);
            if (old == PILE_EMPTY) {
              ins = 1u;
              break;
            }
            if (old == key) break;
            slot = (slot + 1u) & tmask;
          }
        }
      }
    }
    n_dist += (u32)wave_sum((u64)ins);
    if (n_dist > A.p.max_candidates) {
      over = true;
      break;
    }
  }
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
    const u64 key = tab[base + lane];
    const bool has = key != PILE_EMPTY;
    u64 rb = 0;
    u32 len_t = 0;
    if (has) {  // (a key's read is below n_ref)
      const u64 t = key >> 32;
      rb = A.ref_offs[t];
      len_t = (u32)(A.ref_offs[t + 1] - rb);
    }
    u64 mask = __ballot(has);
    while (mask) {
      const int src = __ffsll((long long)mask) - 1;
      mask &= mask - 1ull;
      const u64 k = shfl64(key, src), crb = shfl64(rb, src);
      const long long clen = (long long)(u32)__shfl((int)len_t, src, 64);
      const bool rev = (k & 1ull) != 0ull;
      const long long d = (long long)(((u32)k) >> 1) - PILE_D_BIAS;
      const long long x0 = d < 0 ? -d : 0, x1 = (clen - d) < (long long)n ? (clen - d) : (long long)n;
      if (x1 <= x0) continue;  // (a hit's window lies in both texts: there is an overlap)
      const u32 ell = (u32)(x1 - x0), steps = (ell + 63u) >> 6;  // <= 64: ell <= n <= 4096
      const unsigned char* text = A.ref_text + crb;
      u64 held0 = 0, held1 = 0;
      u32 mism = 0;
      for (u32 c = 0; c < steps; ++c) {
        const long long x = x0 + (long long)(c * 64u + lane);
        if (x < x1) {
          const long long pos = x + d;  // in [0, clen)
          const u32 rk = base_rank(rev ? text[clen - 1 - pos] : text[pos]);
          u32 code = (rk - 1u) & 3u;  // the reference text holds ACGT only
          code = rev ? 3u - code : code;
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
  const u64 hits = A.loc_status[0];
  const bool fits = hits <= A.hits_cap;
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

void launch_ref_iota(unsigned long long* rows, unsigned long long n, hipStream_t st) {
  if (n) hipLaunchKernelGGL(k_ref_iota, dim3(blocks_of(n)), dim3(256), 0, st, rows, n);
}

void launch_ref_order(const RefOrderArgs& a, hipStream_t st) {
  if (a.n) hipLaunchKernelGGL(k_ref_order, dim3(blocks_of(a.n)), dim3(256), 0, st, a);
}

void launch_pile_seed_count(const PileArgs& a, hipStream_t st) {
  if (a.n_reads) hipLaunchKernelGGL(k_pile_seed_count, dim3(blocks_of(a.n_reads)), dim3(256), 0, st, a);
}

void launch_pile_seed_fill(const PileArgs& a, hipStream_t st) {
  if (a.seed_cap) hipLaunchKernelGGL(k_pile_seed_fill, dim3(blocks_of(a.seed_cap)), dim3(256), 0, st, a);
}

uint32_t pile_tab_cap(uint32_t max_candidates) {
  // a batch of 64 hits may carry the table 64 keys past K before the count is looked at; a quarter of the slots stay free
  const uint32_t need = (max_candidates + 64u) / 3u * 4u + 4u;
  uint32_t cap = 128;
  while (cap < need) cap <<= 1;
  return cap;
}

uint32_t pile_lds_bytes(uint32_t len_cap, uint32_t tab_cap) { return len_cap * 8u + tab_cap * 8u + len_cap; }

int launch_pile(const PileArgs& a, hipStream_t st) {
  if (a.n_reads == 0) return (int)hipSuccess;
  const uint32_t lds = pile_lds_bytes(a.len_cap, a.tab_cap);
  if (lds > 32768u) {  // above what a launch gets unasked: up to the 160 KiB of a CDNA4 compute unit
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_pile), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(k_pile, dim3((unsigned)a.n_reads), dim3(64), lds, st, a);
  return (int)hipSuccess;
}

void launch_pile_status(const PileArgs& a, hipStream_t st) { hipLaunchKernelGGL(k_pile_status, dim3(1), dim3(64), 0, st, a); }
