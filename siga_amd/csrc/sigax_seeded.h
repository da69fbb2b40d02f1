// siga_amd/csrc/sigax_seeded.h -- the seeding stage and the candidate table that the seed-and-verify family shares
// (sigax_pileup.*: `siga correct -a overlap`; sigax_mmoverlap.*: `siga overlap -e`), each piece once:
//   reference text  the indexed reads by id (RefOrderArgs; sigax_reference_text_*, sigax_pile_ref_* in sigax_seeded.cpp)
//   seeds           SeedArgs and the two seed kernels of sigax_seeded.hip; what locate left of them (SeedHits) over a text (RefText)
//   host            the workspace's common front and back (SeedWork, seed_work), the stage itself (seed_enqueue), the checks and
//                   the decisions of a batch loop that do not depend on what is verified
//   device          for a .hip file that has included sigax_rank.h: the candidate table (CAND_*, cand_*), seed_span, seed_flags,
//                   seeds_regular / seeds_of, launch_wave_lds.  Device-inline only; every translation unit gets its own copy.
#ifndef SIGA_AMD_SIGAX_SEEDED_H_
#define SIGA_AMD_SIGAX_SEEDED_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sigax.h"

#define SEED_REF_MAX_LEN 0x3FFFFFFFu  // reference reads are shorter than 2^30 bases (the diagonal's 31 bits, CAND_D_BIAS)

// ---- reference text -----------------------------------------------------------------------------------------------------------------
// By read id: the lengths pass has left lens[i] and stretch[i] of BWT row i; k_ref_order turns them into
// rows_by_id[sai[stretch[i]]] = i and lens_by_id[...] = lens[i], which the scan and the write pass take.
struct RefOrderArgs {
  const uint32_t* lens;                  // [n] by row
  const unsigned long long* stretch;     // [n] by row
  const uint32_t* sai;                   // [n]
  unsigned long long n;
  unsigned long long* rows_by_id;        // [n], preset to n (a row out of range: length 0)
  uint32_t* lens_by_id;                  // [n], zeroed
  unsigned long long* bad;               // 1 u64, zeroed: rows whose walk was cut or whose stretch names no read
};
void launch_ref_order(const RefOrderArgs& a, hipStream_t st);
void launch_ref_iota(unsigned long long* rows, unsigned long long n, hipStream_t st);  // rows[i] = i

struct sigax_pile_ref {
  int device;
  unsigned long long n_strings, text_bytes;
  unsigned char* d_text;
  unsigned long long* d_offs;
};

struct RefText {
  const unsigned char* ref_text;
  const unsigned long long* ref_offs;    // [n_ref + 1]
  unsigned long long n_ref;
};

// ---- seeds --------------------------------------------------------------------------------------------------------------------------
// what k_seed_count and k_seed_fill read and write: the windows of S bases at 0, T, 2T, ... and the one that ends the read, none
// for a read shorter than S or longer than max_read_len, as the query table of sigax_locate_device
struct SeedArgs {
  const unsigned char* seqs;
  const unsigned long long* offs;        // [n_reads + 1]
  unsigned long long n_reads;
  uint32_t S, T, max_read_len;
  uint32_t* seed_cnt;                    // [n_reads]
  unsigned long long* seed_start;        // [n_reads + 1]
  unsigned long long* seed_total;        // 1 u64: seed_start[n_reads]
  unsigned long long seed_cap;           // seed slots (queries of the locate call)
  unsigned char* seed_bytes;             // [seed_cap * S + 16]
  unsigned long long* seed_offs;         // [seed_cap + 1]
};
void launch_seed_count(const SeedArgs& a, hipStream_t st);
void launch_seed_fill(const SeedArgs& a, hipStream_t st);

// what locate left.  Hit is `const uint4` for a kernel that only reads the hits ({seed, read, offset, flags}, a sigax_hit) and
// `uint4` for one that leaves its results in their place.
template <class Hit>
struct SeedHits {
  const unsigned long long* seed_start;  // [n_reads + 1]
  unsigned long long seed_cap;
  const uint32_t* qflags;                // [seed_cap]
  const unsigned long long* hit_offs;    // [seed_cap + 1]
  Hit* hits;                             // [hits_cap]
  unsigned long long hits_cap;
  const unsigned long long* loc_status;  // 4 u64: [0] = hits listed
};

// ---- host ---------------------------------------------------------------------------------------------------------------------------
// The workspace of a seeded call, offsets from a 16-byte aligned base: the common front, `middle_bytes` of the caller's own, the
// common back.  words, 16 u64: [0] seeds, [1..3] the caller's, [4..7] locate's status, [8..15] the caller's counters.
struct SeedWork {
  unsigned long long seed_cap;
  unsigned long long seed_cnt, seed_start, partial, words, middle, seed_bytes, seed_offs, totals, qflags, hit_offs, loc_work, loc_work_bytes,
      hits, bytes;
};
// SIGAX_E_ARG for more seed slots than a hit names in 32 bits and for a hits_cap above LOCATE_MAX_SLOTS
int seed_work(unsigned long long n, unsigned long long n_bases, uint32_t S, uint32_t T, unsigned long long hits_cap,
              unsigned long long middle_bytes, SeedWork* out);
// The stage: words and the first zero_middle bytes of the middle zeroed, then seeds counted, scanned, filled and located on both
// strands with at most H hits a seed.  Hits over hits_cap: words[4] carries the number and the kernels behind it write nothing.
int seed_enqueue(sigax_index* ix, const unsigned char* d_seqs, const unsigned long long* d_offs, unsigned long long n, uint32_t S, uint32_t T,
                 uint32_t max_read_len, uint32_t H, void* d_work, const SeedWork& w, unsigned long long zero_middle,
                 unsigned long long hits_cap, hipStream_t st);
template <class Hit>
SeedHits<Hit> seed_hits(void* d_work, const SeedWork& w, unsigned long long hits_cap) {
  char* base = (char*)d_work;
  return {(const unsigned long long*)(base + w.seed_start), w.seed_cap, (const uint32_t*)(base + w.qflags),
          (const unsigned long long*)(base + w.hit_offs), (Hit*)(base + w.hits), hits_cap, (const unsigned long long*)(base + w.words) + 4};
}

unsigned long long up16(unsigned long long v);
unsigned long long env_u64(const char* name, unsigned long long dflt);  // a test hook, read per call
// the index names its reads and holds ACGT only; `needs` and `cannot` are the feature's words in the two refusals
int seeded_usable(const sigax_index* ix, const char* needs, const char* cannot);
int seeded_check_params(uint32_t seed_length, uint32_t seed_stride, uint32_t max_seed_hits, uint32_t min_overlap, uint32_t error_permille,
                        uint32_t max_candidates, uint32_t max_read_len, uint32_t reserved);
// max_read_len 0: SIGAX_PILE_MAX_LEN in a device call; in a batch, the longest of its n reads
uint32_t seeded_max_len(uint32_t max_read_len);
uint32_t seeded_max_len(uint32_t max_read_len, const unsigned long long* offs, unsigned long long n);
// the first try of a piece of nb bases (test_cap, a hook, when it is not ~0); and after a call that listed more hits than that:
// *hits_cap raised for the next try, or *split set, or the failure of a single read whose hits do not fit
unsigned long long seeded_first_hits_cap(unsigned long long test_cap, unsigned long long nb, unsigned long long budget);
int seeded_hits_overflow(unsigned long long listed, unsigned long long budget, unsigned long long cnt, unsigned long long* hits_cap, bool* split);

// slots of the candidate table for K candidates: a batch of 64 hits may carry the table 64 keys past K before the count is looked
// at; a quarter of the slots stay free
inline uint32_t cand_tab_cap(uint32_t max_candidates) {
  const uint32_t need = (max_candidates + 64u) / 3u * 4u + 4u;
  uint32_t cap = 128;
  while (cap < need) cap <<= 1;
  return cap;
}

// ---- device -------------------------------------------------------------------------------------------------------------------------
#ifdef SIGA_AMD_SIGAX_RANK_H_
namespace {

#define CAND_EMPTY (~0ull)
#define CAND_D_BIAS (1ll << 30)  // diagonals are kept as d + 2^30 in 31 bits: reference reads are shorter than 2^30 bases

// the windows at 0, T, 2T, ... and the one that ends the read
__device__ __forceinline__ u32 seeds_regular(u32 n, u32 S, u32 T) { return (n - S) / T + 1u; }
__device__ __forceinline__ u32 seeds_of(u32 n, u32 S, u32 T) { return seeds_regular(n, S, T) + ((n - S) % T ? 1u : 0u); }

__device__ __forceinline__ u32 cand_hash(u64 k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 29;
  return (u32)k;
}

// the seeds of read r of the call and its stretch of the hit list: all clamped to what the buffers hold
struct SeedSpan {
  u64 s0, s1, h0, h1;
};
template <class Hit>
__device__ __forceinline__ SeedSpan seed_span(const SeedHits<Hit>& L, u64 r, u64 total_hits) {
  SeedSpan sp;
  sp.s0 = L.seed_start[r];
  sp.s1 = L.seed_start[r + 1];
  sp.s1 = sp.s1 < L.seed_cap ? sp.s1 : L.seed_cap;
  sp.s0 = sp.s0 < sp.s1 ? sp.s0 : sp.s1;
  sp.h0 = L.hit_offs[sp.s0];
  sp.h1 = L.hit_offs[sp.s1];
  sp.h1 = sp.h1 < total_hits ? sp.h1 : total_hits;
  sp.h0 = sp.h0 < sp.h1 ? sp.h0 : sp.h1;
  return sp;
}

// this lane's share of the read's seeds: those located, and those of them skipped as repeats
template <class Hit>
__device__ __forceinline__ void seed_flags(const SeedHits<Hit>& L, const SeedSpan& sp, u32 lane, u32& located, u32& repeats) {
  located = repeats = 0;
  for (u64 s = sp.s0 + lane; s < sp.s1; s += 64) {
    const u32 f = L.qflags[s];
    if (!(f & SIGAX_LOCATE_SKIPPED)) {
      located += 1u;
      if (f & SIGAX_LOCATE_OVER) repeats += 1u;
    }
  }
}

// The hits of a read of n bases, 64 at a time and one per lane, into the table of distinct triples (tab[0, tab_cap) preset to
// CAND_EMPTY, tab_cap a power of two): a hit becomes the key {read, diagonal + CAND_D_BIAS, strand}, a forward hit (t, o) of the
// seed at p giving d = o - p and a reverse one d = len(t) - o - S - p, and goes in with a 64-bit compare-and-swap.  -> more than
// K distinct keys: the read is over, the table is of no use.
template <class Hit>
__device__ __forceinline__ bool cand_collect(u64* tab, u32 tab_cap, const SeedHits<Hit>& L, const SeedSpan& sp, const RefText& R, u32 n, u32 S,
                                             u32 T, u32 K, u32 lane) {
  const u32 n_reg = seeds_regular(n, S, T), n_seeds = (u32)(sp.s1 - sp.s0), tmask = tab_cap - 1u;
  u32 n_dist = 0;
  for (u64 base = sp.h0; base < sp.h1; base += 64) {
    const u64 at = base + lane;
    u32 ins = 0;
    if (at < sp.h1) {
      const uint4 h = L.hits[at];  // {seed, read, offset, flags}
      const u32 j = h.x - (u32)sp.s0;
      if (!(h.w & SIGAX_HIT_CUT) && (u64)h.y < R.n_ref && j < n_seeds) {
        const long long p = j < n_reg ? (long long)j * T : (long long)(n - S);
        long long d;
        if (h.w & SIGAX_HIT_REV) {
          const long long len_t = (long long)(R.ref_offs[(u64)h.y + 1] - R.ref_offs[h.y]);
          d = len_t - (long long)h.z - (long long)S - p;
        } else {
          d = (long long)h.z - p;
        }
        if (d >= -CAND_D_BIAS && d < CAND_D_BIAS) {
          const u64 key = ((u64)h.y << 32) | ((u64)(u32)(d + CAND_D_BIAS) << 1) | ((h.w & SIGAX_HIT_REV) ? 1ull : 0ull);
          u32 slot = cand_hash(key) & tmask;
          for (u32 probe = 0; probe < tab_cap; ++probe) {  // the table is never full: at most K + 64 keys in (K + 64) 4/3 slots
            const u64 old = atomicCAS(reinterpret_cast<unsigned long long*>(&tab[slot]), CAND_EMPTY, key);
            if (old == CAND_EMPTY) {
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
    if (n_dist > K) return true;
  }
  return false;
}

// a lane's own slot of a sweep: its key and, when it holds one, where its read's text lies (a key's read is below n_ref);
// more(t) loads what else the caller wants of read t, so that the 64 lanes' loads are all in flight together
template <class More>
__device__ __forceinline__ bool cand_slot(const u64* tab, u32 slot, const RefText& R, u64& key, u64& rb, u32& len_t, More more) {
  key = tab[slot];
  const bool has = key != CAND_EMPTY;
  rb = 0;
  len_t = 0;
  if (has) {
    const u64 t = key >> 32;
    rb = R.ref_offs[t];
    len_t = (u32)(R.ref_offs[t + 1] - rb);
    more(t);
  }
  return has;
}

// lane src's slot for the whole wave, facing a query of n columns: candidate t on strand rev at diagonal d, its text of clen
// bases at ref_text + rb, the columns [x0, x1) in both (x1 <= x0: none)
struct SeedCand {
  u64 rb;
  u32 t;
  bool rev;
  long long d, x0, x1, clen;
};
__device__ __forceinline__ SeedCand cand_decode(u64 key, u64 rb, u32 len_t, int src, u32 n) {
  SeedCand c;
  const u64 k = shfl64(key, (u32)src);
  c.rb = shfl64(rb, (u32)src);
  c.clen = (long long)(u32)__shfl((int)len_t, src, 64);
  c.t = (u32)(k >> 32);
  c.rev = (k & 1ull) != 0ull;
  c.d = (long long)(((u32)k) >> 1) - CAND_D_BIAS;
  c.x0 = c.d < 0 ? -c.d : 0;
  c.x1 = (c.clen - c.d) < (long long)n ? (c.clen - c.d) : (long long)n;
  return c;
}

// the 2-bit code of the candidate at pos in [0, clen), reversed and complemented for the reverse strand; the text holds ACGT only
__device__ __forceinline__ u32 cand_code(const unsigned char* text, long long clen, long long pos, bool rev) {
  const u32 code = (base_rank(rev ? text[clen - 1 - pos] : text[pos]) - 1u) & 3u;
  return rev ? 3u - code : code;
}

// one wave a workgroup with `lds` bytes of dynamic LDS; above what a launch gets unasked the limit is raised, up to the 160 KiB
// of a CDNA4 compute unit.  -> hipSuccess or the error of raising it
template <class Kernel, class Args>
int launch_wave_lds(Kernel kernel, const Args& a, unsigned long long n_waves, uint32_t lds, hipStream_t st) {
  if (n_waves == 0) return (int)hipSuccess;
  if (lds > 32768u) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
  }
  hipLaunchKernelGGL(kernel, dim3((unsigned)n_waves), dim3(64), lds, st, a);
  return (int)hipSuccess;
}

}  // namespace
#endif

#endif
