// siga_amd/csrc/sigax_fm.h -- how device code reads an index (fm_layout.h), each piece once.  What the kernels of
// sigax_kernels.hip, sigax_tables.hip and sigax_tail.hip share, and the leaves that sigax_rank.h hands on to the kernels
// that walk the forward strand symbol by symbol:
//   leaves        PosOf, base_rank, comp_rank, chunk_count (a uint4 piece of a one-step granule), sel4, sel5, first_lane64;
//                 the wave sum is sigax_device.h's
//   rank views    Cnt4, Cnt4P, a strand by value (FmRef, fm_ref, fm_pick), C[] and the totals of both strands in LDS (FmTables,
//                 fm_tables_load), fm_rank, fm_rank5, fm_rank4p, fm_char
//   table readers packed_get, row_lookup, text_window, text_bits (row table and stretch text), deep_slot, deep_lookup (deep
//                 start table); sigax_tables.hip builds what they read
//   records       SIGAX_NT; the finder's candidate record (Cand, cand_store, cand_load); store_block
//   launch        nblk (host)
// Not here, because their operands have other shapes: gran_rank, Gran1, Gran2 and rank2 of sigax_rank.h; Gran, Gran2, rank2_from
// and fm_rank4p_from of the finder (sigax_kernels.hip).
// Device-inline only; every translation unit gets its own copy.
#ifndef SIGA_AMD_SIGAX_FM_H_
#define SIGA_AMD_SIGAX_FM_H_

#include <hip/hip_runtime.h>

#include "fm_layout.h"
#include "sigax_device.h"

// Non-temporal hints on data that passes through once -- the finder's candidate records on their way out (bit 2), the
// records on their way into filter/extract (4), the row-table line a block looks up (1): they leave more of the caches to
// the finder's tables.  Measured at BASELINE configs[1] (gpurun_out/r3w/): 118.6 M reads/s without, 119.4-120.5 M with one
// of them, 121.0 M with all three; nothing at the configs[2] shape.  -DSIGAX_NT=0 turns them off.
#ifndef SIGAX_NT
#define SIGAX_NT 7
#endif

namespace {

// ---- leaves -------------------------------------------------------------------------------------------------------------------------
// Position type of an index: u32 while the BWT has fewer than 2^32 symbols (half the registers and ALU work), else u64.
template <bool WIDE> struct PosOf { typedef u32 type; };
template <> struct PosOf<true> { typedef u64 type; };

// alphabet.h:19-39 and kseq.cpp:18-27: byte -> rank; complement in rank space (non-ACGT -> 0 either way)
// Branch-free (a chain of equality tests on one value is lowered to a divergent branch tree): bits 1-2 of 'A','C','T','G'
// are 0,1,2,3; the byte expected at that index and its rank come out of two constants.
__device__ __forceinline__ u32 base_rank(u32 ch) {
  const u32 i = (ch >> 1) & 3u;
  const u32 expect = (0x47544341u >> (i * 8)) & 0xFFu;  // "ACTG"
  const u32 rank = (0x3421u >> (i * 4)) & 0xFu;         // 1, 2, 4, 3
  return expect == ch ? rank : 0u;
}
__device__ __forceinline__ u32 comp_rank(u32 r) { return r ? 5u - r : 0u; }

__device__ __forceinline__ void chunk_count(const uint4& k, int take, u32& a, u32& c, u32& g, u32& t) {
  u32 m = take >= 32 ? 0xFFFFFFFFu : (take <= 0 ? 0u : ((1u << take) - 1u));
  u32 x0 = k.y & m, x1 = k.z & m, x2 = k.w & m;
  a += __popc(x0 & ~x1);
  c += __popc(x1 & ~x0);
  g += __popc(x0 & x1);
  t += __popc(x2);
}

template <typename T>
__device__ __forceinline__ T sel4(u32 i, T v0, T v1, T v2, T v3) {  // v[i], i in 0..3, out of registers
  const T t01 = (i & 1u) ? v1 : v0, t23 = (i & 1u) ? v3 : v2;
  return (i & 2u) ? t23 : t01;
}
// v[r] for r in 0..4 out of registers, as a select tree on the bits of r (again: no equality chain, no branches)
template <typename T>
__device__ __forceinline__ T sel5(u32 r, T v0, T v1, T v2, T v3, T v4) {
  const bool b0 = (r & 1u) != 0, b1 = (r & 2u) != 0, b2 = (r & 4u) != 0;
  const T t01 = b0 ? v1 : v0, t23 = b0 ? v3 : v2;
  const T t = b1 ? t23 : t01;
  return b2 ? v4 : t;
}

__device__ __forceinline__ u64 first_lane64(u64 v) {
  return (u64)__builtin_amdgcn_readfirstlane((u32)v) | ((u64)__builtin_amdgcn_readfirstlane((u32)(v >> 32)) << 32);
}

// ---- rank views: number of A,C,G,T in BWT[0, p)   == FMIndex::getOcc(p - 1) without the '$' column ------------------------------
struct Cnt4 {
  u64 a, c, g, t;
};
template <typename P> struct Cnt4P {
  P a, c, g, t;
};

// By-value view of one strand: granule table, superblock table, length, and which LDS row holds its C[]/totals.
struct FmRef {
  const uint4* g;
  const u64* super;
  u64 n;
  u32 which;
};
__device__ __forceinline__ FmRef fm_ref(const FmStrand& s, u32 which) {
  FmRef r;
  r.g = reinterpret_cast<const uint4*>(s.granules);
  r.super = s.super;
  r.n = s.n;
  r.which = which;
  return r;
}
__device__ __forceinline__ FmRef fm_pick(bool first, const FmRef& a, const FmRef& b) {
  FmRef r;
  r.g = first ? a.g : b.g;
  r.super = first ? a.super : b.super;
  r.n = first ? a.n : b.n;
  r.which = first ? a.which : b.which;
  return r;
}
// C[] and symbol totals of both strands staged in LDS: [which][rank]
struct FmTables {
  u64 C[2][5];
  u64 T[2][5];
};
__device__ __forceinline__ void fm_tables_load(FmTables& t, const FmStrand& fwd, const FmStrand& rev) {
  if (threadIdx.x < 5) {
    t.C[0][threadIdx.x] = fwd.C[threadIdx.x];
    t.C[1][threadIdx.x] = rev.C[threadIdx.x];
    t.T[0][threadIdx.x] = fwd.total[threadIdx.x];
    t.T[1][threadIdx.x] = rev.total[threadIdx.x];
  }
  __syncthreads();
}

template <bool WIDE>
__device__ __forceinline__ Cnt4 fm_rank(const FmRef& s, u64 p) {
  p = p > s.n ? s.n : p;  // never leave the table, whatever an invalid interval holds
  u64 gi = p >> 7;
  int r = (int)(p & 127u);
  const uint4* q = s.g + gi * 4;
  uint4 k0 = q[0], k1 = q[1], k2 = q[2], k3 = q[3];
  u32 a = k0.x, c = k1.x, g = k2.x, t = k3.x;
  chunk_count(k0, r, a, c, g, t);
  chunk_count(k1, r - 32, a, c, g, t);
  chunk_count(k2, r - 64, a, c, g, t);
  chunk_count(k3, r - 96, a, c, g, t);
  Cnt4 o;
  o.a = a; o.c = c; o.g = g; o.t = t;
  if (WIDE) {
    const u64* sb = s.super + (p >> SIGAX_SUPER_SHIFT) * 4;
    o.a += sb[0]; o.c += sb[1]; o.g += sb[2]; o.t += sb[3];
  }
  return o;
}

// all five columns; v[0] = '$'
template <bool WIDE>
__device__ __forceinline__ void fm_rank5(const FmRef& s, u64 p, u64 v[5]) {
  u64 pc = p > s.n ? s.n : p;
  Cnt4 k = fm_rank<WIDE>(s, pc);
  v[1] = k.a; v[2] = k.c; v[3] = k.g; v[4] = k.t;
  v[0] = pc - (k.a + k.c + k.g + k.t);
}

// A,C,G,T counts of BWT[0, p) in the index's position type
template <bool WIDE>
__device__ __forceinline__ Cnt4P<typename PosOf<WIDE>::type> fm_rank4p(const FmRef& s, typename PosOf<WIDE>::type p) {
  typedef typename PosOf<WIDE>::type P;
  u64 pc = (u64)p > s.n ? s.n : (u64)p;
  const uint4* q = s.g + (pc >> 7) * 4;
  int r = (int)(pc & 127u);
  uint4 k0 = q[0], k1 = q[1], k2 = q[2], k3 = q[3];
  u32 a = k0.x, c = k1.x, g = k2.x, t = k3.x;
  chunk_count(k0, r, a, c, g, t);
  chunk_count(k1, r - 32, a, c, g, t);
  chunk_count(k2, r - 64, a, c, g, t);
  chunk_count(k3, r - 96, a, c, g, t);
  Cnt4P<P> o;
  o.a = a; o.c = c; o.g = g; o.t = t;
  if (WIDE) {
    const u64* sb = s.super + (pc >> SIGAX_SUPER_SHIFT) * 4;
    o.a += (P)sb[0]; o.c += (P)sb[1]; o.g += (P)sb[2]; o.t += (P)sb[3];
  }
  return o;
}

// BWT symbol at position i (FMIndex::getChar, src/fmindex.cpp:233-246)
__device__ __forceinline__ u32 fm_char(const FmRef& s, u64 i) {
  const u32* q = reinterpret_cast<const u32*>(s.g) + (i >> 7) * 16 + ((i >> 5) & 3) * 4;
  u32 b = (u32)i & 31u;
  return ((q[1] >> b) & 1u) | (((q[2] >> b) & 1u) << 1) | (((q[3] >> b) & 1u) << 2);
}

// ---- table readers: row table and stretch text (fm_layout.h; k_stretch_scan and k_rows_fill of sigax_tables.hip build them) ---------
// entry p of a bit-packed table of `bits`-bit values (packed_or of sigax_tables.hip sets it)
__device__ __forceinline__ u64 packed_get(const unsigned char* tab, u64 p, u32 bits) {
  const u64 B = p * bits;
  u64 v;
#if (SIGAX_NT & 1)
  {  // the row-table line is used once
    typedef u64 __attribute__((aligned(1))) u64u;
    v = __builtin_nontemporal_load(reinterpret_cast<const u64u*>(tab + (B >> 3)));
  }
#else
  __builtin_memcpy(&v, tab + (B >> 3), 8);  // one unaligned 8-byte load (the table is padded by 8 bytes)
#endif
  return (v >> ((u32)B & 7u)) & ((1ull << bits) - 1ull);
}
// (stretch, offset) of the suffix at `row` of a strand that has the row table; returns the entry's symbols (fm_layout.h)
__device__ __forceinline__ u64 row_lookup(const FmStrand& st, u64 row, u32& ld, u32& t) {
  const u64 v = packed_get(st.sa, row < st.n ? row : 0ull, st.sa_bits);  // never leave the table, whatever a block holds
  ld = (u32)(v & ((1ull << st.ld_bits) - 1ull));
  t = (u32)(v >> st.ld_bits) & ((1u << st.t_bits) - 1u);
  return v >> (st.ld_bits + st.t_bits);
}
// The symbols on the backward path from offset t of stretch ld, 2 bits each (rank - 1), next one in the top two bits:
// offsets t-1, t-2, ... -- at least SIGAX_TEXT_WINDOW of them, or all t (the caller knows from t where the read ends).
__device__ __forceinline__ u64 text_window(const FmStrand& st, u32 ld, u32 t) {
  if (t == 0) return 0ull;
  const u32 end = 2u * t;                                  // the row's bits [0, end) hold offsets 0 .. t-1
  const u32 b = end > 64u ? (end - 64u + 7u) >> 3 : 0u;  // first byte of the 8 that end at or past bit `end`
  u64 w;
  __builtin_memcpy(&w, st.text + (u64)ld * st.text_stride + b, 8);  // rows are padded (fm_layout.h)
  return w << (64u - (end - 8u * b));
}
__device__ __forceinline__ u64 text_bits(const FmStrand& st, u32 ld, u32 off) {  // symbols off, off+1, ... lowest first
  u64 w;
  __builtin_memcpy(&w, st.text + (u64)ld * st.text_stride + (off >> 2), 8);
  return w >> (2u * (off & 3u));
}

// ---- table readers: deep start table (fm_layout.h; k_deep_scan and k_deep_fill of sigax_tables.hip build it) ------------------------
__device__ __forceinline__ u64 deep_slot(u64 k0, u64 k1, u64 nslots) {
  u64 h = (k0 ^ (k1 * 0x9E3779B97F4A7C15ull)) * 0xBF58476D1CE4E5B9ull;
  h ^= h >> 31;
  h *= 0x94D049BB133111EBull;
  h ^= h >> 29;
  return __umul64hi(h, nslots);
}
// the chain's state after the K-mer (k0, k1 = its code with the tag of fm_layout.h), or false: not a K-mer of the text
template <bool WIDE>
__device__ __forceinline__ bool deep_lookup(const void* tab, u64 nslots, u64 k0, u64 k1, typename PosOf<WIDE>::type& lo0,
                                            typename PosOf<WIDE>::type& lo1, typename PosOf<WIDE>::type& sz) {
  typedef typename PosOf<WIDE>::type P;
  const ulonglong2* q = reinterpret_cast<const ulonglong2*>(tab);
  u64 slot = deep_slot(k0, k1, nslots);
  for (;;) {
    const ulonglong2 key = q[2 * slot], pay = q[2 * slot + 1];
    if (key.y == 0ull) return false;  // an empty slot ends the probe sequence (the table is never full)
    if (key.x == k0 && key.y == k1) {
      if (WIDE) {
        const u64 m40 = (1ull << 40) - 1ull;
        lo0 = (P)(pay.x & m40);
        lo1 = (P)((pay.x >> 40) | ((pay.y & 0xFFFFull) << 24));
        sz = (P)((pay.y >> 16) & m40);
      } else {
        lo0 = (P)(u32)pay.x;
        lo1 = (P)(u32)(pay.x >> 32);
        sz = (P)(u32)pay.y;
      }
      return true;
    }
    slot = slot + 1 == nslots ? 0 : slot + 1;
  }
}

// ---- records ------------------------------------------------------------------------------------------------------------------------
// A candidate block as the finder leaves it in the arena: one naturally aligned record (32 B with u32 positions, 64 B
// with u64) = one or two 16-byte stores per half instead of the five scattered ones of an 80-byte sigax_block.
//   capped[0] = [c0lo, c0lo + d - 1], capped[1] = [c1lo, c1lo + d - 1]   (both intervals of a pair have one size)
//   raw[0]    = [r0lo, r0lo + sz - 1], raw[1]   = [r1lo, r1lo + sz - 1]
template <bool WIDE> struct Cand;
template <> struct __attribute__((aligned(32))) Cand<false> {
  u32 c0lo, d, c1lo, r0lo, r1lo, sz, len, af;
};
template <> struct __attribute__((aligned(64))) Cand<true> {
  u64 c0lo, d, c1lo, r0lo, r1lo, sz;
  u32 len, af;
  u64 pad;
};
static_assert(sizeof(Cand<false>) == 32 && sizeof(Cand<true>) == 64, "candidate record sizes");

__device__ __forceinline__ void cand_store(Cand<false>* dst, u32 c0lo, u32 d, u32 c1lo, u32 r0lo, u32 r1lo, u32 sz, u32 len, u32 af) {
  uint4* q = reinterpret_cast<uint4*>(dst);
  q[0] = make_uint4(c0lo, d, c1lo, r0lo);
  q[1] = make_uint4(r1lo, sz, len, af);
}
__device__ __forceinline__ void cand_store(Cand<true>* dst, u64 c0lo, u64 d, u64 c1lo, u64 r0lo, u64 r1lo, u64 sz, u32 len, u32 af) {
  ulonglong2* q = reinterpret_cast<ulonglong2*>(dst);
  q[0] = make_ulonglong2(c0lo, d);
  q[1] = make_ulonglong2(c1lo, r0lo);
  q[2] = make_ulonglong2(r1lo, sz);
  q[3] = make_ulonglong2((u64)len | ((u64)af << 32), 0ull);
}
template <bool WIDE>
__device__ __forceinline__ Cand<WIDE> cand_load(const Cand<WIDE>* src);
template <>
__device__ __forceinline__ Cand<false> cand_load<false>(const Cand<false>* src) {
  const uint4* q = reinterpret_cast<const uint4*>(src);
#if (SIGAX_NT & 4)
  typedef u32 nt4 __attribute__((ext_vector_type(4)));
  const nt4 na = __builtin_nontemporal_load(reinterpret_cast<const nt4*>(q)), nb = __builtin_nontemporal_load(reinterpret_cast<const nt4*>(q) + 1);
  uint4 a = make_uint4(na.x, na.y, na.z, na.w), b = make_uint4(nb.x, nb.y, nb.z, nb.w);
#else
  uint4 a = q[0], b = q[1];
#endif
  Cand<false> c;
  c.c0lo = a.x; c.d = a.y; c.c1lo = a.z; c.r0lo = a.w; c.r1lo = b.x; c.sz = b.y; c.len = b.z; c.af = b.w;
  return c;
}
template <>
__device__ __forceinline__ Cand<true> cand_load<true>(const Cand<true>* src) {
  const ulonglong2* q = reinterpret_cast<const ulonglong2*>(src);
  ulonglong2 a = q[0], b = q[1], c2 = q[2], d = q[3];
  Cand<true> c;
  c.c0lo = a.x; c.d = a.y; c.c1lo = b.x; c.r0lo = b.y; c.r1lo = c2.x; c.sz = c2.y; c.len = (u32)d.x; c.af = (u32)(d.x >> 32);
  c.pad = 0;
  return c;
}

// one 80-byte sigax_block as five 16-byte stores
__device__ __forceinline__ void store_block(sigax_block* dst, u64 c0lo, u64 c0hi, u64 c1lo, u64 c1hi, u64 r0lo, u64 r0hi,
                                            u64 r1lo, u64 r1hi, u32 len, u32 af) {
  ulonglong2* d = reinterpret_cast<ulonglong2*>(dst);
  d[0] = make_ulonglong2(c0lo, c0hi);
  d[1] = make_ulonglong2(c1lo, c1hi);
  d[2] = make_ulonglong2(r0lo, r0hi);
  d[3] = make_ulonglong2(r1lo, r1hi);
  d[4] = make_ulonglong2((u64)len | ((u64)af << 32), 0ull);
}

// ---- launch (host) ------------------------------------------------------------------------------------------------------------------
inline unsigned nblk(u64 n, u64 per) { return (unsigned)((n + per - 1) / per); }

}  // namespace

#endif
