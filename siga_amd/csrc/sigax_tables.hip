// siga_amd/csrc/sigax_tables.hip -- the device half of sigax_tables.cpp: the kernels that build an index's tables
// (fm_layout.h) and the two small index queries, with their launch wrappers and size functions (sigax_kernels.h).
//
//   k_occ_batch       FMIndex::getOcc                                        (src/fmindex.cpp:188-231,320-323)
//   k_kmer_count      FMIndex::Interval::occurrences                         (src/fmindex.h:67-86)
//   k_stretch_scan, k_rows_fill           row table and stretch text
//   k_isai, k_xmap                        direct map of a strand as extension index
//   k_suffix_order_check                  self-check of an index against the order of record
//   k_start_build                         start table of the block finder
//   k_deep_scan, k_deep_fill              deep start table of the block finder
//   k_build2_a, k_build2_b                two-step table
//
// How the hot path reads what these build is in sigax_fm.h (packed_get, row_lookup, text_window, text_bits, deep_slot,
// deep_lookup); the finder, filter/extract and the corrector are in sigax_kernels.hip, the scan that launch_build2 uses in
// sigax_tail.hip.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "sigax_kernels.h"
#include "sigax_fm.h"

// -------------------------------------------------------------------------------------------------------
// k_occ_batch / k_kmer_count
// -------------------------------------------------------------------------------------------------------
template <bool WIDE>
__global__ __launch_bounds__(256) void k_occ_batch(FmStrand s, const u64* pos, u64 n, u64* out) {
  u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  u64 v[5];
  fm_rank5<WIDE>(fm_ref(s, 0), pos[i] + 1, v);  // fmindex.cpp:191: ++i, so 2^64-1 wraps to the empty prefix
  for (int k = 0; k < 5; ++k) out[i * 5 + k] = v[k];
}

template <bool WIDE>
__global__ __launch_bounds__(256) void k_kmer_count(FmStrand s, const unsigned char* kmers, u32 k, u64 n, u64* out) {
  u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const unsigned char* w = kmers + i * k;
  FmRef f = fm_ref(s, 0);
  u64 C[5] = {s.C[0], s.C[1], s.C[2], s.C[3], s.C[4]};
  u64 T[5] = {s.total[0], s.total[1], s.total[2], s.total[3], s.total[4]};
  auto sel = [](const u64 v[5], u32 r) { return r == 0 ? v[0] : r == 1 ? v[1] : r == 2 ? v[2] : r == 3 ? v[3] : v[4]; };
  // Interval::get (fmindex.h:67-79): init with the last symbol, update while valid
  u32 r = base_rank(w[k - 1]);
  u64 lo = sel(C, r), hi = lo + sel(T, r) - 1;
  for (u32 j = k - 1; j > 0; --j) {
    if (!(hi != ~0ull && hi >= lo)) break;
    r = base_rank(w[j - 1]);
    u64 l[5], u[5];
    fm_rank5<WIDE>(f, lo, l);       // getOcc(c, lower - 1)
    fm_rank5<WIDE>(f, hi + 1, u);   // getOcc(c, upper)
    lo = sel(C, r) + sel(l, r);
    hi = sel(C, r) + sel(u, r) - 1;
  }
  out[i] = (hi != ~0ull && hi >= lo) ? hi - lo + 1 : 0;
}

// -------------------------------------------------------------------------------------------------------
// Row table + stretch text of fm_layout.h.  One lane per symbol of rank 0 in the text (a read's terminator, or a non-ACGT
// base, which the index stores as rank 0 too: alphabet.h:19-39): from the row of the suffix that starts there (rows
// 0 .. C['A']-1) walk backwards (LF) to the row whose BWT symbol has rank 0.  k_stretch_scan learns the distance and
// Occ('$') there (and the longest distance of the index, which sizes the entries); k_rows_fill walks again and writes
// (steps still to go, that Occ) at every row passed and the symbols passed into the stretch's text row.  Every row lies on
// exactly one such walk.
// -------------------------------------------------------------------------------------------------------
template <bool WIDE>
__device__ __forceinline__ u32 lf_row(const FmRef& f, const u64* C, u64 p, u64* next) {
  const u32 c = fm_char(f, p);
  const Cnt4 k = fm_rank<WIDE>(f, p);
  if (c == 0) *next = p - (k.a + k.c + k.g + k.t);  // Occ('$', p - 1)
  else *next = C[c] + (c == 1 ? k.a : c == 2 ? k.c : c == 3 ? k.g : k.t);
  return c;
}
#define STRETCH_BAD (~0ull)  // not a BWT of '$'-terminated reads: the walk did not end
template <bool WIDE>
__global__ __launch_bounds__(256) void k_stretch_scan(FmStrand s, u64 n_stretch, u64* info, u32* maxlen) {
  const u64 j = (u64)blockIdx.x * 256 + threadIdx.x;
  u32 mine = 0;
  if (j < n_stretch) {
    const FmRef f = fm_ref(s, 0);
    const u64 C[5] = {s.C[0], s.C[1], s.C[2], s.C[3], s.C[4]};
    u64 p = j, len = 0, v = STRETCH_BAD;
    for (;;) {
      u64 q;
      if (lf_row<WIDE>(f, C, p, &q) == 0) { v = (len << 32) | (q & 0xFFFFFFFFull); break; }
      p = q;
      if (++len >= s.n || len >= (1ull << 28)) { len = 0; break; }
    }
    info[j] = v;
    mine = (u32)len;
  }
  for (int off = 32; off > 0; off >>= 1) mine = max(mine, (u32)__shfl_xor((int)mine, off, 64));
  if ((threadIdx.x & 63u) == 0 && mine) atomicMax(maxlen, mine);
}
// entry p of a bit-packed table of `bits`-bit values (zeroed before): set (packed_get of sigax_fm.h reads it)
__device__ __forceinline__ void packed_or(unsigned char* tab, u64 p, u32 bits, u64 v) {
  const u64 B = p * bits;
  u64* w = reinterpret_cast<u64*>(tab) + (B >> 6);
  const u32 sh = (u32)B & 63u;
  atomicOr(w, v << sh);
  if (sh + bits > 64u) atomicOr(w + 1, v >> (64u - sh));
}
// direct map of strand X as extension index (fm_layout.h): sai_y = the other strand's .sai ids, isai_x = inverse of X's
__global__ __launch_bounds__(256) void k_xmap(const u32* sai_y, const u32* isai_x, const u32* slen_x, u64 n, u64* xmap) {
  const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const u32 ldx = isai_x[sai_y[i]];
  xmap[i] = (u64)ldx | ((u64)slen_x[ldx] << 32);
}
__global__ __launch_bounds__(256) void k_isai(const u32* sai, u64 n, u32* isai) {
  const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
  if (i < n) isai[sai[i]] = (u32)i;
}
// -------------------------------------------------------------------------------------------------------
// Self-check of an index against the order of record (sigax_index_check_order): the row table IS the suffix array, the
// stretch text IS the reads, so whether the BWT rows are in suffix order can be seen on the device without a second
// suffix sort: one lane per pair of adjacent rows compares the two suffixes of r0 $ r1 $ ... r(n-1) $ -- one '$' smaller
// than A, C, G, T, comparisons running on past a '$' into the next read, the end of the text smallest (the order `siga
// index` produces: SURVEY.md App. C model B; src/suffix_array_builder.cpp:472-674).  28 symbols per 8-byte load.
// -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_suffix_order_check(FmStrand st, const u32* sai, const u32* isai, const u32* read_len, u64 n_strings,
                                                            u64* bad) {
  const u64 p = (u64)blockIdx.x * 256 + threadIdx.x;
  if (p + 1 >= st.n) return;
  u32 la, ta, lb, tb;
  row_lookup(st, p, la, ta);
  row_lookup(st, p + 1, lb, tb);
  int verdict = -1;  // 1: suffix(p) < suffix(p + 1); 0: not
  for (u32 hops = 0; verdict < 0 && hops < 4096u; ++hops) {
    const u32 ida = sai[la], idb = sai[lb];
    const u32 ra = read_len[ida] - ta, rb = read_len[idb] - tb;  // symbols left in each read
    const u32 m = ra < rb ? ra : rb;
    for (u32 k = 0; k < m && verdict < 0;) {
      const u32 c = m - k < 28u ? m - k : 28u;
      const u64 x = (text_bits(st, la, ta + k) ^ text_bits(st, lb, tb + k)) & ((1ull << (2u * c)) - 1ull);
      if (x) {
        const u32 d = (u32)__builtin_ctzll(x) >> 1;
        const u32 sa = (u32)(text_bits(st, la, ta + k + d) & 3ull), sb = (u32)(text_bits(st, lb, tb + k + d) & 3ull);
        verdict = sa < sb ? 1 : 0;
      }
      k += c;
    }
    if (verdict >= 0) break;
    if (ra != rb) { verdict = ra < rb ? 1 : 0; break; }  // a '$' against a base
    // both reads end here: '$' against '$', on into the reads that follow them in the text (the end of the text is smallest)
    if ((u64)ida + 1 >= n_strings || (u64)idb + 1 >= n_strings) { verdict = ((u64)ida + 1 >= n_strings && (u64)idb + 1 < n_strings) ? 1 : 0; break; }
    la = isai[ida + 1]; ta = 0;
    lb = isai[idb + 1]; tb = 0;
  }
  if (verdict == 0) {
    atomicAdd(&bad[0], 1ull);
    atomicMin(&bad[1], p);
  } else if (verdict < 0) {
    atomicAdd(&bad[2], 1ull);  // undecided after 4096 reads' worth of ties (thousands of identical reads in a row)
  }
}

#define ROWS_KMAX 14  // most symbols an entry can carry (fm_layout.h)
template <bool WIDE>
__global__ __launch_bounds__(256) void k_rows_fill(FmStrand s, u64 n_stretch, const u64* info, unsigned char* sa, u32 sa_bits, u32 ld_bits, u32 t_bits,
                                                   unsigned char* text, u32 text_stride, u32* slen) {
  const u64 j = (u64)blockIdx.x * 256 + threadIdx.x;
  if (j >= n_stretch) return;
  const u64 v = info[j];
  if (v == STRETCH_BAD) return;  // rows of such a walk keep entry 0: "ends here, stretch 0" is never consulted then
  const FmRef f = fm_ref(s, 0);
  const u64 C[5] = {s.C[0], s.C[1], s.C[2], s.C[3], s.C[4]};
  const u64 ld = v & 0xFFFFFFFFull;
  if (slen != nullptr) slen[ld] = (u32)(v >> 32);  // the stretch's length, by its rank among the '$' rows
  const u32 K = sa != nullptr ? (sa_bits - ld_bits - t_bits) >> 1 : 0u;  // symbols carried by an entry
  u64 p = j;
  unsigned char* trow = text ? text + ld * text_stride : nullptr;
  // A window of the last ROWS_KMAX rows slides along: when the K-th symbol after a row has been seen its entry is complete
  // (R[ROWS_KMAX - 1] = the newest row; wsym = the symbols seen as rank - 1, newest in the lowest two bits, so the K
  // symbols that follow the row K places back read first-symbol-highest: the order text_window() hands them out in).
  u64 R[ROWS_KMAX];
  u32 wsym = 0, vm = 0;
#pragma unroll
  for (int i = 0; i < ROWS_KMAX; ++i) R[i] = 0;
  auto insert = [&](u64 row, u32 c, bool real, u64 t_of_row) {
#pragma unroll
    for (int i = 0; i + 1 < ROWS_KMAX; ++i) R[i] = R[i + 1];
    R[ROWS_KMAX - 1] = row;
    wsym = (wsym << 2) | ((c - 1u) & 3u);
    vm = (vm << 1) | (real ? 1u : 0u);
    if (K == 0 || sa == nullptr) return;
    u64 r0 = R[0];
#pragma unroll
    for (int i = 1; i < ROWS_KMAX; ++i)
      if ((u32)(ROWS_KMAX - i) == K) r0 = R[i];
    if ((vm >> (K - 1u)) & 1u) {
      const u64 syms = (u64)wsym & ((1ull << (2u * K)) - 1ull);
      packed_or(sa, r0, sa_bits, (syms << (ld_bits + t_bits)) | ((t_of_row + (K - 1u)) << ld_bits) | ld);
    }
  };
  for (u64 t = v >> 32;; --t) {
    if (K == 0 && sa != nullptr) packed_or(sa, p, sa_bits, (t << ld_bits) | ld);
    u64 q;
    const u32 c = lf_row<WIDE>(f, C, p, &q);  // the symbol at offset t - 1; rank 0 exactly when t == 0
    insert(p, c, true, t);
    if (t == 0) break;
    if (trow) packed_or(trow, t - 1, 2u, (u64)((c - 1u) & 3u));  // offset t - 1 at bits 2 (t - 1) .. of the stretch's own (zeroed) row
    p = q;
  }
  // the rows whose K symbols run past the read's first base: rank 0 from there on (t counts on below zero for the formula)
  for (u32 i = 1; i < K; ++i) insert(0, 0, false, 0ull - i);
}

// -------------------------------------------------------------------------------------------------------
// Start table of the block finder (fm_layout.h): one lane per 12-mer walks IntervalPair::init + eleven updateL steps
// (src/overlap_builder.cpp:91-122) with `prim` as the primary index.
// -------------------------------------------------------------------------------------------------------
template <bool WIDE>
__global__ __launch_bounds__(256) void k_start_build(FmStrand prim, FmStrand other, void* tab) {
  typedef typename PosOf<WIDE>::type P;
  const u32 code = blockIdx.x * 256 + threadIdx.x;
  if (code >= (1u << (2 * SIGAX_START_K))) return;
  const FmRef f = fm_ref(prim, 0);
  u32 r = 1u + ((code >> (2 * (SIGAX_START_K - 1))) & 3u);
  P lo0 = (P)prim.C[r], sz = (P)prim.total[r], lo1 = (P)other.C[r];
  u32 s = 1;
  for (int i = 1; i < SIGAX_START_K && sz != 0; ++i, ++s) {
    r = 1u + ((code >> (2 * (SIGAX_START_K - 1 - i))) & 3u);
    const u64 n = prim.n;
    const u64 pl = (u64)lo0 > n ? n : (u64)lo0, pu0 = (u64)(P)(lo0 + sz), pu = pu0 > n ? n : pu0;
    const Cnt4P<P> l = fm_rank4p<WIDE>(f, (P)pl), u = fm_rank4p<WIDE>(f, (P)pu);
    const P da = u.a - l.a, dc = u.c - l.c, dg = u.g - l.g, dt = u.t - l.t;
    const P dd = sz - (da + dc + dg + dt);
    const P acc = r == 1 ? dd : r == 2 ? dd + da : r == 3 ? dd + da + dc : dd + da + dc + dg;
    const P lc = r == 1 ? l.a : r == 2 ? l.c : r == 3 ? l.g : l.t;
    const P dcur = r == 1 ? da : r == 2 ? dc : r == 3 ? dg : dt;
    lo1 += acc;
    lo0 = (P)prim.C[r] + lc;
    sz = dcur;
  }
  if (WIDE) {
    ulonglong2* q = reinterpret_cast<ulonglong2*>(tab) + 2ull * code;
    q[0] = make_ulonglong2((u64)lo0, (u64)lo1);
    q[1] = make_ulonglong2((u64)sz, (u64)s);
  } else {
    reinterpret_cast<uint4*>(tab)[code] = make_uint4((u32)lo0, (u32)lo1, (u32)sz, s);
  }
}

// -------------------------------------------------------------------------------------------------------
// Deep start table of the block finder (fm_layout.h): the distinct K-mers of a strand's text are the runs of equal
// K-symbol prefixes among adjacent rows of its row table (k_deep_scan counts them, then lists each run's first row); one
// lane per distinct K-mer then walks IntervalPair::init + K - 1 updateL steps (src/overlap_builder.cpp:91-122) with that
// strand as primary index -- the arithmetic of k_start_build and of the finder itself -- and puts the state into the hash
// table (k_deep_fill).  The walk must come out at the run's own first row: anything else (an index whose rows are not in
// suffix order, a row table of a walk that did not end) raises *err and the host throws the table away.
// -------------------------------------------------------------------------------------------------------
// the first K symbols of the suffix at row p in text order, symbol j at bits 2 j of f0 (j < 28) / 2 (j - 28) of f1; false
// when the row's stretch ends before that
__device__ __forceinline__ bool deep_row_kmer(const FmStrand& st, const u32* slen, u64 n_stretch, u64 p, u32 K, u64& f0, u64& f1) {
  u32 ld, t;
  row_lookup(st, p, ld, t);
  f0 = f1 = 0;
  if ((u64)ld >= n_stretch) return false;
  if ((u64)t + K > (u64)slen[ld]) return false;
  const u64 m56 = (1ull << 56) - 1ull;
  f0 = text_bits(st, ld, t) & (K >= 28u ? m56 : ((1ull << (2u * K)) - 1ull));
  if (K > 28u) f1 = text_bits(st, ld, t + 28u) & (K >= 56u ? m56 : ((1ull << (2u * (K - 28u))) - 1ull));
  return true;
}
__global__ __launch_bounds__(256) void k_deep_scan(FmStrand st, const u32* slen, u64 n_stretch, u32 K, u64* count, u64* list, u64 list_cap) {
  const u32 lane = threadIdx.x & 63u;
  // waves walk the rows in strides of the grid (a launch holds fewer than 2^32 threads; BASELINE configs[4] has 1.3e10 rows)
  for (u64 p0 = (u64)blockIdx.x * 256; p0 < st.n; p0 += (u64)gridDim.x * 256) {
    const u64 p = p0 + threadIdx.x;
    u64 f0 = 0, f1 = 0;
    bool v = false;
    if (p < st.n) v = deep_row_kmer(st, slen, n_stretch, p, K, f0, f1);
    // the row before: the lane below has it, except for the wave's first lane
    u64 g0 = __shfl_up(f0, 1, 64), g1 = __shfl_up(f1, 1, 64);
    bool pv = __shfl_up((int)v, 1, 64) != 0;
    if (lane == 0) {
      pv = false;
      if (p > 0 && p < st.n) pv = deep_row_kmer(st, slen, n_stretch, p - 1, K, g0, g1);
    }
    const bool first = v && (!pv || g0 != f0 || g1 != f1);
    const u64 m = __ballot(first);
    if (!m) continue;
    u64 base = 0;
    if (lane == 0) base = atomicAdd(count, (u64)__popcll(m));
    base = __shfl(base, 0, 64);
    if (list != nullptr && first) {
      const u64 i = base + (u32)__popcll(m & ((1ull << lane) - 1ull));
      if (i < list_cap) list[i] = p;
    }
  }
}
template <bool WIDE>
__global__ __launch_bounds__(256) void k_deep_fill(FmStrand prim, FmStrand other, const u32* slen, u64 n_stretch, u32 K, const u64* list, u64 n_list,
                                                   u64* tab, u64 nslots, u64* err) {
  typedef typename PosOf<WIDE>::type P;
  const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;  // (fewer than 2^32 distinct K-mers: the host checks)
  if (i >= n_list) return;
  const u64 p = list[i];
  u64 f0, f1;
  if (!deep_row_kmer(prim, slen, n_stretch, p, K, f0, f1)) {
    atomicAdd(err, 1ull);
    return;
  }
  auto sym = [&](u32 j) -> u32 { return (u32)((j < 28u ? f0 >> (2u * j) : f1 >> (2u * (j - 28u))) & 3ull); };
  const FmRef f = fm_ref(prim, 0);
  // the chain consumes the K-mer from its last symbol backwards
  u32 r = 1u + sym(K - 1u);
  P lo0 = (P)prim.C[r], sz = (P)prim.total[r], lo1 = (P)other.C[r];
  u64 k0 = (u64)(r - 1u), k1 = 0;
  for (u32 c = 1; c < K; ++c) {
    r = 1u + sym(K - 1u - c);
    if (c < 32u) k0 |= (u64)(r - 1u) << (2u * c);
    else k1 |= (u64)(r - 1u) << (2u * (c - 32u));
    if (sz == 0) continue;
    const u64 n = prim.n;
    const u64 pl = (u64)lo0 > n ? n : (u64)lo0, pu0 = (u64)(P)(lo0 + sz), pu = pu0 > n ? n : pu0;
    const Cnt4P<P> l = fm_rank4p<WIDE>(f, (P)pl), u = fm_rank4p<WIDE>(f, (P)pu);
    const P da = u.a - l.a, dc = u.c - l.c, dg = u.g - l.g, dt = u.t - l.t;
    const P dd = sz - (da + dc + dg + dt);
    const P acc = r == 1 ? dd : r == 2 ? dd + da : r == 3 ? dd + da + dc : dd + da + dc + dg;
    const P lc = r == 1 ? l.a : r == 2 ? l.c : r == 3 ? l.g : l.t;
    const P dcur = r == 1 ? da : r == 2 ? dc : r == 3 ? dg : dt;
    lo1 += acc;
    lo0 = (P)prim.C[r] + lc;
    sz = dcur;
  }
  if (sz == 0 || (u64)lo0 != p || (WIDE && (((u64)lo0 | (u64)lo1 | (u64)sz) >> 40) != 0)) {
    atomicAdd(err, 1ull);
    return;
  }
  k1 |= (u64)(0x8000u | K) << 48;
  u64 slot = deep_slot(k0, k1, nslots);
  for (u64 tries = 0; tries < nslots; ++tries) {
    if (atomicCAS(&tab[slot * 4 + 1], 0ull, k1) == 0ull) {
      tab[slot * 4] = k0;
      if (WIDE) {
        tab[slot * 4 + 2] = (u64)lo0 | ((u64)lo1 << 40);
        tab[slot * 4 + 3] = ((u64)lo1 >> 24) | ((u64)sz << 16);
      } else {
        tab[slot * 4 + 2] = (u64)(u32)lo0 | ((u64)(u32)lo1 << 32);
        tab[slot * 4 + 3] = (u64)(u32)sz;
      }
      return;
    }
    slot = slot + 1 == nslots ? 0 : slot + 1;
  }
  atomicAdd(err, 1ull);
}

// ---- two-step table (fm_layout.h) -------------------------------------------------------------------------------
// built on the device from the one-step granules: one wave per 64 rows
template <bool WIDE>
__global__ __launch_bounds__(256) void k_build2_a(FmStrand s, u32* gran2, u32* cnt, u64 ng2) {
  const FmRef F = fm_ref(s, 0);
  const u32 lane = threadIdx.x & 63u;
  const u64 wave = ((u64)blockIdx.x * 256 + threadIdx.x) >> 6, nw = (u64)gridDim.x * 4;
  for (u64 g = wave; g < ng2; g += nw) {
    const u64 p = g * 64 + lane;
    u32 c1 = 0, c2 = 0;
    if (p < s.n) {
      c1 = fm_char(F, p);
      if (c1 >= 1 && c1 <= 4) {
        const Cnt4 k = fm_rank<WIDE>(F, p);
        const u64 rk = c1 == 1 ? k.a : c1 == 2 ? k.c : c1 == 3 ? k.g : k.t;
        c2 = fm_char(F, s.C[c1] + rk);  // BWT[LF(p)]
      } else {
        c1 = c1 > 4 ? 0 : c1;
      }
    }
    const u64 y1 = __ballot((c1 & 1u) != 0), z1 = __ballot((c1 & 2u) != 0), w1 = __ballot((c1 & 4u) != 0);
    const u64 y2 = __ballot((c2 & 1u) != 0), z2 = __ballot((c2 & 2u) != 0), w2 = __ballot((c2 & 4u) != 0);
    u32 mine = 0;  // lane t < 20 ends up with the granule's count for header word t
    for (u32 b = 1; b <= 4; ++b) {
      const u32 v = (u32)__popcll(__ballot(c1 == b));
      if (lane == b - 1) mine = v;
    }
    for (u32 c = 1; c <= 4; ++c)
      for (u32 x = 1; x <= 4; ++x) {
        const u32 v = (u32)__popcll(__ballot(c1 == c && c2 == x));
        if (lane == 4 + (c - 1) * 4 + (x - 1)) mine = v;
      }
    if (lane < 20) cnt[(u64)lane * ng2 + g] = mine;
    if (lane == 0) {
      u32* q = gran2 + g * SIGAX_GRAN2_WORDS + 20;
      q[0] = (u32)y1; q[1] = (u32)(y1 >> 32); q[2] = (u32)z1; q[3] = (u32)(z1 >> 32); q[4] = (u32)w1; q[5] = (u32)(w1 >> 32);
      q[6] = (u32)y2; q[7] = (u32)(y2 >> 32); q[8] = (u32)z2; q[9] = (u32)(z2 >> 32); q[10] = (u32)w2; q[11] = (u32)(w2 >> 32);
    }
  }
}
// counter `col` of every line; with 64-bit positions relative to the line's superblock, whose base goes to super2
__global__ __launch_bounds__(256) void k_build2_b(const u64* offs, u32* gran2, u32 col, u64 ng2, u64* super2) {
  const u64 g = (u64)blockIdx.x * 256 + threadIdx.x;
  if (g >= ng2) return;
  u64 base = 0;
  if (super2) {
    const u32 sh = SIGAX_SUPER_SHIFT - 6;  // lines per superblock = 2^sh
    const u64 first = (g >> sh) << sh;
    base = offs[first];
    if (g == first) super2[(g >> sh) * 20 + col] = base;
  }
  gran2[g * SIGAX_GRAN2_WORDS + col] = (u32)(offs[g] - base);
}

// -------------------------------------------------------------------------------------------------------
// launch wrappers
// -------------------------------------------------------------------------------------------------------
void launch_occ_batch(const FmStrand& s, bool wide, const u64* pos, u64 n, u64* out, hipStream_t st) {
  if (n == 0) return;
  if (wide) hipLaunchKernelGGL(k_occ_batch<true>, dim3(nblk(n, 256)), dim3(256), 0, st, s, pos, n, out);
  else hipLaunchKernelGGL(k_occ_batch<false>, dim3(nblk(n, 256)), dim3(256), 0, st, s, pos, n, out);
}

void launch_kmer_count(const FmStrand& s, bool wide, const unsigned char* kmers, u32 k, u64 n, u64* out, hipStream_t st) {
  if (n == 0) return;
  if (wide) hipLaunchKernelGGL(k_kmer_count<true>, dim3(nblk(n, 256)), dim3(256), 0, st, s, kmers, k, n, out);
  else hipLaunchKernelGGL(k_kmer_count<false>, dim3(nblk(n, 256)), dim3(256), 0, st, s, kmers, k, n, out);
}

unsigned long long start_table_bytes(bool wide) { return (1ull << (2 * SIGAX_START_K)) * (wide ? 32u : 16u); }
void launch_start_build(const FmStrand& prim, const FmStrand& other, bool wide, void* tab, hipStream_t st) {
  const unsigned g = (1u << (2 * SIGAX_START_K)) / 256u;
  if (wide) hipLaunchKernelGGL(k_start_build<true>, dim3(g), dim3(256), 0, st, prim, other, tab);
  else hipLaunchKernelGGL(k_start_build<false>, dim3(g), dim3(256), 0, st, prim, other, tab);
}

unsigned long long deep_entry_bytes() { return 32; }
void launch_deep_scan(const FmStrand& s, const u32* slen, u64 n_stretch, u32 K, u64* count, u64* list, u64 list_cap, hipStream_t st) {
  if (s.n == 0) return;
  hipLaunchKernelGGL(k_deep_scan, dim3((unsigned)std::min<u64>((s.n + 255) / 256, 1u << 22)), dim3(256), 0, st, s, slen, n_stretch, K, count, list, list_cap);
}
void launch_deep_fill(const FmStrand& prim, const FmStrand& other, bool wide, const u32* slen, u64 n_stretch, u32 K, const u64* list, u64 n_list,
                      void* tab, u64 nslots, u64* err, hipStream_t st) {
  if (n_list == 0) return;
  if (wide) hipLaunchKernelGGL(k_deep_fill<true>, dim3(nblk(n_list, 256)), dim3(256), 0, st, prim, other, slen, n_stretch, K, list, n_list, (u64*)tab, nslots, err);
  else hipLaunchKernelGGL(k_deep_fill<false>, dim3(nblk(n_list, 256)), dim3(256), 0, st, prim, other, slen, n_stretch, K, list, n_list, (u64*)tab, nslots, err);
}
void launch_suffix_order_check(const FmStrand& s, const u32* sai, u32* isai_tmp, const u32* read_len, u64 n_strings, u64* bad3, hipStream_t st) {
  if (n_strings == 0 || s.n < 2) return;
  hipLaunchKernelGGL(k_isai, dim3(nblk(n_strings, 256)), dim3(256), 0, st, sai, n_strings, isai_tmp);
  hipLaunchKernelGGL(k_suffix_order_check, dim3(nblk(s.n - 1, 256)), dim3(256), 0, st, s, sai, (const u32*)isai_tmp, read_len, n_strings, bad3);
}

void launch_build2(const FmStrand& s, bool wide, u32* gran2, u64* super2, u32* cnt, u64* offs, u64* partial, u64* total, hipStream_t st) {
  const u64 ng2 = s.n / SIGAX_GRAN2_SYMS + 1;
  const unsigned g = (unsigned)std::min<u64>(nblk(ng2, 4), 65536);
  if (wide) hipLaunchKernelGGL(k_build2_a<true>, dim3(g), dim3(256), 0, st, s, gran2, cnt, ng2);
  else hipLaunchKernelGGL(k_build2_a<false>, dim3(g), dim3(256), 0, st, s, gran2, cnt, ng2);
  for (u32 col = 0; col < 20; ++col) {
    launch_scan(cnt + (u64)col * ng2, ng2, partial, offs, total, st);  // sigax_tail.hip
    hipLaunchKernelGGL(k_build2_b, dim3(nblk(ng2, 256)), dim3(256), 0, st, (const u64*)offs, gran2, col, ng2, wide ? super2 : (u64*)nullptr);
  }
}

void launch_stretch_scan(const FmStrand& s, bool wide, u64 n_stretch, u64* info, u32* maxlen, hipStream_t st) {
  if (n_stretch == 0) return;
  if (wide) hipLaunchKernelGGL(k_stretch_scan<true>, dim3(nblk(n_stretch, 256)), dim3(256), 0, st, s, n_stretch, info, maxlen);
  else hipLaunchKernelGGL(k_stretch_scan<false>, dim3(nblk(n_stretch, 256)), dim3(256), 0, st, s, n_stretch, info, maxlen);
}
void launch_rows_fill(const FmStrand& s, bool wide, u64 n_stretch, const u64* info, unsigned char* sa, u32 sa_bits, u32 ld_bits, u32 t_bits,
                      unsigned char* text, u32 text_stride, u32* slen, hipStream_t st) {
  if (n_stretch == 0) return;
  if (wide) hipLaunchKernelGGL(k_rows_fill<true>, dim3(nblk(n_stretch, 256)), dim3(256), 0, st, s, n_stretch, info, sa, sa_bits, ld_bits, t_bits, text, text_stride, slen);
  else hipLaunchKernelGGL(k_rows_fill<false>, dim3(nblk(n_stretch, 256)), dim3(256), 0, st, s, n_stretch, info, sa, sa_bits, ld_bits, t_bits, text, text_stride, slen);
}
void launch_xmap(const u32* sai_y, const u32* sai_x, u32* isai_tmp, const u32* slen_x, u64 n, u64* xmap, hipStream_t st) {
  if (n == 0) return;
  hipLaunchKernelGGL(k_isai, dim3(nblk(n, 256)), dim3(256), 0, st, sai_x, n, isai_tmp);
  hipLaunchKernelGGL(k_xmap, dim3(nblk(n, 256)), dim3(256), 0, st, sai_y, (const u32*)isai_tmp, slen_x, n, xmap);
}
