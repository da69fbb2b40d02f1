// siga_amd/csrc/sigax_mmoverlap.hip -- `siga overlap -e` on the device (gfx950 / CDNA4, wave64): every indexed read is lined up,
// without gaps, against the indexed reads that share a seed with it, and the alignments with few enough mismatches are kept as
// edge records and containment flags (rules: include/sigax.h).  No counterpart in the reference, whose overlap finder is exact
// (OverlapBlockFinder, src/overlap_builder.cpp:838-912).
//
//   k_mmo          one wave per read: the distinct candidates of its hits, each verified, what is accepted left in the read's own
//                  stretch of the hit list
//   k_mmo_commit   one wave per read: when the call's records fit, they go behind the cursor and the flags are set; with
//                  SIGAX_MMO_CONTAINMENTS every flag gives a containment record behind the read's dovetail records
//   k_mmo_status   the eight status words, and the cursor moved
//   k_mmo_keys, k_mmo_keys2, k_mmo_gather, k_mmo_compact   the finish: two stable radix passes, repeats dropped
//
// The pieces k_mmo shares with k_pile (the table of candidate keys: cand_collect, cand_slot, cand_decode, cand_code; seed_span,
// seed_flags) are sigax_seeded.h's.
//
// Shape of k_mmo.  A workgroup is one wave.  (1) As k_pile: the read's hits are taken 64 at a time, one per lane, and go as keys
// {read, diagonal, strand} into an open-addressed table in dynamic LDS with a 64-bit compare-and-swap, which makes the triples
// distinct; more than K ends the read.  (2) The read's own codes are held in registers, 2 bits a column: lane l has the columns
// 64 c + l in two u64.  The table is swept 64 slots at a time; the lanes load offsets and name rank of their own slot's read, so
// the 64 loads are in flight together, then every occupied slot is taken by the whole wave in turn: lane l faces column 64 c + l
// of the query for the c that touch [x0, x1), so the candidate's bases are read as 64 neighbouring bytes a step, backwards for
// the reverse strand, and the mismatches are summed over the wave.  (3) What a sweep accepts is collected one result a lane and
// written by neighbouring lanes, 16 bytes each, over the read's own hits, which nobody reads any more: records from the front of
// the stretch, read ids to flag from its back.  A candidate gives at most one of the two and comes from at least one hit, so they
// fit.  A flag's 16 bytes hold its whole containment record {contained, container, o, af | num_diff << 8 | len << 19}, whether
// or not the call asks for it: o in full width, since a container may be longer than any query (rule 1 stops it as a query, not
// as a candidate); the contained read is a query or lies within one, so len <= 4096 takes 13 bits, and num_diff <= len / 4 takes
// 11.  No atomic is taken on the record cursor: the call's records are counted per read and scanned, and k_mmo_commit writes them
// only if all of them fit -- the rule that an overflowing call writes nothing needs the count before the first write.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include "sigax_rank.h"
#include "sigax_mmoverlap.h"

namespace {

__global__ __launch_bounds__(64) void k_mmo(MmoArgs A) {
  extern __shared__ __align__(16) unsigned char mmo_lds[];
  u64* tab = reinterpret_cast<u64*>(mmo_lds);  // [tab_cap]: candidate keys

  const u32 lane = threadIdx.x;
  const u64 r = blockIdx.x;
  const u64 total_hits = A.L.loc_status[0];
  if (total_hits > A.L.hits_cap) return;  // the caller's hits did not fit: nothing is written (sigax.h)

  const u32 S = A.p.seed_length, T = A.p.seed_stride;
  const u64 i = A.first_read + r;  // below n_ref (the host checks the range)
  const u64 b0 = A.R.ref_offs[i], n64 = A.R.ref_offs[i + 1] - b0;
  const unsigned char* q = A.R.ref_text + b0;

  // ---- rule 1 ----
  if (n64 < S || n64 > A.p.max_read_len) {
    if (lane == 0) atomicAdd(&A.counters[MMO_C_LENGTH], 1ull);
    return;
  }
  const u32 n = (u32)n64;  // <= max_read_len <= 4096
  const u32 rank_q = A.name_rank[i];

  // the read's codes: lane l holds the columns 64 c + l, c < 32 in q0 and the others in q1
  u64 q0 = 0, q1 = 0;
  for (u32 c = 0; c * 64u < n; ++c) {
    const u32 x = c * 64u + lane;
    if (x < n) {
      const u64 code = (u64)((base_rank(q[x]) - 1u) & 3u);  // the reference text holds ACGT only
      if (c < 32u) q0 |= code << (2u * c);
      else q1 |= code << (2u * (c - 32u));
    }
  }
  for (u32 s = lane; s < A.tab_cap; s += 64) tab[s] = CAND_EMPTY;
  __syncthreads();

  // ---- rule 2: the seeds' flags, and the hits into the table of distinct triples ----
  const SeedSpan sp = seed_span(A.L, r, total_hits);
  u32 located, repeats;
  seed_flags(A.L, sp, lane, located, repeats);
  const bool over = cand_collect(tab, A.tab_cap, A.L, sp, A.R, n, S, T, A.p.max_candidates, lane);
  wave_add(&A.counters[MMO_C_LOCATED], (u64)located);
  wave_add(&A.counters[MMO_C_REPEATS], (u64)repeats);
  if (over) {
    if (lane == 0) atomicAdd(&A.counters[MMO_C_OVER], 1ull);
    return;
  }
  __syncthreads();

  // ---- rules 3-7: every candidate once, lanes across the query's columns ----
  const u64 room = sp.h1 - sp.h0;  // results fit: a candidate gives at most one and comes from at least one hit
  u32 tested = 0, taken = 0, n_rec = 0, n_flag = 0;
  for (u32 base = 0; base < A.tab_cap; base += 64) {
    u64 key, rb;
    u32 len_t, rank_t = 0;
    const bool has = cand_slot(tab, base + lane, A.R, key, rb, len_t, [&](u64 t) { rank_t = A.name_rank[t]; });
    u64 mask = __ballot(has && rank_t != rank_q);  // rule 3
    uint4 my_rec = make_uint4(0, 0, 0, 0), my_flag = make_uint4(0, 0, 0, 0);
    u32 s_rec = 0, s_flag = 0;  // this sweep's results: the k-th of a kind with lane k
    while (mask) {
      const int src = __ffsll((long long)mask) - 1;
      mask &= mask - 1ull;
      const SeedCand k = cand_decode(key, rb, len_t, src, n);
      const u32 crank = (u32)__shfl((int)rank_t, src, 64), t = k.t;
      const bool rev = k.rev;
      const long long d = k.d, x0 = k.x0, x1 = k.x1, clen = k.clen;
      if (x1 <= x0) continue;  // (a hit's window lies in both texts: there is an overlap)
      const u32 ell = (u32)(x1 - x0);
      tested += 1u;
      if (ell < A.p.min_overlap) continue;
      const unsigned char* text = A.R.ref_text + k.rb;
      u32 mism = 0;
      for (u32 c = (u32)x0 >> 6; c <= ((u32)x1 - 1u) >> 6; ++c) {  // x0 < x1 <= n <= 4096
        const long long x = (long long)(c * 64u + lane);
        if (x >= x0 && x < x1) {
          const long long pos = x + d;  // in [0, clen)
          const u32 code = cand_code(text, clen, pos, rev);
          const u32 mine = (u32)((c < 32u ? q0 >> (2u * c) : q1 >> (2u * (c - 32u))) & 3ull);
          mism += code != mine ? 1u : 0u;
        }
      }
      const u32 m = (u32)wave_sum((u64)mism);
      if ((u64)m > ((u64)ell * A.p.error_permille) / 1000ull) continue;
      taken += 1u;
      // rules 5-7, the same in every lane
      const bool q_in = ell == n, t_in = (long long)ell == clen;
      if (q_in || t_in) {
        // the contained read is the query (for DUP: the larger name rank) or the candidate; o = the first column of the
        // container's forward text that it covers: d (reverse: L - d - n) for the query, -d for the candidate
        const bool q_is = (q_in && t_in) ? rank_q > crank : q_in;
        const u32 o = q_is ? (u32)(rev ? clen - d - (long long)n : d) : (u32)(-d);
        const u32 af = SIGAX_MM_CONTAINMENT | (rev ? 4u : 0u);
        const u32 packed = af | (m << 8) | ((q_is ? n : ell) << 19);  // m <= 1024, the contained read's length <= 4096
        const uint4 flag = q_is ? make_uint4((u32)i, t, o, packed) : make_uint4(t, (u32)i, o, packed);
        if (lane == s_flag) my_flag = flag;
        s_flag += 1u;
      } else {
        u32 af = d < 0 ? (rev ? 6u : 0u) : (rev ? 5u : 3u);
        uint4 rec;
        if (rank_q > crank) {
          rec = make_uint4((u32)i, t, ell, af | (m << 8));
        } else {
          af = (af & 4u) ? af : af ^ 3u;
          rec = make_uint4(t, (u32)i, ell, af | (m << 8));
        }
        if (lane == s_rec) my_rec = rec;
        s_rec += 1u;
      }
    }
    if (lane < s_rec && (u64)(n_rec + lane) < room) A.L.hits[sp.h0 + n_rec + lane] = my_rec;
    if (lane < s_flag && (u64)(n_flag + lane) < room) A.L.hits[sp.h1 - 1 - (n_flag + lane)] = my_flag;
    n_rec += s_rec;
    n_flag += s_flag;
  }
  if (lane == 0) {
    A.n_rec[r] = n_rec + ((A.p.flags & SIGAX_MMO_CONTAINMENTS) ? n_flag : 0u);  // the records the commit writes for this read
    A.n_flag[r] = n_flag;
    if (tested) atomicAdd(&A.counters[MMO_C_TESTED], (u64)tested);
    if (taken) atomicAdd(&A.counters[MMO_C_ACCEPTED], (u64)taken);
  }
}

// whether the call goes through: the hits were listed and the records fit behind the cursor
__device__ __forceinline__ bool mmo_fits(const MmoArgs& A, u64* cursor0) {
  const u64 c = *A.cursor;
  *cursor0 = c;
  return A.L.loc_status[0] <= A.L.hits_cap && c <= A.edges_cap && *A.rec_total <= A.edges_cap - c;
}

__global__ __launch_bounds__(256) void k_mmo_commit(MmoArgs A) {
  const u32 lane = threadIdx.x & 63u;
  const u64 r = (u64)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= A.n_reads) return;
  u64 cursor0;
  if (!mmo_fits(A, &cursor0)) return;
  const SeedSpan sp = seed_span(A.L, r, A.L.loc_status[0]);
  const u64 room = sp.h1 - sp.h0;
  const bool conts = (A.p.flags & SIGAX_MMO_CONTAINMENTS) != 0;
  u64 n_rec = A.n_rec[r], n_flag = A.n_flag[r];
  if (conts) n_rec = n_rec >= n_flag ? n_rec - n_flag : 0;  // the dovetail records alone
  n_rec = n_rec < room ? n_rec : room;
  n_flag = n_flag < room - n_rec ? n_flag : room - n_rec;
  const u64 out0 = cursor0 + A.rec_offs[r];
  for (u64 k = lane; k < n_rec; k += 64) {
    const uint4 v = A.L.hits[sp.h0 + k];
    sigax_mm_edge e;
    e.query = v.x;
    e.target = v.y;
    e.length = v.z;
    e.af = v.w & 0xFFu;
    e.num_diff = v.w >> 8;
    e.reserved = 0;
    if (out0 + k < A.edges_cap) A.edges[out0 + k] = e;  // (it is: the total fits)
  }
  for (u64 k = lane; k < n_flag; k += 64) {
    const uint4 v = A.L.hits[sp.h1 - 1 - k];
    if ((u64)v.x < A.R.n_ref) A.contained[v.x] = 1;
    if (conts) {
      sigax_mm_edge e;
      e.query = v.x;
      e.target = v.y;
      e.length = v.w >> 19;
      e.af = v.w & 0xFFu;
      e.num_diff = (v.w >> 8) & 0x7FFu;
      e.reserved = v.z;
      if (out0 + n_rec + k < A.edges_cap) A.edges[out0 + n_rec + k] = e;  // (it is: the total fits)
    }
  }
}

__global__ void k_mmo_status(MmoArgs A) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const u64 hits = A.L.loc_status[0];
  const bool listed = hits <= A.L.hits_cap;
  u64 cursor0;
  const bool fits = mmo_fits(A, &cursor0);
  A.status[0] = hits;
  A.status[1] = listed ? A.counters[MMO_C_LENGTH] : 0ull;
  A.status[2] = listed ? A.counters[MMO_C_OVER] : 0ull;
  A.status[3] = listed ? A.counters[MMO_C_LOCATED] : 0ull;
  A.status[4] = listed ? A.counters[MMO_C_REPEATS] : 0ull;
  A.status[5] = listed ? A.counters[MMO_C_TESTED] : 0ull;
  A.status[6] = listed ? A.counters[MMO_C_ACCEPTED] : 0ull;
  A.status[7] = listed ? *A.rec_total : 0ull;
  if (fits) *A.cursor = cursor0 + *A.rec_total;
}

// ---- finish ----
__global__ __launch_bounds__(256) void k_mmo_keys(MmoFinishArgs A) {
  const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
  if (i >= A.n) return;
  const sigax_mm_edge e = A.edges[i];
  A.keys[0][i] = ((u64)(e.af & 15u) << 45) | ((u64)(e.length & 0x1FFFu) << 32) | (u64)e.reserved;
  A.vals[0][i] = i;
}

// the first pass has left the records' places in (af, length, reserved) order in vals[1]: their (query, target) in that order
__global__ __launch_bounds__(256) void k_mmo_keys2(MmoFinishArgs A) {
  const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
  if (i >= A.n) return;
  const u64 at = A.vals[1][i];
  u64 key = 0;
  if (at < A.n) {
    const sigax_mm_edge e = A.edges[at];
    key = ((u64)e.query << 32) | (u64)e.target;
  }
  A.keys[0][i] = key;
}

__device__ __forceinline__ bool mmo_same(const sigax_mm_edge& a, const sigax_mm_edge& b) {
  return a.query == b.query && a.target == b.target && a.af == b.af && a.length == b.length && a.reserved == b.reserved;
}

// the second pass has left the places in full order in vals[0]: the records in that order, and which of them open a run
__global__ __launch_bounds__(256) void k_mmo_gather(MmoFinishArgs A) {
  const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
  if (i >= A.n) return;
  const u64 at = A.vals[0][i], before = i ? A.vals[0][i - 1] : 0;
  if (at >= A.n || before >= A.n) {  // (not after a sort of 0 .. n - 1)
    A.head[i] = 0;
    return;
  }
  const sigax_mm_edge e = A.edges[at];
  A.sorted[i] = e;
  A.head[i] = (i == 0 || !mmo_same(e, A.edges[before])) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_mmo_compact(MmoFinishArgs A) {
  const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
  if (i == 0) *A.n_unique = A.scan[A.n];
  if (i >= A.n || !A.head[i]) return;
  const u64 to = A.scan[i];
  if (to < A.n) A.edges[to] = A.sorted[i];
}

}  // namespace

uint32_t mmo_lds_bytes(uint32_t tab_cap) { return tab_cap * 8u; }

int launch_mmo(const MmoArgs& a, hipStream_t st) { return launch_wave_lds(k_mmo, a, a.n_reads, mmo_lds_bytes(a.tab_cap), st); }

void launch_mmo_commit(const MmoArgs& a, hipStream_t st) {
  if (a.n_reads) hipLaunchKernelGGL(k_mmo_commit, dim3((unsigned)((a.n_reads + 3) / 4)), dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_mmo_status, dim3(1), dim3(64), 0, st, a);
}

hipError_t mmo_sort_bytes(unsigned long long n, unsigned long long* bytes) {
  size_t tb = 0;
  *bytes = 0;
  if (n == 0) return hipSuccess;
  const hipError_t e = rocprim::radix_sort_pairs(nullptr, tb, (const u64*)nullptr, (u64*)nullptr, (const u64*)nullptr, (u64*)nullptr, (size_t)n, 0u, 64u);
  *bytes = tb;
  return e;
}

hipError_t launch_mmo_finish(const MmoFinishArgs& a, hipStream_t st) {
  if (a.n == 0) return hipMemsetAsync(a.n_unique, 0, 8, st);
  const unsigned grid = blocks_of(a.n);
  size_t tb = (size_t)a.sort_tmp_bytes;
  hipLaunchKernelGGL(k_mmo_keys, dim3(grid), dim3(256), 0, st, a);
  // stable passes, the minor key first: (af, length, reserved) in 49 bits (4 + 13 + 32: an overlap has at most 4096 columns, a
  // containment's offset is as wide as its container is long), then
  // (query, target)
  hipError_t e = rocprim::radix_sort_pairs(a.sort_tmp, tb, (const u64*)a.keys[0], a.keys[1], (const u64*)a.vals[0], a.vals[1], (size_t)a.n, 0u, 49u, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_mmo_keys2, dim3(grid), dim3(256), 0, st, a);
  tb = (size_t)a.sort_tmp_bytes;
  e = rocprim::radix_sort_pairs(a.sort_tmp, tb, (const u64*)a.keys[0], a.keys[1], (const u64*)a.vals[1], a.vals[0], (size_t)a.n, 0u, 64u, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_mmo_gather, dim3(grid), dim3(256), 0, st, a);
  launch_scan(a.head, a.n, a.partial, a.scan, a.scan + a.n, st);
  hipLaunchKernelGGL(k_mmo_compact, dim3(grid), dim3(256), 0, st, a);
  return hipGetLastError();
}
