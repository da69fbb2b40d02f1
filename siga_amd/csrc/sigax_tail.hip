// siga_amd/csrc/sigax_tail.hip -- the tail of `siga overlap` behind filter/extract: scan, ordered copy, edge records, with
// their launch wrappers (sigax_kernels.h).
//
//   k_scan_*          exclusive scan of u32 counts into u64 offsets (launch_scan; launch_build2 of sigax_tables.hip uses it too)
//   k_order_scatter   ordered compaction of the per-read block lists (replaces the hits text round trip,
//                     src/overlap_builder.cpp:234-254,269-280)
//   k_edges_*         Hit2OverlapConverter::convert                          (src/overlap_builder.cpp:345-375)
//
// The candidate record a lane-group block points back to (Cand, cand_load) is sigax_fm.h's; the kernels that write it are in
// sigax_kernels.hip.
#include <hip/hip_runtime.h>

#include "sigax_kernels.h"
#include "sigax_fm.h"

// -------------------------------------------------------------------------------------------------------
// exclusive scan of u32 counts into u64 offsets (two small kernels), ordered scatter of the final blocks
// -------------------------------------------------------------------------------------------------------
#define SCAN_ITEMS 2048  // per workgroup of 256 threads

__device__ __forceinline__ u64 block_exclusive_scan(u64 v, u64* total) {
  __shared__ u64 wsum[4];
  u32 lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  u64 x = v;
  for (int off = 1; off < 64; off <<= 1) {
    u64 y = __shfl_up(x, off, 64);
    if (lane >= (u32)off) x += y;
  }
  if (lane == 63) wsum[wid] = x;
  __syncthreads();
  u64 base = 0;
  for (u32 w = 0; w < wid; ++w) base += wsum[w];
  u64 tot = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  __syncthreads();
  *total = tot;
  return base + x - v;
}

__global__ __launch_bounds__(256) void k_scan_partials(const u32* cnt, u64 n, u64* partial) {
  u64 base = (u64)blockIdx.x * SCAN_ITEMS + (u64)threadIdx.x * 8;
  u64 s = 0;
  for (int k = 0; k < 8; ++k)
    if (base + k < n) s += cnt[base + k];
  u64 tot;
  block_exclusive_scan(s, &tot);
  if (threadIdx.x == 0) partial[blockIdx.x] = tot;
}

// Each workgroup sums the totals of the workgroups before it itself (at most a few thousand u64 values, from L2) instead
// of waiting for a one-workgroup launch that scanned them.  even_out (or NULL): even_out[i] = offs[2i], i <= n / 2 -- the
// per-read offsets of a per-(read, side) scan (n even).
__global__ __launch_bounds__(256) void k_scan_apply(const u32* cnt, u64 n, const u64* partial, u64* offs, u64* total_out, u64* even_out) {
  u64 before = 0;
  for (u64 i = threadIdx.x; i < blockIdx.x; i += 256) before += partial[i];
  u64 carry;
  block_exclusive_scan(before, &carry);
  u64 base = (u64)blockIdx.x * SCAN_ITEMS + (u64)threadIdx.x * 8;
  u64 v[8], s = 0;
  for (int k = 0; k < 8; ++k) {
    v[k] = (base + k < n) ? cnt[base + k] : 0;
    s += v[k];
  }
  u64 tot;
  u64 ex = block_exclusive_scan(s, &tot) + carry;
  for (int k = 0; k < 8; ++k) {
    if (base + k < n) {
      offs[base + k] = ex;
      if (even_out != nullptr && !(k & 1)) even_out[(base + k) >> 1] = ex;  // base is a multiple of 8
    }
    ex += v[k];
  }
  if (base <= n && n < base + 8) {  // the thread owning position n writes the grand total
    offs[n] = ex;
    *total_out = ex;
    if (even_out != nullptr) even_out[n >> 1] = ex;
  }
}

// one lane per (read, side) item: copy its blocks from the unordered arena to their place in the ordered output; blocks
// written by the lane-group kernels get their raw pair, length and flags from the candidate record here
template <bool WIDE>
__device__ __forceinline__ void order_fill_from_cand(const OrderArgs& A, u64 item, u32 src, ulonglong2& v2, ulonglong2& v3, ulonglong2& v4) {
  const Cand<WIDE>* rec = reinterpret_cast<const Cand<WIDE>*>(A.arena) + (item >> 1) * 4 * A.cap + (src & 0x3FFFFFFFu);
  const Cand<WIDE> b = cand_load<WIDE>(rec);
  v2 = make_ulonglong2((u64)b.r0lo, (u64)b.r0lo + b.sz - 1);
  v3 = make_ulonglong2((u64)b.r1lo, (u64)b.r1lo + b.sz - 1);
  v4 = make_ulonglong2((u64)b.len | ((u64)b.af << 32), 0ull);
}
// Hit2OverlapConverter::convert's test for one (query, target) pair (src/overlap_builder.cpp:358,365); nq, lq: the query's
// name rank and length, which an item loads once for all its targets
__device__ __forceinline__ bool edge_kept(const uint32_t* name_rank, const uint32_t* read_len, u32 nq, u32 lq, u32 t, u32 len, u32 af) {
  u32 nt = name_rank[t];
  if (nq == nt) return false;                       // query.name != target.name (:358)
  bool contained = (len == lq) || (len == read_len[t]);  // Match::isContainment (coord.h:150-152)
  if (nq < nt || (contained && (af & 1u))) return false;              // dedup rule (:365)
  return true;
}
// The ordered copy: what a run without edge records ends with, and what a run with them does only when somebody asks for
// its blocks (sigax_batch_download, sigax_batch_device_outputs with d_blocks).  bad_ids (or NULL): out-of-range read ids
// are counted here in a run without edge records.
__global__ __launch_bounds__(256) void k_order_scatter(OrderArgs A) {
  u64 w = (u64)blockIdx.x * 256 + threadIdx.x;
  if (w >= A.n_items) return;
  u32 cnt = A.fin_cnt[w];
  if (A.read_ids != nullptr && A.bad_ids != nullptr && A.read_ids[w >> 1] >= A.n_index_reads) atomicAdd(A.bad_ids, 1ull);
  if (!cnt) return;
  u64 srcb = A.item_base[w], dstb = A.offs2[w];
  for (u32 i = 0; i < cnt; ++i) {
    if (srcb + i >= A.fin_cap || dstb + i >= A.out_cap) break;  // only after an overflow, whose results the host discards
    const ulonglong2* s = reinterpret_cast<const ulonglong2*>(A.fin + srcb + i);
    ulonglong2* d = reinterpret_cast<ulonglong2*>(A.out + dstb + i);
    ulonglong2 v0 = s[0], v1 = s[1], v4 = s[4];
    ulonglong2 v2, v3;
    if (v4.y >> 63) {
      if (A.wide) order_fill_from_cand<true>(A, w, (u32)v4.y, v2, v3, v4);
      else order_fill_from_cand<false>(A, w, (u32)v4.y, v2, v3, v4);
    } else {
      v2 = s[2]; v3 = s[3];
    }
    d[0] = v0; d[1] = v1; d[2] = v2; d[3] = v3; d[4] = v4;
  }
}

// -------------------------------------------------------------------------------------------------------
// edges: Hit2OverlapConverter::convert (overlap_builder.cpp:345-375) in two passes with the scan of the per-item counts
// between them, one lane per (read, side) item: its blocks are consecutive in the ordered output, its records consecutive
// in the edge list (hits order = the ED order at -t 1).  The ordered blocks themselves are not needed for it.
//   stage: reads each block where filter/extract left it (fin + item_base) -- its capped0 range, and length and flags from
//          the block or, for a lane-group block, from the half of its candidate record that holds them --, tests the
//          block's one target and leaves a 16-byte record at the block's ORDERED index (neighbouring items write
//          neighbouring records): the final sigax_edge, or EDGE_ST_DROPPED; a block whose range holds several targets
//          (duplicates, repeats, exhaustive mode) is counted by walking it and left as EDGE_ST_WALK
//   emit:  copies the staged records that were kept to their places and walks the EDGE_ST_WALK blocks again, from fin
// `af` of a record holds the three AlignFlags bits, so the two markers are no record's af.
// -------------------------------------------------------------------------------------------------------
static_assert(sizeof(sigax_edge) == 16, "a staged record is a sigax_edge");
#define EDGE_ST_DROPPED 0xFFFFFFFFu
#define EDGE_ST_WALK 0xFFFFFFFEu

// length | af << 32 of the block at fin[at]; v4 = its last 16 bytes
__device__ __forceinline__ u64 edge_len_af(const EdgeArgs& A, u64 item, const ulonglong2& v4) {
  if (!(v4.y >> 63)) return v4.x;
  const u64 rec = (item >> 1) * 4 * A.cap + ((u32)v4.y & 0x3FFFFFFFu);
  if (A.wide) return reinterpret_cast<const ulonglong2*>(reinterpret_cast<const Cand<true>*>(A.arena) + rec)[3].x;
  const uint4 h = reinterpret_cast<const uint4*>(reinterpret_cast<const Cand<false>*>(A.arena) + rec)[1];
  return (u64)h.z | ((u64)h.w << 32);
}

__global__ __launch_bounds__(256) void k_edges_stage(EdgeArgs A) {
  const u64 w = (u64)blockIdx.x * 256 + threadIdx.x;
  if (w >= A.n_items) return;
  const u32 cnt = A.fin_cnt[w];
  u32 kept = 0;
  u32 q = A.read_base + (u32)(w >> 1);
  bool known = true;  // the read is one of the index's
  if (A.read_ids != nullptr) {
    q = A.read_ids[w >> 1];
    known = q < A.n_index_reads;
    if (!known) atomicAdd(A.bad_ids, 1ull);
  }
  if (cnt && known) {
    const u64 srcb = A.item_base[w], dstb = A.offs2[w];
    const u32 nq = A.name_rank[q], lq = A.read_len[q];
    uint4* stage = reinterpret_cast<uint4*>(A.stage);
    for (u32 i = 0; i < cnt; ++i) {
      if (srcb + i >= A.fin_cap || dstb + i >= A.stage_cap) break;  // only after an overflow, whose results the host discards
      const ulonglong2* s = reinterpret_cast<const ulonglong2*>(A.fin + srcb + i);
      const ulonglong2 v0 = s[0], v4 = s[4];
      const u64 la = edge_len_af(A, w, v4);
      const u32 len = (u32)la, af = (u32)(la >> 32);
      const u32* sa = (af & 2u) ? A.rsai : A.sai;
      uint4 rec = make_uint4(q, 0u, len, EDGE_ST_DROPPED);
      if (v0.x == v0.y) {
        if (v0.x < A.n_sai) {
          rec.y = sa[v0.x];
          if (edge_kept(A.name_rank, A.read_len, nq, lq, rec.y, len, af)) {
            rec.w = af;
            ++kept;
          }
        }
      } else if (v0.x < v0.y) {
        rec.w = EDGE_ST_WALK;
        for (u64 j = v0.x; j <= v0.y && j < A.n_sai; ++j)
          if (edge_kept(A.name_rank, A.read_len, nq, lq, sa[j], len, af)) ++kept;
      }
      stage[dstb + i] = rec;
    }
  }
  A.item_edges[w] = kept;
}

__global__ __launch_bounds__(256) void k_edges_emit(EdgeArgs A) {
  const u64 w = (u64)blockIdx.x * 256 + threadIdx.x;
  if (w >= A.n_items) return;
  const u32 cnt = A.fin_cnt[w];
  if (!cnt) return;
  u64 e = A.edge_offs[w];
  const u64 e_end = A.edge_offs[w + 1];
  if (e_end == e) return;  // no record from this item (most items: the self-containment blocks)
  const u64 first = A.offs2[w];
  const uint4* stage = reinterpret_cast<const uint4*>(A.stage);
  uint4* edges = reinterpret_cast<uint4*>(A.edges);  // sigax_edge = (query, target, length, af)
  for (u32 i = 0; i < cnt && e < e_end; ++i) {
    if (first + i >= A.stage_cap) return;  // only after an overflow, whose results the host discards
    const uint4 rec = stage[first + i];
    if (rec.w == EDGE_ST_DROPPED) continue;
    if (rec.w != EDGE_ST_WALK) {
      if (e < A.edge_cap) edges[e] = rec;
      ++e;
      continue;
    }
    const u64 at = A.item_base[w] + i;
    if (at >= A.fin_cap) return;
    const ulonglong2* s = reinterpret_cast<const ulonglong2*>(A.fin + at);
    const ulonglong2 v0 = s[0], v4 = s[4];
    const u64 la = edge_len_af(A, w, v4);
    const u32 len = (u32)la, af = (u32)(la >> 32);
    const u32* sa = (af & 2u) ? A.rsai : A.sai;
    // (not rec.x: after an overflow the staged record may be a stale one)
    const u32 q = A.read_ids != nullptr ? A.read_ids[w >> 1] : A.read_base + (u32)(w >> 1);
    const u32 nq = A.name_rank[q], lq = A.read_len[q];
    for (u64 j = v0.x; j <= v0.y && j < A.n_sai; ++j) {
      const u32 t = sa[j];
      if (edge_kept(A.name_rank, A.read_len, nq, lq, t, len, af)) {
        if (e < A.edge_cap) edges[e] = make_uint4(q, t, len, af);
        ++e;
      }
    }
  }
}

// -------------------------------------------------------------------------------------------------------
// launch wrappers
// -------------------------------------------------------------------------------------------------------
void launch_scan(const u32* cnt, u64 n, u64* partial, u64* offs, u64* total_out, hipStream_t st, u64* even_out) {
  // offs has n+1 entries; offs[n] = total.  Two launches: per-workgroup totals, then the scan itself (k_scan_apply)
  unsigned g = nblk(n + 1, SCAN_ITEMS);
  hipLaunchKernelGGL(k_scan_partials, dim3(g), dim3(256), 0, st, cnt, n, partial);
  hipLaunchKernelGGL(k_scan_apply, dim3(g), dim3(256), 0, st, cnt, n, (const u64*)partial, offs, total_out, even_out);
}

u64 scan_partials_needed(u64 n) { return (n + 1 + SCAN_ITEMS - 1) / SCAN_ITEMS + 1; }

void launch_order_scatter(const OrderArgs& a, hipStream_t st) {
  if (a.n_items == 0) return;
  hipLaunchKernelGGL(k_order_scatter, dim3(nblk(a.n_items, 256)), dim3(256), 0, st, a);
}

void launch_edges_stage(const EdgeArgs& a, hipStream_t st) {
  if (a.n_items == 0) return;
  hipLaunchKernelGGL(k_edges_stage, dim3(nblk(a.n_items, 256)), dim3(256), 0, st, a);
}

void launch_edges_emit(const EdgeArgs& a, hipStream_t st) {
  if (a.n_items == 0) return;
  hipLaunchKernelGGL(k_edges_emit, dim3(nblk(a.n_items, 256)), dim3(256), 0, st, a);
}
