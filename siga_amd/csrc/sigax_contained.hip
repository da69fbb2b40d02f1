// siga_amd/csrc/sigax_contained.hip -- contained reads placed in a unitig call's layout on the device (gfx950 / CDNA4, wave64), so
// that they vote in the consensus pass and pair (rules: include/sigax.h).  No counterpart in the reference, which
// drops contained reads before it builds its graph.
//
//   k_cp_owner        one lane per placement: its unitig (a bisection over lay_offs), and per read the first placement that names it
//   k_cp_choice<0,1>  one lane per containment record: valid or not; two 64-bit minima per contained read give its choice
//   k_cp_init, k_cp_jump   the chain of choices resolved by pointer doubling, ceil(log2 n_reads) + 1 rounds, positions composed
//   k_cp_place        one lane per read: its class, and the placement in the root's unitig
//   (two stable radix passes order the placed contained reads by (unitig, offset, read id))
//   k_cp_keys2, k_cp_kept, k_cp_count, k_cp_scatter_chain, k_cp_scatter_cont   the per-unitig counts, and after their scan the
//                     ordered merge: a placement's rank among the others by bisection, among its own kind by a scan or the sort
//   k_cp_status       the eight status words
//
// Every kernel is one lane per element with loops of at most 33 steps, every index is checked against the size of its table, and
// nothing depends on the order in which lanes arrive: minima, sums and a maximum are all the atomics there are.
#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>

#include "sigax_contained.h"
#include "sigax_device.h"

namespace {

__device__ __forceinline__ u64 cp_units(const ContArgs& A) {
  u64 nu = *A.n_unitigs;
  nu = nu < A.max_unitigs ? nu : A.max_unitigs;
  return nu < A.n_reads ? nu : A.n_reads;
}

// the placements of unitig u (u < cp_units), or an empty span where lay_offs does not ascend or leaves the layout
__device__ __forceinline__ void cp_span(const ContArgs& A, u64 u, u64* a, u64* b) {
  const u64 x = A.lay_offs[u], y = A.lay_offs[u + 1];
  const bool ok = x <= y && y <= A.n_reads;
  *a = ok ? x : 0;
  *b = ok ? y : 0;
}

// the first i in [lo, hi) with key(i) >= v (AFTER: > v); key ascends; hi - lo < 2^32
template <bool AFTER, class Key>
__device__ __forceinline__ u64 cp_bound(u64 lo, u64 hi, u64 v, Key key) {
  for (int step = 0; step < 33 && lo < hi; ++step) {
    const u64 mid = lo + ((hi - lo) >> 1);
    const u64 k = key(mid);
    if (AFTER ? k <= v : k < v)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(256) void k_cp_owner(ContArgs A) {
  const u64 j = (u64)blockIdx.x * 256 + threadIdx.x;
  if (j >= A.n_reads) return;
  const u64 nu = cp_units(A);
  u32 own = CP_NONE;
  if (nu) {
    const u64 u = last_at_most(A.lay_offs, nu, j);
    u64 a, b;
    cp_span(A, u, &a, &b);
    if (a <= j && j < b) {
      own = (u32)u;
      const u32 r = A.layout[j].read;
      if ((u64)r < A.n_reads) atomicMin(&A.slot[r], (u32)j);
    }
  }
  A.owner[j] = own;
}

// rule 1
__device__ __forceinline__ bool cp_valid(const ContArgs& A, const sigax_mm_edge& e) {
  if ((u64)e.query >= A.n_reads || (u64)e.target >= A.n_reads || e.query == e.target || !(e.af & SIGAX_MM_CONTAINMENT)) return false;
  if (!A.contained[e.query]) return false;
  return (u64)e.reserved + (u64)A.lengths[e.query] <= (u64)A.lengths[e.target];
}

// rule 2 in two steps: (contained[target], num_diff) first, then (target, reversed, offset) among the records that reach it
template <int PASS>
__global__ __launch_bounds__(256) void k_cp_choice(ContArgs A) {
  const u64 k = (u64)blockIdx.x * 256 + threadIdx.x;
  u64 invalid = 0;
  if (k < A.n_conts) {
    const sigax_mm_edge e = A.conts[k];
    if (!cp_valid(A, e)) {
      invalid = PASS == 0 ? 1 : 0;
    } else {
      const u64 key1 = ((u64)(A.contained[e.target] ? 1u : 0u) << 32) | (u64)e.num_diff;
      if (PASS == 0) {
        atomicMin(&A.best1[e.query], key1);
      } else if (A.best1[e.query] == key1) {
        atomicMin(&A.best2[e.query], ((u64)e.target << 33) | ((u64)((e.af >> 2) & 1u) << 32) | (u64)e.reserved);  // target < 2^31
      }
    }
  }
  if (PASS == 0) wave_add(&A.words[CP_C_INVALID_RECORDS], invalid);
}

__global__ __launch_bounds__(256) void k_cp_init(ContArgs A) {
  const u64 c = (u64)blockIdx.x * 256 + threadIdx.x;
  u64 is_contained = 0;
  if (c < A.n_reads) {
    uint4 s = make_uint4(CP_NONE, 0, 0, 0);
    if (A.contained[c]) {
      is_contained = 1;
      const u64 b = A.best2[c];
      if (b != ~0ull) s = make_uint4((u32)(b >> 33), (u32)(b >> 32) & 1u, (u32)b, 1u);
    }
    A.state[0][c] = s;
  }
  wave_add(&A.words[CP_C_CONTAINED], is_contained);
}

// rule 3: c lies at (s.z, s.y) in r = s.x, r at (p.z, p.y) in p.x: c's place in p.x.  Modulo 2^32: a chain that ends never wraps
__global__ __launch_bounds__(256) void k_cp_jump(ContArgs A, const uint4* src, uint4* dst) {
  const u64 c = (u64)blockIdx.x * 256 + threadIdx.x;
  if (c >= A.n_reads) return;
  uint4 s = src[c];
  if (s.x != CP_NONE && (u64)s.x < A.n_reads) {
    const uint4 p = src[s.x];
    if (p.x != CP_NONE) {
      const u32 off = p.y ? p.z + A.lengths[s.x] - s.z - A.lengths[c] : p.z + s.z;
      s = make_uint4(p.x, s.y ^ p.y, off, s.w + p.w);
    }
  }
  dst[c] = s;
}

// rules 3 (the end of the walk) and 4
__global__ __launch_bounds__(256) void k_cp_place(ContArgs A, const uint4* fin) {
  const u64 c = (u64)blockIdx.x * 256 + threadIdx.x;
  u64 placed = 0, no_chain = 0, removed = 0;
  u32 steps = 0;
  if (c < A.n_reads) {
    u32 cls = SIGAX_CP_NOT_CONTAINED, pu = CP_NONE, pf = 0;
    u64 off = 0;
    if (A.contained[c]) {
      const uint4 s = fin[c];
      const u64 r = s.x;
      if (s.x == CP_NONE) {
        cls = SIGAX_CP_NO_RECORD;
      } else if (r >= A.n_reads || fin[r].x != CP_NONE || A.contained[r]) {
        cls = SIGAX_CP_NO_ROOT;  // a cycle, or a contained read without a choice at the end
      } else {
        steps = s.w;
        const u32 j = A.slot[r];
        const u32 u = j != CP_NONE && (u64)j < A.n_reads ? A.owner[j] : CP_NONE;
        if (u == CP_NONE) {
          cls = SIGAX_CP_ROOT_REMOVED;
        } else {
          const sigax_placement pl = A.layout[j];
          const u64 Lr = A.lengths[r], Lc = A.lengths[c];
          const u32 v2 = pl.flags & SIGAX_PLACED_REV;
          off = v2 ? pl.offset + Lr - (u64)s.z - Lc : pl.offset + (u64)s.z;
          const u64 U = A.seq_offs[(u64)u + 1] - A.seq_offs[u];
          if (off <= U && Lc <= U - off) {
            cls = SIGAX_CP_PLACED;
            pu = u;
            pf = (s.y ^ v2) | SIGAX_PLACED_CONTAINED;
          } else {
            cls = SIGAX_CP_INVALID;
          }
        }
      }
      placed = cls == SIGAX_CP_PLACED;
      no_chain = cls == SIGAX_CP_NO_RECORD || cls == SIGAX_CP_NO_ROOT;
      removed = cls == SIGAX_CP_ROOT_REMOVED;
    }
    A.place_class[c] = (unsigned char)cls;
    A.pu[c] = pu;
    A.pflags[c] = pf;
    A.poff[c] = off;
    A.keys[0][c] = pu != CP_NONE ? off : ~0ull;  // ids ascend: the two stable passes leave (unitig, offset, read id) order
    A.vals[0][c] = (u32)c;
  }
  wave_add(&A.words[CP_C_PLACED], placed);
  wave_add(&A.words[CP_C_NO_CHAIN], no_chain);
  wave_add(&A.words[CP_C_ROOT_REMOVED], removed);
  const u32 longest = wave_max32(steps);
  if (longest && (threadIdx.x & 63u) == 0u) atomicMax(&A.words[CP_C_LONGEST], (u64)longest);
}

// the first pass has left the read ids in offset order in vals[1]: their unitigs in that order
__global__ __launch_bounds__(256) void k_cp_keys2(ContArgs A) {
  const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
  if (i >= A.n_reads) return;
  const u64 c = A.vals[1][i];
  A.keys[0][i] = c < A.n_reads ? (u64)A.pu[c] : (u64)CP_NONE;
}

__device__ __forceinline__ bool cp_read_placed(const ContArgs& A, u32 r) { return (u64)r < A.n_reads && A.place_class[r] == SIGAX_CP_PLACED; }

__global__ __launch_bounds__(256) void k_cp_kept(ContArgs A) {
  const u64 j = (u64)blockIdx.x * 256 + threadIdx.x;
  if (j >= A.n_reads) return;
  A.kept[j] = A.owner[j] != CP_NONE && !cp_read_placed(A, A.layout[j].read) ? 1u : 0u;
}

// the placed contained reads of unitig u in the sorted list: [first, last)
__device__ __forceinline__ void cp_cont_span(const ContArgs& A, u64 u, u64* first, u64* last) {
  const u64* k = A.keys[1];
  *first = cp_bound<false>(0, A.n_reads, u, [k](u64 i) { return k[i]; });
  *last = cp_bound<true>(*first, A.n_reads, u, [k](u64 i) { return k[i]; });
}

__global__ __launch_bounds__(256) void k_cp_count(ContArgs A) {
  const u64 u = (u64)blockIdx.x * 256 + threadIdx.x;
  if (u >= A.max_unitigs) return;
  u32 n = 0;
  if (u < cp_units(A)) {
    u64 a, b, first, last;
    cp_span(A, u, &a, &b);
    cp_cont_span(A, u, &first, &last);
    n = (u32)(A.keptscan[b] - A.keptscan[a] + (last - first));
  }
  A.cnt[u] = n;
}

// rule 5: a chain placement keeps its rank among the chain placements that stay, and goes behind the contained ones that begin
// before it
__global__ __launch_bounds__(256) void k_cp_scatter_chain(ContArgs A) {
  const u64 j = (u64)blockIdx.x * 256 + threadIdx.x;
  if (j >= A.n_reads || !A.kept[j]) return;
  const u64 u = A.owner[j];  // below cp_units: k_cp_owner
  u64 a, b, first, last;
  cp_span(A, u, &a, &b);
  cp_cont_span(A, u, &first, &last);
  const u64 off = placement_offset(A.layout, j);
  const u32* ids = A.vals[0];
  const u64* poff = A.poff;
  const u64 n = A.n_reads;
  const u64 before = cp_bound<false>(first, last, off, [ids, poff, n](u64 i) { return (u64)ids[i] < n ? poff[ids[i]] : ~0ull; }) - first;
  const u64 to = A.lay_offs2[u] + (A.keptscan[j] - A.keptscan[a]) + before;
  if (to < A.n_reads) A.layout2[to] = A.layout[j];
}

// ... and a contained one its rank in the sorted list, behind the chain placements that begin at or before it
__global__ __launch_bounds__(256) void k_cp_scatter_cont(ContArgs A) {
  const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
  if (i >= A.n_reads) return;
  const u64 u = A.keys[1][i], c = A.vals[0][i];
  if (u >= cp_units(A) || c >= A.n_reads) return;  // (CP_NONE: the reads that are not placed, at the end of the list)
  u64 a, b, first, last;
  cp_span(A, u, &a, &b);
  cp_cont_span(A, u, &first, &last);
  const u64 off = A.poff[c];
  const sigax_placement* lay = A.layout;
  const u64 upto = cp_bound<true>(a, b, off, [lay](u64 j) { return placement_offset(lay, j); });
  const u64 to = A.lay_offs2[u] + (i - first) + (A.keptscan[upto] - A.keptscan[a]);
  if (to < A.n_reads) {
    sigax_placement p;
    p.read = (u32)c;
    p.flags = A.pflags[c];
    p.offset = off;
    A.layout2[to] = p;
  }
}

__global__ void k_cp_status(ContArgs A) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  A.status[0] = A.words[CP_C_CONTAINED];
  A.status[1] = A.n_conts;
  A.status[2] = A.words[CP_C_INVALID_RECORDS];
  A.status[3] = A.words[CP_C_PLACED];
  A.status[4] = A.words[CP_C_NO_CHAIN];
  A.status[5] = A.words[CP_C_ROOT_REMOVED];
  A.status[6] = A.words[CP_C_LONGEST];
  A.status[7] = A.words[CP_TOTAL];
}

}  // namespace

hipError_t contained_sort_bytes(unsigned long long n, unsigned long long* bytes) {
  size_t tb = 0;
  *bytes = 0;
  if (n == 0) return hipSuccess;
  const hipError_t e = rocprim::radix_sort_pairs(nullptr, tb, (const u64*)nullptr, (u64*)nullptr, (const u32*)nullptr, (u32*)nullptr, (size_t)n, 0u, 64u);
  *bytes = tb;
  return e;
}

// n_reads > 0 and max_unitigs > 0; the scratch zeroed or filled as ContArgs says
hipError_t launch_contained_place(const ContArgs& a, hipStream_t st) {
  const unsigned gr = blocks_of(a.n_reads), gu = blocks_of(a.max_unitigs);
  hipLaunchKernelGGL(k_cp_owner, dim3(gr), dim3(256), 0, st, a);
  if (a.n_conts) {
    hipLaunchKernelGGL(k_cp_choice<0>, dim3(blocks_of(a.n_conts)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_cp_choice<1>, dim3(blocks_of(a.n_conts)), dim3(256), 0, st, a);
  }
  hipLaunchKernelGGL(k_cp_init, dim3(gr), dim3(256), 0, st, a);
  for (unsigned r = 0; r < a.rounds; ++r) hipLaunchKernelGGL(k_cp_jump, dim3(gr), dim3(256), 0, st, a, (const uint4*)a.state[r & 1], a.state[(r & 1) ^ 1]);
  hipLaunchKernelGGL(k_cp_place, dim3(gr), dim3(256), 0, st, a, (const uint4*)a.state[a.rounds & 1]);
  // stable passes, the minor key first: the offset, then the unitig (CP_NONE for the reads that are not placed)
  size_t tb = (size_t)a.sort_tmp_bytes;
  hipError_t e = rocprim::radix_sort_pairs(a.sort_tmp, tb, (const u64*)a.keys[0], a.keys[1], (const u32*)a.vals[0], a.vals[1], (size_t)a.n_reads, 0u, 64u, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_cp_keys2, dim3(gr), dim3(256), 0, st, a);
  tb = (size_t)a.sort_tmp_bytes;
  e = rocprim::radix_sort_pairs(a.sort_tmp, tb, (const u64*)a.keys[0], a.keys[1], (const u32*)a.vals[1], a.vals[0], (size_t)a.n_reads, 0u, 32u, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_cp_kept, dim3(gr), dim3(256), 0, st, a);
  launch_scan(a.kept, a.n_reads, a.partial, a.keptscan, a.keptscan + a.n_reads, st);
  hipLaunchKernelGGL(k_cp_count, dim3(gu), dim3(256), 0, st, a);
  launch_scan(a.cnt, a.max_unitigs, a.partial, a.lay_offs2, a.words + CP_TOTAL, st);
  hipLaunchKernelGGL(k_cp_scatter_chain, dim3(gr), dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_cp_scatter_cont, dim3(gr), dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_cp_status, dim3(1), dim3(64), 0, st, a);
  return hipGetLastError();
}
