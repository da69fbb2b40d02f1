// siga_amd/csrc/sigax_unitig.hip -- `siga unitig` on the device (gfx950 / CDNA4, wave64): every unbranched chain of overlaps
// compacted into one sequence, the fixpoint of the reference's Bigraph::simplify (src/bigraph.cpp:341-414, Vertex::merge at
// :131-202) over the edge records of an overlap run.  The rules are in include/sigax.h and DESIGN.md 9d; the restatement the
// tests hold this against is tests/unitig_cases.py::expected.
//
// A read has two ends, B = 0 (prefix) and E = 1 (suffix); state 2r + e = "read r, left through end e".
//   k_uni_degree  one lane per record: the kept ones add to deg[2r + e] of the ends they touch (atomics), the ignored ones
//                 are counted
//   k_uni_links   one lane per record: a simple record writes link[end] = {the end it touches on the other read, len} at both
//                 its ends.  An end of degree 1 is touched by one kept record, so no two lanes write one entry.
//   k_uni_init / k_uni_jump   list ranking by pointer jumping over the 2 n states, ping-pong buffers, `rounds` =
//                 ceil(log2 n) + 1 launches the host counts: a state carries {state reached, hops, smallest read id on the way,
//                 bases on the way}.  A state that still has a successor after the last round lies on a cycle, and has
//                 then been round it at least once: its smallest id is the cycle's.
//   k_uni_cut     the lane of that read's state (m, B) takes the link into m's B end out, at both its ends, and notes the
//                 overlap it closed; ranking runs once more (its launches leave at once when no cycle was cut)
//   k_uni_heads   one lane per read: which of its two directions leads to the head of its unitig (the terminal with the
//                 smaller id), and for a head the unitig's reads and bases; launch_scan turns these into unitig numbers,
//                 layout offsets and sequence offsets
//   k_uni_place   one lane per read: its placement record (one 16-byte store), for a head the unitig's table entries, and
//                 where the bases it contributes go
//   k_uni_bases   the bytes.  The stretches the placements contribute lie back to back in the output, in layout order, and
//                 most are short (27 bases on average at BASELINE configs[1]): a wave takes 64 consecutive placements,
//                 keeps their {destination, source, direction} in LDS, and its lanes take consecutive 16-byte pieces of the
//                 destination range the 64 cover.  A piece that lies in one stretch is one 16-byte load (ascending, or
//                 descending and complemented for a reverse placement) and one 16-byte store; a piece over several
//                 stretches is gathered byte by byte; the range's unaligned head and tail are byte stores.
// Tip trimming and the graph between the unitigs (sigax_unitigs_trim_*; tests/trim_cases.py::expected_trim): the
// kernels above as <TRIM = true> skip reads with removed[r] != 0 and the records that touch one, and
//   k_trim_decide one lane per read: a head judges its unitig by its two end degrees, its bases and its reads (what
//                 k_uni_heads left) and writes the verdict under its own id; islands and dead ends are counted
//   k_step_mark<TrimStep>   one lane per read: it finds its head through the final rank entry and takes the verdict into removed[]
//   k_lift_flag / k_lift_write   one lane per record: a live record that is no link of the final graph is flagged, launch_scan
//                 gives it its place, and it is written over unitig ids and unitig ends (one 16-byte load, one 16-byte store)
// A round's launches leave at once when the round before it removed nothing (idle_round).
// What a removing step of a round must provide is written down at `Step`; every step begins with launch_step_graph and ends with
// k_step_mark, and the wave reductions, counter slots and base helpers are sigax_device.h's.
// Non-maximal overlap cutting (sigax_unitigs_prune_*; tests/prune_cases.py::expected_prune): the kernels above as
// <TRIM = 2> also skip the records with cut[i] != 0, k_uni_degree<2> takes the longest participant per read end (atomicMax), and
//   k_prune_clear  the step's scratch emptied: the maxima and, careful mode, the table (a kernel: idle rounds write nothing)
//   k_prune_unique one lane per read: a head scores its unitig from its reads and bases (double, one log pair per unitig)
//   k_prune_keys  careful mode, one lane per record: the (read end, unitig at the other end) pairs of the participants within
//                 delta of their end's maximum go into an open-addressing table; the longest self record per read end
//   k_prune_cut   one lane per record: candidate from either side, held back or not, cut[i] = round
// Chimeric unitig removal (sigax_unitigs_chimeric_*; tests/chimeric_cases.py::expected_chimeric): a third step of a
// round, over the <TRIM = 2> kernels and k_prune_unique under the chimeric threshold, and
//   k_chim_clear   the step's scratch emptied (a kernel: idle rounds write nothing)
//   k_chim_minima  one lane per record, twice: an end of degree 1 learns the read end at its record's other side; an end of
//                  degree >= 2 takes the smallest (bases, head) and (reads, head) over the unitigs its participants lead to
//                  (64-bit atomicMin behind a plain compare), then the smallest among those not of the first one's unitig
//   k_chim_decide  one lane per read: a head judges its unitig from its two end degrees, its neighbours' degrees, scores and minima
//   k_step_mark<ChimStep>   one lane per read: removed[r] = round | 0x80000000 under a chimeric head
// Bubble popping (sigax_unitigs_bubble_*; tests/bubble_cases.py::expected_bubble): a step between the trim and the
// chimeric step of a round, over the <TRIM = 2> kernels, and
//   k_arm_clear<BubStep>   the step's scratch emptied (a kernel: idle rounds write nothing)
//   k_bub_ends     one lane per record: an end of degree 1 learns the read end at its record's other side and the record's length
//   k_bub_place    one lane per read: the step's own layout, where in its unitig the bases a read adds begin (bases test only)
//   k_bub_arms     one lane per read: a head judges whether its unitig is an arm that takes part, and with which (lo, hi, span)
//   k_arm_group<.., true>   one lane per read: an arm finds its group's slot in an open-addressing table under the key (lo, hi, span)
//                  and offers (K << 32) | ~head
//   k_bub_losers   one lane per read: an arm that is not its group's maximum is popped (no bases test) or appended to a list
//   k_bub_compare  one wave per appended loser: lanes stride over the window, each base found by bisecting the placements
//   k_step_mark<BubStep>   one lane per read: removed[r] = round | 0x40000000 under a popped head
// Indel bubble popping (sigax_unitigs_indel_*; tests/indel_cases.py::expected_indel): a step between the bubble and the
// chimeric step of a round, over the <TRIM = 2> kernels, k_bub_ends, k_bub_place and k_bub_arms as they are, and
//   k_arm_clear<IndStep>   the bubble step's clear, and no pair appended
//   k_arm_group<.., false>  one lane per read: the bubble step's grouping under the key (lo, hi) alone
//   k_ind_losers   one lane per read: a loser of the winner's span, or more than E bases from it, stays; another is appended to a list
//   k_ind_compare  one wave per appended pair: both windows staged as bytes in LDS (at most 4096 + 4096), then the furthest-reaching
//                  recurrence over the 2 E + 1 diagonals, one per lane, neighbours by shuffles, at most E + 1 turns
//   k_step_mark<IndStep>   one lane per read: removed[r] = round | 0x20000000 under a popped head
// Transitive reduction (sigax_unitigs_reduce_*; tests/reduce_cases.py::expected_reduce): a pass before the cut step of
// every round and one more before the final unitigs.  It flags records in bit 31 of cut[], and every kernel above already takes a
// record with cut[i] != 0 as not there, so none of them changed.  A record a-b of overlap len is explained through a third read's
// state w iff records a-w and (w ^ 1)-b exist with ext(a -> w) + ext((w ^ 1) -> b) == ext(a -> b): given a-w, the one record that
// can close the triangle has the overlap len + ext(a -> w).  So the pass keeps the participants twice: by state (an adjacency in CSR
// form: the walk needs "every w at a") and by exact key (an open-addressing table: the walk then asks one yes/no question per w).
//   k_red_clear    bit 31 off every cut[i]; the counts, the table and the pass's counters emptied (a kernel: an idle pass writes nothing)
//   k_red_count    one lane per record: a participant adds to the count of both its states; launch_scan gives the segments
//   k_red_fill     one lane per record: {other state, extension} into both segments (8 bytes each), and the record's index into the
//                  table under (smaller state, larger state, overlap); a slot names a record, a probe compares that record's fields,
//                  so the 96-bit key is exact and the table is 4 bytes a slot, at least four slots a record
//   k_red_walk     one lane per record: over the segment of a, then of b, entries with a smaller extension on a third read are
//                  probed; the first hit sets cut[i] = 0x80000000.  One lane per record and not a lane group: at 21 records per read
//                  end (exhaustive, 30-fold) a segment is a third of a wave, and a hit ends the walk early; an end of degree 5000 is
//                  5000 turns of one lane, slow and not wrong.  Witnesses are read from the adjacency and the table alone, which this
//                  kernel does not write: verdicts do not depend on each other.
//   k_red_note     one lane: the pass's counts into the call's (first pass, latest pass, passes that ran)
// The tables' probe loops are bounded by their capacity, which holds at least twice the keys that can go in.
// No loop's trip count depends on the records: ignored records never enter the links, and the links of simple records are
// consistent by construction -- but for the reduction's walk, whose trips are the degree of a read end (at most 2 n_edges, the
// adjacency's size, which the host knows).  Every store is bounds-checked all the same.  Plain vector stores only; integer work, no LDS
// beyond the 64 descriptors and the indel step's two windows, no MFMA.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "sigax_device.h"
#include "sigax_kernels.h"

namespace {
constexpr u32 NIL = 0xFFFFFFFFu;

// ---- phase 1, 2: records ----
// what a record is: 0 malformed, 1 below min_overlap, 2 kept; for a kept one the two ends it touches and its kind
struct RecClass {
  u32 kind, sq, st;  // states 2q + end, 2t + end
  bool contain, self;
};
__device__ __forceinline__ RecClass classify(const uint4 rec, const UnitigArgs& A) {
  RecClass c;
  c.kind = 0;
  c.sq = c.st = 0;
  c.contain = c.self = false;
  const u32 q = rec.x, t = rec.y, len = rec.z, af = rec.w;
  if ((u64)q >= A.n_reads || (u64)t >= A.n_reads) return c;
  if (af > 7u || ((af >> 2) & 1u) != ((af ^ (af >> 1)) & 1u)) return c;
  const u32 lq = A.lengths[q], lt = A.lengths[t];
  if (len == 0u || len > (lq < lt ? lq : lt)) return c;
  if (len < A.min_overlap) {
    c.kind = 1;
    return c;
  }
  c.kind = 2;
  c.sq = 2u * q + ((af & 1u) ? 0u : 1u);
  c.st = 2u * t + ((af & 2u) ? 1u : 0u);
  c.contain = len == lq || len == lt;
  c.self = q == t;
  return c;
}

// TRIM = 1: the kernels of sigax_unitigs_trim_*: reads with removed[r] != 0 are not there, nor are the records that touch one.
// They take the longer argument block; TRIM = 0 is sigax_unitigs_device's code as it was, over the block it had.  TRIM = 2: the
// kernels of sigax_unitigs_prune_*, as 1 and without the records that were cut, over a block of their own again.
template <int TRIM>
using ArgsOf = std::conditional_t<TRIM == 2, UnitigPruneArgs, std::conditional_t<TRIM == 1, UnitigTrimArgs, UnitigArgs>>;
// a trim round after one that removed nothing has nothing to do (as k_uni_init(second) when no cycle was cut)
template <int TRIM>
__device__ __forceinline__ bool idle_round(const ArgsOf<TRIM>& A) {
  if constexpr (TRIM != 0) return A.round > 1u && A.trim[TRIM_ROUND0 + A.round - 1u] == 0ull;
  return false;
}
// both reads of a kept record alive
template <int TRIM>
__device__ __forceinline__ bool live_pair(const ArgsOf<TRIM>& A, const RecClass& c) {
  if constexpr (TRIM != 0) return (A.removed[c.sq >> 1] | A.removed[c.st >> 1]) == 0u;
  return true;
}
// record i was cut in an earlier round (i < n_edges)
template <int TRIM>
__device__ __forceinline__ bool was_cut(const ArgsOf<TRIM>& A, u64 i) {
  if constexpr (TRIM == 2) return A.cut[i] != 0u;
  return false;
}

template <int TRIM>
__global__ __launch_bounds__(256) void k_uni_degree(ArgsOf<TRIM> A) {
  if (idle_round<TRIM>(A)) return;
  const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
  u32 bad = 0, low = 0, dropped = 0;
  if (i < A.n_edges) {
    const RecClass c = classify(reinterpret_cast<const uint4*>(A.edges)[i], A);
    bad = c.kind == 0u;
    low = c.kind == 1u;
    if (was_cut<TRIM>(A, i)) {
    } else if (c.kind == 2u && !live_pair<TRIM>(A, c)) {
      dropped = 1;
    } else if (c.kind == 2u) {
      if (c.contain) {  // both directions (src/bigraph.cpp:497-522): every end of both reads
        atomicAdd(&A.deg[c.sq & ~1u], 1u);
        atomicAdd(&A.deg[c.sq | 1u], 1u);
        atomicAdd(&A.deg[c.st & ~1u], 1u);
        atomicAdd(&A.deg[c.st | 1u], 1u);
      } else {
        atomicAdd(&A.deg[c.sq], 1u);
        atomicAdd(&A.deg[c.st], 1u);
        if constexpr (TRIM == 2) {  // a participant of the cut step
          if (A.maxlen) {
            const u32 len = reinterpret_cast<const uint4*>(A.edges)[i].z;
            atomicMax(&A.maxlen[c.sq], len);
            atomicMax(&A.maxlen[c.st], len);
          }
        }
      }
    }
  }
  const u64 tb = wave_sum(bad), tl = wave_sum(low);
  if ((threadIdx.x & 63u) == 0u) {
    if (tb) atomicAdd(&A.counts[UNI_C_BAD], tb);
    if (tl) atomicAdd(&A.counts[UNI_C_LOW], tl);
  }
  if constexpr (TRIM != 0) {
    const u64 td = wave_sum(dropped);
    if ((threadIdx.x & 63u) == 0u && td && A.round == 0u) atomicAdd(counter_slot(A.trim, TRIM_C_DROPPED), td);
  }
}

template <int TRIM>
__global__ __launch_bounds__(256) void k_uni_links(ArgsOf<TRIM> A) {
  if (idle_round<TRIM>(A)) return;
  const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
  u32 simple = 0;
  if (i < A.n_edges) {
    const uint4 rec = reinterpret_cast<const uint4*>(A.edges)[i];
    const RecClass c = classify(rec, A);
    if (c.kind == 2u && !c.contain && !c.self && !was_cut<TRIM>(A, i) && live_pair<TRIM>(A, c) && A.deg[c.sq] == 1u && A.deg[c.st] == 1u) {
      A.link[c.sq] = make_uint2(c.st, rec.z);
      A.link[c.st] = make_uint2(c.sq, rec.z);
      simple = 1;
    }
  }
  const u64 ts = wave_sum(simple);
  if ((threadIdx.x & 63u) == 0u && ts) atomicAdd(&A.counts[UNI_C_SIMPLE], ts);
}

// ---- phase 3, 4: list ranking ----
// rk[s] = {successor or NIL, state reached so far, hops so far, smallest read id so far}; dist[s] = bases so far: a hop
// into read y over an overlap of len adds L[y] - len.  second: the ranking after the cut, which has nothing to do when
// nothing was cut.
template <int TRIM>
__global__ __launch_bounds__(256) void k_uni_init(ArgsOf<TRIM> A, uint4* __restrict__ rk, u64* __restrict__ dist, int second) {
  if (idle_round<TRIM>(A)) return;
  if (second && A.counts[UNI_C_CYCLES] == 0ull) return;
  const u64 s = (u64)blockIdx.x * 256u + threadIdx.x;
  if (s >= 2 * A.n_reads) return;
  const uint2 lk = A.link[s];
  const u32 r = (u32)(s >> 1);
  if (lk.x == NIL || (u64)lk.x >= 2 * A.n_reads) {
    rk[s] = make_uint4(NIL, (u32)s, 0u, r);
    dist[s] = 0;
  } else {
    const u32 y = lk.x >> 1, nx = lk.x ^ 1u;
    rk[s] = make_uint4(nx, nx, 1u, r < y ? r : y);
    dist[s] = (u64)A.lengths[y] - lk.y;
  }
}

template <int TRIM>
__global__ __launch_bounds__(256) void k_uni_jump(ArgsOf<TRIM> A, const uint4* __restrict__ in, const u64* __restrict__ din,
                                                  uint4* __restrict__ out, u64* __restrict__ dout, int second) {
  if (idle_round<TRIM>(A)) return;
  if (second && A.counts[UNI_C_CYCLES] == 0ull) return;
  const u64 s = (u64)blockIdx.x * 256u + threadIdx.x;
  if (s >= 2 * A.n_reads) return;
  uint4 a = in[s];
  u64 d = din[s];
  if (a.x != NIL) {
    const uint4 b = in[a.x];
    d += din[a.x];
    a = make_uint4(b.x, b.y, a.z + b.z, a.w < b.w ? a.w : b.w);
  }
  out[s] = a;
  dout[s] = d;
}

template <int TRIM>
__global__ __launch_bounds__(256) void k_uni_cut(ArgsOf<TRIM> A, const uint4* __restrict__ rk) {
  if (idle_round<TRIM>(A)) return;
  const u64 m = (u64)blockIdx.x * 256u + threadIdx.x;
  u32 cut = 0;
  if (m < A.n_reads) {
    const uint4 a = rk[2 * m];
    if (a.x != NIL && a.w == (u32)m) {  // on a cycle, and its smallest read: the one lane of the cycle that acts
      const uint2 lk = A.link[2 * m];
      if (lk.x != NIL && (u64)lk.x < 2 * A.n_reads) {
        A.link[2 * m] = make_uint2(NIL, 0u);
        A.link[lk.x] = make_uint2(NIL, 0u);
        A.closing[m] = SIGAX_UNITIG_CIRCULAR | (lk.y << 1);
        cut = 1;
      }
    }
  }
  const u64 tc = wave_sum(cut);
  if ((threadIdx.x & 63u) == 0u && tc) atomicAdd(&A.counts[UNI_C_CYCLES], tc);
}

// ---- phase 5: heads ----
// (head_dir, sigax_device.h: the direction of read r that leads to its unitig's head)
template <int TRIM>
__global__ __launch_bounds__(256) void k_uni_heads(ArgsOf<TRIM> A, const uint4* __restrict__ rk, const u64* __restrict__ dist) {
  if (idle_round<TRIM>(A)) return;
  const u64 r = (u64)blockIdx.x * 256u + threadIdx.x;
  if (r >= A.n_reads) return;
  bool alive = true;
  if constexpr (TRIM != 0) alive = A.removed[r] == 0u;  // a removed read lies alone in the ranking: it heads nothing
  const uint4 a0 = rk[2 * r], a1 = rk[2 * r + 1];
  const u32 d = head_dir(a0, a1);
  const uint4 to = d ? a1 : a0, away = d ? a0 : a1;
  u32 one = 0, reads = 0;
  u64 bases = 0;
  if (alive && to.z == 0u && to.x == NIL) {  // nothing between r and the head: r is it
    one = 1;
    reads = away.z + 1u;
    bases = (u64)A.lengths[r] + dist[2 * r + (d ^ 1u)];
  }
  A.cnt[r] = one;
  A.cnt[A.n_reads + 1 + r] = reads;
  A.cnt[2 * (A.n_reads + 1) + r] = (u32)bases;
  A.cnt[3 * (A.n_reads + 1) + r] = (u32)(bases >> 32);
}

// ---- phase 6: placements ----
template <int TRIM>
__global__ __launch_bounds__(256) void k_uni_place(ArgsOf<TRIM> A, const uint4* __restrict__ rk, const u64* __restrict__ dist) {
  const u64 r = (u64)blockIdx.x * 256u + threadIdx.x;
  const u64 n = A.n_reads;
  if (r >= n) return;
  const u64 *unum = A.scan, *layr = A.scan + (n + 1), *lo = A.scan + 2 * (n + 1), *hi = A.scan + 3 * (n + 1);
  bool alive = true;
  if constexpr (TRIM != 0) {  // a removed read has no placement and heads nothing
    alive = A.removed[r] == 0u;
    if (!alive) A.umap[r] = NIL;
  }
  if (alive) {
    const uint4 a0 = rk[2 * r], a1 = rk[2 * r + 1];
    const u32 d = head_dir(a0, a1);
    const uint4 to = d ? a1 : a0;
    const u64 h = to.y >> 1;  // the head
    if (h >= n) return;
    const u64 off = dist[2 * r + d], slot = layr[h] + to.z, seq0 = lo[h] + (hi[h] << 32);
    if (slot < n) {
      // entered through the end it is left through on the way to the head: through B = forward
      reinterpret_cast<uint4*>(A.layout)[slot] = make_uint4((u32)r, d ? SIGAX_PLACED_REV : 0u, (u32)off, (u32)(off >> 32));
      // the bases r adds: its last L - len, len = the overlap with the read before it
      const uint2 lk = A.link[2 * r + d];
      const u64 skip = lk.x == NIL ? 0ull : (u64)lk.y, L = A.lengths[r], b0 = A.offs[r];
      A.dst[slot] = seq0 + off + skip;
      A.src[slot] = (d ? b0 + L - 1ull - skip : b0 + skip) | ((u64)d << 63);
    }
    if constexpr (TRIM != 0) A.umap[r] = ((u32)unum[h] << 1) | d;
    if (to.z == 0u && to.x == NIL) {  // the head writes its unitig's entries
      const u64 u = unum[r];
      if (u < n) {
        A.seq_offs[u] = seq0;
        A.lay_offs[u] = layr[r];
        A.uflags[u] = A.closing[r];
      }
    }
  }
  if (r == 0) {
    const u64 U = unum[n], bases = lo[n] + (hi[n] << 32);
    if (U <= n) {
      A.seq_offs[U] = bases;
      A.lay_offs[U] = layr[n];
    }
    A.dst[n] = bases;
    if constexpr (TRIM != 0) {  // the placements are those of the alive reads: k_uni_bases<1> stops after them
      if (layr[n] < n) A.dst[layr[n]] = bases;
    }
    const u64 cyc = A.counts[UNI_C_CYCLES], simple = A.counts[UNI_C_SIMPLE];
    A.status[0] = U;
    A.status[1] = bases;
    A.status[2] = A.counts[UNI_C_BAD];
    A.status[3] = A.counts[UNI_C_LOW];
    A.status[4] = simple - (cyc < simple ? cyc : simple);  // a cycle's closing record is not merged
    A.status[5] = cyc;
  }
}

// ---- phase 7: bases ----
struct BaseSh {
  u64 dst[4][65];
  u64 src[4][64];
};

template <int TRIM>
__global__ __launch_bounds__(256) void k_uni_bases(ArgsOf<TRIM> A) {
  __shared__ BaseSh sh;
  const u32 wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  u64 n = A.n_reads;
  if constexpr (TRIM != 0) {  // the placements of the alive reads (k_uni_place<1> closed dst after them)
    const u64 placed = A.scan[(A.n_reads + 1) + A.n_reads];
    if (placed < n) n = placed;
  }
  const u64 first = ((u64)blockIdx.x * 4u + wave) * 64u;  // the wave's first placement
  const bool live = first < n;
  // bytes of reads: nothing beyond src_end is read, nothing beyond dst_cap written (sum of the unitigs <= sum of the reads)
  const u64 src_end = A.offs[A.n_reads], dst_cap = src_end - A.offs[0];
  const u32 cnt = live ? (u32)(n - first < 64 ? n - first : 64) : 0u;
  if (lane < cnt) {
    sh.dst[wave][lane] = A.dst[first + lane];
    sh.src[wave][lane] = A.src[first + lane];
  }
  if (live && lane == 0) sh.dst[wave][cnt] = A.dst[first + cnt];
  __syncthreads();
  if (!live) return;
  const u64* D = sh.dst[wave];
  const u64* S = sh.src[wave];
  const u64 lo = D[0];
  u64 hi = D[cnt];
  if (hi > dst_cap) hi = dst_cap;
  if (lo >= hi) return;
  unsigned char* out = A.useqs;
  // the source byte of destination byte p, p in stretch k
  auto fetch = [&](u64 p, u32 k) -> u32 {
    const u64 s = S[k], rel = p - D[k];
    const bool rev = (s >> 63) != 0ull;
    const u64 at = rev ? (s & ~(1ull << 63)) - rel : s + rel;
    if (at >= src_end) return 'N';  // (no consistent input comes here)
    const u32 b = A.seqs[at];
    return rev ? comp_byte(b) : b;
  };
  // stretch of destination byte p: the last k with D[k] <= p (D ascends over a wave's stretches).  (Not last_at_most: D is the
  // wave's window in LDS, indexed in 32 bits, and cnt <= 64 bounds the steps.)
  auto find = [&](u64 p) -> u32 {
    u32 a = 0, b = cnt;
    while (b - a > 1u) {  // at most 6 steps
      const u32 m = (a + b) >> 1;
      if (D[m] <= p) a = m;
      else b = m;
    }
    return a;
  };
  // pieces of 16 bytes on the output's own 16-byte grid (the caller's buffer is 16-byte aligned: sigax.h)
  const u64 p0 = lo & ~15ull, pieces = (hi - p0 + 15) >> 4;
  for (u64 c = lane; c < pieces; c += 64) {
    const u64 b = p0 + 16 * c;
    if (b >= lo && b + 16 <= hi) {
      u32 k = find(b);
      uint4 v;
      if (D[k + 1] >= b + 16) {  // one stretch: one 16-byte load
        const u64 s = S[k], rel = b - D[k];
        const bool rev = (s >> 63) != 0ull;
        const u64 at = rev ? (s & ~(1ull << 63)) - rel : s + rel;  // first byte's source; a reverse stretch goes down from it
        const u64 from = rev ? at - 15ull : at;
        if (rev ? (at < 15ull || at >= src_end) : (at + 16 > src_end)) {
          unsigned char t[16];
          for (u32 j = 0; j < 16; ++j) t[j] = (unsigned char)fetch(b + j, k);
          __builtin_memcpy(&v, t, 16);
        } else {
          uint4 w;
          __builtin_memcpy(&w, A.seqs + from, 16);  // (no alignment promised: the compiler picks the access)
          if (rev) {
            // byte j of the piece = complement of byte 15 - j of the load (written out in each bases kernel: as a shared
            // function it compiles to other code, and these kernels stay as they are)
            const u32 x[4] = {w.w, w.z, w.y, w.x};
            u32 y[4];
            for (u32 q = 0; q < 4; ++q) {
              const u32 e = x[q];
              y[q] = comp_byte(e >> 24) | (comp_byte((e >> 16) & 255u) << 8) | (comp_byte((e >> 8) & 255u) << 16) | (comp_byte(e & 255u) << 24);
            }
            v = make_uint4(y[0], y[1], y[2], y[3]);
          } else {
            v = w;
          }
        }
      } else {
        unsigned char t[16];
        for (u32 j = 0; j < 16; ++j) {
          const u64 p = b + j;
          while (k + 1 < cnt && D[k + 1] <= p) ++k;  // (at most cnt steps over the piece)
          t[j] = (unsigned char)fetch(p, k);
        }
        __builtin_memcpy(&v, t, 16);
      }
      *reinterpret_cast<uint4*>(out + b) = v;
    } else {  // the range's head or tail: byte stores
      const u64 from = b < lo ? lo : b, to = b + 16 < hi ? b + 16 : hi;
      if (from < to) {
        u32 k = find(from);
        for (u64 p = from; p < to; ++p) {
          while (k + 1 < cnt && D[k + 1] <= p) ++k;
          out[p] = (unsigned char)fetch(p, k);
        }
      }
    }
  }
}

// ---- tip trimming: one round's verdicts and marks (TrimVisitor, src/bigraph_visitors.cpp:1119-1161) ----
// One lane per read.  A head judges its unitig: its left end is the end the head is entered through (nothing links there),
// its right end the state the walk away from the head stops in; a ring's two ends each carry its closing record.
__global__ __launch_bounds__(256) void k_trim_decide(UnitigTrimArgs A, const uint4* __restrict__ rk) {
  if (idle_round<1>(A)) return;
  const u64 r = (u64)blockIdx.x * 256u + threadIdx.x;
  const u64 n = A.n_reads;
  u32 island = 0, dead_end = 0;
  if (r < n) {
    u32 v = 0;
    if (A.removed[r] == 0u && A.cnt[r] != 0u) {
      const u64 K = A.cnt[n + 1 + r], bases = (u64)A.cnt[2 * (n + 1) + r] | ((u64)A.cnt[3 * (n + 1) + r] << 32);
      const uint4 a0 = rk[2 * r], a1 = rk[2 * r + 1];
      const u32 d = head_dir(a0, a1);
      const u32 last = (d ? a0 : a1).y;
      const u32 dl = A.deg[2 * r + d], dr = (u64)last < 2 * n ? A.deg[last] : 1u;
      const u64 L = A.min_branch_length, C = A.min_branch_coverage;
      if ((dl == 0u || dr == 0u) && bases <= L &&
          (A.min_branch_coverage == TRIM_NO_COVERAGE || (K - 1ull) * (L ? L : 1ull) <= ((C ? C : 1ull) - 1ull) * bases)) {
        v = 1;
        island = dl == 0u && dr == 0u;
        dead_end = island ^ 1u;
      }
    }
    A.verdict[r] = v;
  }
  const u64 ti = wave_sum(island), td = wave_sum(dead_end);
  if ((threadIdx.x & 63u) == 0u) {
    if (ti) atomicAdd(counter_slot(A.trim, TRIM_C_ISLANDS), ti);
    if (td) atomicAdd(counter_slot(A.trim, TRIM_C_DEAD_ENDS), td);
  }
}

// ---- what a removing step of a round is ----
// A step that takes reads out -- trim, bubble, indel, chimeric -- provides: its argument block (the block of the step before it,
// extended); its own counter block in it, zeroed before round 1, with a "reads" counter and one flag per round at ROUND0 + r; its
// bit in removed[] (0 for the trim step, whose block is `trim` itself); kernels of its own that leave verdict[head] for every
// unitig (after launch_step_graph: the graph of the live records and k_uni_heads); a k_x_status that writes its status words with
// rounds_ran.  k_step_mark<Step> then does what is common to them all.
template <class ArgsT, u64* ArgsT::*BLOCK, u32 C_READS_, u32 ROUND0_, u32 BIT_, u32 APPENDED_ = 0u>
struct Step {
  typedef ArgsT Args;
  static constexpr u32 C_READS = C_READS_, ROUND0 = ROUND0_, BIT = BIT_, APPENDED = APPENDED_;  // APPENDED: the word that counts a list
  static __device__ __forceinline__ u64* block(const ArgsT& A) { return A.*BLOCK; }
};
using TrimStep = Step<UnitigTrimArgs, &UnitigTrimArgs::trim, TRIM_C_READS, TRIM_ROUND0, 0u>;
using ChimStep = Step<UnitigChimericArgs, &UnitigChimericArgs::chim, CHIM_C_READS, CHIM_ROUND0, REMOVED_CHIMERIC>;
using BubStep = Step<UnitigBubbleArgs, &UnitigBubbleArgs::bub, BUB_C_READS, BUB_ROUND0, REMOVED_BUBBLE, BUB_APPENDED>;
using IndStep = Step<UnitigIndelArgs, &UnitigIndelArgs::ind, IND_C_READS, IND_ROUND0, REMOVED_INDEL, IND_APPENDED>;

// the head of the unitig of state s (s < 2 n_reads), by the final rank entry; NIL where the entry names no read
__device__ __forceinline__ u32 head_of(const UnitigArgs& A, const uint4* __restrict__ rk, u32 s) {
  const u64 r = s >> 1;
  const uint4 a0 = rk[2 * r], a1 = rk[2 * r + 1];
  const u32 h = (head_dir(a0, a1) ? a1 : a0).y >> 1;
  return (u64)h < A.n_reads ? h : NIL;
}
// the rounds in which a step did something, from its block's flags
__device__ __forceinline__ u64 rounds_ran(const u64* block, u32 round0) {
  u64 rounds = 0;
  for (u32 r = 1; r <= TRIM_MAX_ROUNDS; ++r) rounds += block[round0 + r] != 0ull;
  return rounds;
}

// One lane per read: the verdict lies under its head, which the final rank entry names; removed[r] = round | the step's bit.  The
// wave's count goes to the trim block's reads and to the step's own, and the round is flagged in both.
template <class S>
__global__ __launch_bounds__(256) void k_step_mark(typename S::Args A, const uint4* __restrict__ rk) {
  if (idle_round<1>(A)) return;
  const u64 r = (u64)blockIdx.x * 256u + threadIdx.x;
  const u64 n = A.n_reads;
  u32 gone = 0;
  if (r < n && A.removed[r] == 0u) {
    const u32 h = head_of(A, rk, 2u * (u32)r);  // (a state fits 32 bits: the host refuses n_reads >= 2^31)
    if (h != NIL && A.verdict[h] != 0u) {
      A.removed[r] = A.round | S::BIT;
      gone = 1;
    }
  }
  const u64 tg = wave_sum(gone);
  if ((threadIdx.x & 63u) == 0u && tg) {
    atomicAdd(counter_slot(A.trim, TRIM_C_READS), tg);
    if constexpr (S::BIT != 0u) atomicAdd(counter_slot(S::block(A), S::C_READS), tg);
    A.trim[TRIM_ROUND0 + A.round] = 1ull;  // (every wave that writes here writes the same)
    if constexpr (S::BIT != 0u) S::block(A)[S::ROUND0 + A.round] = 1ull;
  }
}

// ---- the records that were not merged, over unitigs ----
// lifted: kept, both reads alive, and not a link of the final graph (a ring's closing record was one and was cut: lifted)
template <int TRIM>
__device__ __forceinline__ bool lifted(const ArgsOf<TRIM>& A, const RecClass& c, u64 i) {
  if (c.kind != 2u || was_cut<TRIM>(A, i) || !live_pair<TRIM>(A, c)) return false;
  const bool simple = !c.contain && !c.self && A.deg[c.sq] == 1u && A.deg[c.st] == 1u;
  return !(simple && A.link[c.sq].x == c.st);
}

template <int TRIM>
__global__ __launch_bounds__(256) void k_lift_flag(ArgsOf<TRIM> A) {
  const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
  if (i >= A.n_edges) return;
  A.eflag[i] = lifted<TRIM>(A, classify(reinterpret_cast<const uint4*>(A.edges)[i], A), i) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_lift_write(UnitigTrimArgs A) {
  const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
  if (i >= A.n_edges || A.eflag[i] == 0u) return;
  const u64 at = A.escan[i];
  if (at >= A.n_edges) return;
  const uint4 rec = reinterpret_cast<const uint4*>(A.edges)[i];
  const RecClass c = classify(rec, A);  // (kept: the flag says so)
  const u32 mq = A.umap[c.sq >> 1], mt = A.umap[c.st >> 1];
  // read end e of a read placed reversed is the other end of its unitig
  const u32 eq = (c.sq ^ mq) & 1u, et = (c.st ^ mt) & 1u;
  const u32 b0 = eq == 0u, b1 = et == 1u;
  reinterpret_cast<uint4*>(A.uedges)[at] = make_uint4(mq >> 1, mt >> 1, rec.z, b0 | (b1 << 1) | ((b0 ^ b1) << 2));
}

__global__ void k_trim_status(UnitigTrimArgs A) {
  if (threadIdx.x != 0u || blockIdx.x != 0u) return;
  A.status[6] = rounds_ran(A.trim, TRIM_ROUND0);
  A.status[7] = counter_total(A.trim, TRIM_C_ISLANDS);
  A.status[8] = counter_total(A.trim, TRIM_C_DEAD_ENDS);
  A.status[9] = counter_total(A.trim, TRIM_C_READS);
  A.status[10] = counter_total(A.trim, TRIM_C_DROPPED);
  A.status[11] = A.uedges ? A.trim[TRIM_LIFTED] : 0ull;
}

// ---- non-maximal overlap cutting: one round's cut step (MaximumOverlapVisitor, src/bigraph_visitors.cpp:410-512) ----
// Before a cut step: the longest participant per read end back to 0 and, careful mode, the longest self record and the key table
// back to empty.  A kernel and no memset, so that the rounds after one that changed nothing do not write the table again.
__global__ __launch_bounds__(256) void k_prune_clear(UnitigPruneArgs A) {
  if (idle_round<2>(A)) return;
  const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
  if (i < 2 * A.n_reads) {
    A.maxlen[i] = 0u;
    if (A.careful) A.maxself[i] = 0u;
  }
  if (A.careful && i < A.key_cap) A.keys[i] = ~0ull;
}

// One lane per read.  A head scores its unitig: (N - K) (log(G - b) - log(G - 2 b)) - K log 2 in double, K its reads, b its
// bases; log(0.001) stands for the second logarithm when b < G <= 2 b, as in the reference; b >= G: not unique.
__global__ __launch_bounds__(256) void k_prune_unique(UnitigPruneArgs A) {
  if (idle_round<2>(A)) return;
  const u64 r = (u64)blockIdx.x * 256u + threadIdx.x;
  const u64 n = A.n_reads;
  u32 u = 0;
  if (r < n) {
    if (A.removed[r] == 0u && A.cnt[r] != 0u) {
      const u64 K = A.cnt[n + 1 + r], b = (u64)A.cnt[2 * (n + 1) + r] | ((u64)A.cnt[3 * (n + 1) + r] << 32);
      const u64 N = A.num_reads, G = A.genome_size;
      if (b < G && K <= N) {
        const u64 rest = G - b;  // G > 2 b  <=>  rest > b
        const double second = rest > b ? log((double)(rest - b)) : log(0.001);
        const double score = (double)(N - K) * (log((double)rest) - second) - (double)K * log(2.0);
        u = score >= A.uniq_threshold ? 1u : 0u;
      }
    }
    A.uniq[r] = u;
  }
  const u64 tu = wave_sum(u);
  if ((threadIdx.x & 63u) == 0u && tu && A.round == 1u) atomicAdd(counter_slot(A.prune, PRUNE_C_UNIQUE), tu);
}

// a participant of the cut step: live, and no containment -> its two read ends and its length
__device__ __forceinline__ bool participant(const UnitigPruneArgs& A, u64 i, u32& s, u32& t, u32& len) {
  const uint4 rec = reinterpret_cast<const uint4*>(A.edges)[i];
  const RecClass c = classify(rec, A);
  s = c.sq;
  t = c.st;
  len = rec.z;
  return c.kind == 2u && !c.contain && A.cut[i] == 0u && live_pair<2>(A, c);
}
__device__ __forceinline__ u64 key_hash(u64 k) {
  k ^= k >> 33;
  k *= 0xFF51AFD7ED558CCDull;
  k ^= k >> 33;
  k *= 0xC4CEB9FE1A85EC53ull;
  return k ^ (k >> 33);
}
__device__ __forceinline__ void key_insert(const UnitigPruneArgs& A, u64 key) {
  const u64 mask = A.key_cap - 1ull;
  u64 at = key_hash(key) & mask;
  for (u64 p = 0; p < A.key_cap; ++p, at = (at + 1ull) & mask) {  // (never more than key_cap probes; at most half the table fills)
    const u64 was = atomicCAS(&A.keys[at], ~0ull, key);
    if (was == ~0ull || was == key) return;
  }
}
__device__ __forceinline__ bool key_there(const UnitigPruneArgs& A, u64 key) {
  const u64 mask = A.key_cap - 1ull;
  u64 at = key_hash(key) & mask;
  for (u64 p = 0; p < A.key_cap; ++p, at = (at + 1ull) & mask) {
    const u64 is = A.keys[at];
    if (is == key) return true;
    if (is == ~0ull) return false;
  }
  return false;
}

// Careful mode, one lane per record: what holds a candidate back.
__global__ __launch_bounds__(256) void k_prune_keys(UnitigPruneArgs A, const uint4* __restrict__ rk) {
  if (idle_round<2>(A)) return;
  const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
  if (i >= A.n_edges) return;
  u32 s, t, len;
  if (!participant(A, i, s, t, len)) return;
  const u32 hs = head_of(A, rk, s), ht = head_of(A, rk, t);
  if (hs == NIL || ht == NIL) return;
  if (hs == ht) {
    atomicMax(&A.maxself[s], len);
    atomicMax(&A.maxself[t], len);
  }
  const u32 ms = A.maxlen[s], mt = A.maxlen[t];
  if ((ms > len ? ms - len : 0u) < A.delta) key_insert(A, ((u64)s << 32) | ht);
  if ((mt > len ? mt - len : 0u) < A.delta) key_insert(A, ((u64)t << 32) | hs);
}

// One lane per record: cut iff a candidate from one of its two sides and not held back on that side.
__global__ __launch_bounds__(256) void k_prune_cut(UnitigPruneArgs A, const uint4* __restrict__ rk) {
  if (idle_round<2>(A)) return;
  const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
  u32 cut = 0;
  u32 s, t, len;
  if (i < A.n_edges && participant(A, i, s, t, len)) {
    const u32 hs = head_of(A, rk, s), ht = head_of(A, rk, t);
    if (hs != NIL && ht != NIL) {
      const u32 ms = A.maxlen[s], mt = A.maxlen[t];
      bool from_s = A.uniq[hs] != 0u && (ms > len ? ms - len : 0u) >= A.delta;
      bool from_t = A.uniq[ht] != 0u && (mt > len ? mt - len : 0u) >= A.delta;
      if (A.careful) {
        if (hs == ht) {  // a self record of the unitig: held back where the longest at that end is one too
          if (from_s && A.maxself[s] == ms) from_s = false;
          if (from_t && A.maxself[t] == mt) from_t = false;
        } else {  // held back where, seen from the other end, the unitig it comes from is among the longest
          if (from_s && key_there(A, ((u64)t << 32) | hs)) from_s = false;
          if (from_t && key_there(A, ((u64)s << 32) | ht)) from_t = false;
        }
      }
      if (from_s || from_t) {
        A.cut[i] = A.round;
        cut = 1;
      }
    }
  }
  const u64 tc = wave_sum(cut);
  if ((threadIdx.x & 63u) == 0u && tc) {
    atomicAdd(counter_slot(A.prune, PRUNE_C_CUT), tc);
    A.trim[TRIM_ROUND0 + A.round] = 1ull;  // (every wave that writes here writes the same)
    A.prune[PRUNE_ROUND0 + A.round] = 1ull;
  }
}

__global__ void k_prune_status(UnitigPruneArgs A) {
  if (threadIdx.x != 0u || blockIdx.x != 0u) return;
  A.status[12] = counter_total(A.prune, PRUNE_C_CUT);
  A.status[13] = rounds_ran(A.prune, PRUNE_ROUND0);
  A.status[14] = counter_total(A.prune, PRUNE_C_UNIQUE);
  A.status[15] = 0ull;
}

// ---- chimeric unitig removal: one round's chimeric step (ChimericVisitor, src/bigraph_visitors.cpp:83-198) ----
// reads and bases of the unitig under head h (h < n_reads), as k_uni_heads left them
__device__ __forceinline__ u64 unit_reads(const UnitigArgs& A, u32 h) { return A.cnt[A.n_reads + 1 + h]; }
__device__ __forceinline__ u64 unit_bases(const UnitigArgs& A, u32 h) {
  return (u64)A.cnt[2 * (A.n_reads + 1) + h] | ((u64)A.cnt[3 * (A.n_reads + 1) + h] << 32);
}
__device__ __forceinline__ u64 chim_pack(u64 v, u32 h) { return ((v < 0xFFFFFFFFull ? v : 0xFFFFFFFFull) << 32) | h; }
// (the entry only ever falls: a stale read costs an atomic that changes nothing, never a missed minimum)
__device__ __forceinline__ void chim_min(u64* at, u64 v) {
  if (v < *at) atomicMin(at, v);
}

// Before a chimeric step: neighbours and minima back to empty.  A kernel, as k_prune_clear: idle rounds write nothing.
__global__ __launch_bounds__(256) void k_chim_clear(UnitigChimericArgs A) {
  if (idle_round<2>(A)) return;
  const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
  if (i >= 2 * A.n_reads) return;
  A.nbr[i] = NIL;
  A.minb[0][i] = ~0ull;
  A.minb[1][i] = ~0ull;
  A.mink[0][i] = ~0ull;
  A.mink[1][i] = ~0ull;
}

// One lane per record, a participant in both directions a -> b.  second = 0: an end of degree 1 learns its neighbour (its one
// record: a single writer), an end of degree >= 2 takes the minima over the unitigs at its records' other ends.  second = 1: the
// minima among the records whose unitig is not the first minimum's.
__global__ __launch_bounds__(256) void k_chim_minima(UnitigChimericArgs A, const uint4* __restrict__ rk, int second) {
  if (idle_round<2>(A)) return;
  const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
  if (i >= A.n_edges) return;
  u32 s, t, len;
  if (!participant(A, i, s, t, len)) return;
  const u32 hs = head_of(A, rk, s), ht = head_of(A, rk, t);
  if (hs == NIL || ht == NIL) return;
  const u64 bs = chim_pack(unit_bases(A, hs), hs), bt = chim_pack(unit_bases(A, ht), ht);
  const u64 ks = chim_pack(unit_reads(A, hs), hs), kt = chim_pack(unit_reads(A, ht), ht);
  for (int dir = 0; dir < 2; ++dir) {
    const u32 a = dir ? t : s, b = dir ? s : t, hb = dir ? hs : ht;
    const u64 vb = dir ? bs : bt, vk = dir ? ks : kt;
    const u32 da = A.deg[a];
    if (!second) {
      if (da == 1u) {
        A.nbr[a] = b;
      } else if (da >= 2u) {
        chim_min(&A.minb[0][a], vb);
        chim_min(&A.mink[0][a], vk);
      }
    } else if (da >= 2u) {
      if ((u32)A.minb[0][a] != hb) chim_min(&A.minb[1][a], vb);
      if ((u32)A.mink[0][a] != hb) chim_min(&A.mink[1][a], vk);
    }
  }
}

// good(p) for the unitig under head h with `bases` and K reads: U(p) unique under Tc (k_prune_unique left it), and every other
// unitig at p longer than bases + delta_c, or every one with more than K + 3 reads.  The minimum over the others is the second
// entry where the first names h itself.  All ones = no others: both hold.
__device__ __forceinline__ bool chim_good(const UnitigChimericArgs& A, const uint4* __restrict__ rk, u32 p, u32 h, u64 bases, u64 K) {
  const u32 hp = head_of(A, rk, p);
  if (hp == NIL || A.uniq[hp] == 0u) return false;
  u64 mb = A.minb[0][p], mk = A.mink[0][p];
  if (mb != ~0ull && (u32)mb == h) mb = A.minb[1][p];
  if (mk != ~0ull && (u32)mk == h) mk = A.mink[1][p];
  const bool by_bases = mb == ~0ull || (mb >> 32) > bases + (u64)A.chimeric_delta;
  const bool by_reads = mk == ~0ull || (mk >> 32) > K + 3ull;
  return by_bases || by_reads;
}

// One lane per read.  A head judges its unitig, its ends found as k_trim_decide finds them.
__global__ __launch_bounds__(256) void k_chim_decide(UnitigChimericArgs A, const uint4* __restrict__ rk) {
  if (idle_round<2>(A)) return;
  const u64 r = (u64)blockIdx.x * 256u + threadIdx.x;
  const u64 n = A.n_reads;
  u32 v = 0;
  if (r < n) {
    if (A.removed[r] == 0u && A.cnt[r] != 0u) {
      const u64 K = unit_reads(A, (u32)r), bases = unit_bases(A, (u32)r);
      const uint4 a0 = rk[2 * r], a1 = rk[2 * r + 1];
      const u32 d = head_dir(a0, a1);
      const u32 sl = 2u * (u32)r + d, sr = (d ? a0 : a1).y;
      const u64 L = A.min_chimeric_length, C = A.min_chimeric_coverage;
      if ((u64)sr < 2 * n && A.deg[sl] == 1u && A.deg[sr] == 1u && bases <= L &&
          (A.min_chimeric_coverage == TRIM_NO_COVERAGE || (K - 1ull) * (L ? L : 1ull) <= ((C ? C : 1ull) - 1ull) * bases)) {
        const u32 p = A.nbr[sl], q = A.nbr[sr];
        if ((u64)p < 2 * n && (u64)q < 2 * n && A.deg[p] >= 2u && A.deg[q] >= 2u &&
            (chim_good(A, rk, p, (u32)r, bases, K) || chim_good(A, rk, q, (u32)r, bases, K)))
          v = 1;
      }
    }
    A.verdict[r] = v;
  }
  const u64 tv = wave_sum(v);
  if ((threadIdx.x & 63u) == 0u && tv) atomicAdd(counter_slot(A.chim, CHIM_C_UNITIGS), tv);
}

__global__ void k_chim_status(UnitigChimericArgs A) {
  if (threadIdx.x != 0u || blockIdx.x != 0u) return;
  A.status[16] = counter_total(A.chim, CHIM_C_UNITIGS);
  A.status[17] = counter_total(A.chim, CHIM_C_READS);
  A.status[18] = rounds_ran(A.chim, CHIM_ROUND0);
  A.status[19] = 0ull;
}

// ---- bubble popping: one round's bubble step (the reference declares SmoothingVisitor and leaves it empty: the rules are sigax.h's) ----

// Before a bubble or an indel step (S): neighbours, group table and maxima back to empty, nothing appended to the step's list.  A
// kernel, as k_prune_clear.
template <class S>
__global__ __launch_bounds__(256) void k_arm_clear(typename S::Args A) {
  if (idle_round<2>(A)) return;
  const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
  if (i < 2 * A.n_reads) {
    A.bnbr[i] = NIL;
    A.blen[i] = 0u;
  }
  if (i < A.group_cap) {
    A.table[i] = NIL;
    A.best[i] = 0ull;
  }
  if (i == 0) S::block(A)[S::APPENDED] = 0ull;
}

// One lane per record, a participant in both directions a -> b: an end of degree 1 learns its neighbour and its record's length (its
// one record: a single writer).
__global__ __launch_bounds__(256) void k_bub_ends(UnitigBubbleArgs A) {
  if (idle_round<2>(A)) return;
  const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
  if (i >= A.n_edges) return;
  u32 s, t, len;
  if (!participant(A, i, s, t, len)) return;
  if (A.deg[s] == 1u) {
    A.bnbr[s] = t;
    A.blen[s] = len;
  }
  if (A.deg[t] == 1u) {
    A.bnbr[t] = s;
    A.blen[t] = len;
  }
}

// One lane per read, as k_uni_place finds its slot: {read | reversed << 31, the overlap with the read before it, where in the unitig
// the bases it adds begin}.  Those begins ascend along a unitig: k_bub_compare bisects on them.
__global__ __launch_bounds__(256) void k_bub_place(UnitigBubbleArgs A, const uint4* __restrict__ rk, const u64* __restrict__ dist) {
  if (idle_round<2>(A)) return;
  const u64 r = (u64)blockIdx.x * 256u + threadIdx.x;
  const u64 n = A.n_reads;
  if (r >= n || A.removed[r] != 0u) return;
  const u64* layr = A.scan + (n + 1);
  const uint4 a0 = rk[2 * r], a1 = rk[2 * r + 1];
  const u32 d = head_dir(a0, a1);
  const uint4 to = d ? a1 : a0;
  const u64 h = to.y >> 1;
  if (h >= n) return;
  const u64 slot = layr[h] + to.z;
  if (slot >= n) return;
  const uint2 lk = A.link[2 * r + d];
  const u32 skip = lk.x == NIL ? 0u : lk.y;
  const u64 from = dist[2 * r + d] + skip;
  A.where[slot] = make_uint4((u32)r | (d << 31), skip, (u32)from, (u32)(from >> 32));
}

// One lane per read.  A head judges whether its unitig is an arm that takes part, its ends found as k_chim_decide finds them.
__global__ __launch_bounds__(256) void k_bub_arms(UnitigBubbleArgs A, const uint4* __restrict__ rk) {
  if (idle_round<2>(A)) return;
  const u64 r = (u64)blockIdx.x * 256u + threadIdx.x;
  const u64 n = A.n_reads;
  if (r >= n) return;
  uint4 arm = make_uint4(0u, 0u, 0u, 0u);
  u32 side = 0;
  if (A.removed[r] == 0u && A.cnt[r] != 0u && A.closing[r] == 0u) {  // a head, and no ring
    const u64 bases = unit_bases(A, (u32)r);
    const uint4 a0 = rk[2 * r], a1 = rk[2 * r + 1];
    const u32 d = head_dir(a0, a1);
    const u32 sl = 2u * (u32)r + d, sr = (d ? a0 : a1).y;
    if ((u64)sr < 2 * n && A.deg[sl] == 1u && A.deg[sr] == 1u) {
      const u32 p = A.bnbr[sl], q = A.bnbr[sr];
      if ((u64)p < 2 * n && (u64)q < 2 * n && p != q && head_of(A, rk, p) != (u32)r && head_of(A, rk, q) != (u32)r) {
        side = p < q;
        const u32 o_lo = side ? A.blen[sl] : A.blen[sr], o_hi = side ? A.blen[sr] : A.blen[sl];
        const u64 ends = (u64)o_lo + o_hi;
        if (bases > ends && bases - ends <= (u64)A.max_bubble_span) arm = make_uint4(side ? p : q, side ? q : p, (u32)(bases - ends), o_lo);
      }
    }
  }
  A.arm[r] = arm;
  A.aside[r] = side;
  A.gslot[r] = NIL;
}

// One lane per read.  An arm that takes part finds the slot of its group -- the first free one on the probe path of its key, or the
// one an arm of that key opened -- and offers (K << 32) | ~head to the group's maximum.  arm[] is the kernel before's: stable.  The key
// is (lo, hi, span) in the bubble step (SPAN) and (lo, hi) alone in the indel step, where arms of every span that takes part meet in
// one group.
template <class ArgsT, bool SPAN>
__global__ __launch_bounds__(256) void k_arm_group(ArgsT A) {
  if (idle_round<2>(A)) return;
  const u64 r = (u64)blockIdx.x * 256u + threadIdx.x;
  if (r >= A.n_reads) return;
  const uint4 arm = A.arm[r];
  if (arm.z == 0u) return;
  const u64 mask = A.group_cap - 1ull;
  const u64 ends = ((u64)arm.x << 32) | arm.y;
  u64 at = key_hash(SPAN ? ends ^ key_hash(arm.z) : ends) & mask;
  for (u64 p = 0; p < A.group_cap; ++p, at = (at + 1ull) & mask) {  // (never more than group_cap probes; at most half the table fills)
    const u32 was = atomicCAS(&A.table[at], NIL, (u32)r);
    bool mine = was == NIL || was == (u32)r;
    if (!mine && (u64)was < A.n_reads) {
      const uint4 o = A.arm[was];
      mine = o.x == arm.x && o.y == arm.y && (!SPAN || o.z == arm.z);
    }
    if (mine) {
      A.gslot[r] = (u32)at;
      atomicMax(&A.best[at], (unit_reads(A, (u32)r) << 32) | (u64)(~(u32)r));
      return;
    }
  }
}

// One lane per read.  An arm that is not its group's maximum is a loser: without a bases test it is popped here, with one it is
// appended to the list k_bub_compare walks (a wave's losers behind one add).
__global__ __launch_bounds__(256) void k_bub_losers(UnitigBubbleArgs A) {
  if (idle_round<2>(A)) return;
  const u64 r = (u64)blockIdx.x * 256u + threadIdx.x;
  const u64 n = A.n_reads;
  const u32 lane = threadIdx.x & 63u;
  bool loser = false;
  if (r < n) {
    const u32 g = A.gslot[r];
    if ((u64)g < A.group_cap) loser = (u32)(~A.best[g]) != (u32)r;
  }
  const bool no_bases = A.max_divergence_permille == BUBBLE_NO_BASES;
  if (r < n) A.verdict[r] = loser && no_bases ? 1u : 0u;
  const u64 losers = __ballot(loser);
  if (!losers) return;
  if (no_bases) {
    if (lane == 0u) atomicAdd(counter_slot(A.bub, BUB_C_POPPED), (u64)__popcll(losers));
    return;
  }
  u64 base = 0;
  if (lane == 0u) base = atomicAdd(A.bub + BUB_APPENDED, (u64)__popcll(losers));
  base = __shfl(base, 0, 64);
  const u64 at = base + (u64)__popcll(losers & ((1ull << lane) - 1ull));
  if (loser && at < n) A.losers[at] = (u32)r;
}

// base o_lo + t of A(U), U the arm under head h: S(U) is read through the placements k_bub_place left, as the final pass would write
// it; an arm entered through its right end is read from its far end, complemented.
__device__ __forceinline__ u32 arm_base(const UnitigBubbleArgs& A, u32 h, const uint4 arm, u32 side, u64 t, u64 src_end) {
  const u64 n = A.n_reads, bases = unit_bases(A, h), K = unit_reads(A, h), first = A.scan[(n + 1) + h];
  const u64 in = (u64)arm.w + t;
  if (in >= bases || K == 0ull || first >= n) return 'N';  // (no consistent state comes here)
  const u64 x = side ? in : bases - 1ull - in;
  u64 a = 0, b = K < n - first ? K : n - first;  // the last placement that begins at or before x
  for (int step = 0; step < 32 && b - a > 1ull; ++step) {
    const u64 m = (a + b) >> 1;
    const uint4 e = A.where[first + m];
    if (((u64)e.z | ((u64)e.w << 32)) <= x) a = m;
    else b = m;
  }
  const uint4 e = A.where[first + a];
  const u64 r = e.x & 0x7FFFFFFFu, from = (u64)e.z | ((u64)e.w << 32);
  const u32 rev = e.x >> 31;
  if (r >= n || from < e.y || x < from - e.y) return 'N';
  const u64 j = x - (from - e.y), L = A.lengths[r];
  if (j >= L) return 'N';
  const u64 at = A.offs[r] + (rev ? L - 1ull - j : j);
  if (at >= src_end) return 'N';
  u32 c = A.seqs[at];
  if (rev) c = comp_byte(c);
  return side ? c : comp_byte(c);
}

// One wave per appended loser, the grid's W waves striding over the list (at most n_reads / W + 1 turns); lanes stride over the window (at most
// Lb / 64 + 1 turns).  Popped iff mism * 1000 <= D * span.
__global__ __launch_bounds__(256) void k_bub_compare(UnitigBubbleArgs A) {
  if (idle_round<2>(A)) return;
  const u64 n = A.n_reads;
  const u32 wave = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u, waves = gridDim.x * 4u;
  u64 appended = A.bub[BUB_APPENDED];
  if (appended > n) appended = n;
  const u64 src_end = A.offs[n];
  u64 popped = 0, kept = 0;
  for (u64 i = wave; i < appended; i += waves) {
    const u32 h = A.losers[i];
    if ((u64)h >= n) continue;
    const u32 g = A.gslot[h];
    if ((u64)g >= A.group_cap) continue;
    const u32 w = (u32)(~A.best[g]);
    if ((u64)w >= n) continue;
    const uint4 al = A.arm[h], aw = A.arm[w];
    const u32 sl = A.aside[h], sw = A.aside[w];
    const u64 span = al.z < A.max_bubble_span ? al.z : A.max_bubble_span;
    u64 mism = 0;
    for (u64 t = lane; t < span; t += 64) mism += arm_base(A, h, al, sl, t, src_end) != arm_base(A, w, aw, sw, t, src_end);
    mism = wave_sum(mism);
    if (mism * 1000ull <= (u64)A.max_divergence_permille * span) {
      if (lane == 0u) A.verdict[h] = 1u;
      ++popped;
    } else {
      ++kept;
    }
  }
  if (lane == 0u) {
    if (popped) atomicAdd(counter_slot(A.bub, BUB_C_POPPED), popped);
    if (kept) atomicAdd(counter_slot(A.bub, BUB_C_KEPT), kept);
  }
}

__global__ void k_bub_status(UnitigBubbleArgs A) {
  if (threadIdx.x != 0u || blockIdx.x != 0u) return;
  A.status[20] = counter_total(A.bub, BUB_C_POPPED);
  A.status[21] = counter_total(A.bub, BUB_C_READS);
  A.status[22] = rounds_ran(A.bub, BUB_ROUND0);
  A.status[23] = counter_total(A.bub, BUB_C_KEPT);
}

// ---- indel bubble popping: one round's indel step, after the bubble step (the rules are sigax.h's own, as the bubble step's) ----

// One lane per read.  An arm that is not its group's maximum is a loser: of the winner's span (the bubble step's business) or more
// than max_edits bases from it, it stays and is counted; otherwise it is appended to the list k_ind_compare walks.
__global__ __launch_bounds__(256) void k_ind_losers(UnitigIndelArgs A) {
  if (idle_round<2>(A)) return;
  const u64 r = (u64)blockIdx.x * 256u + threadIdx.x;
  const u64 n = A.n_reads;
  const u32 lane = threadIdx.x & 63u;
  bool loser = false, compared = false;
  if (r < n) {
    A.verdict[r] = 0u;
    const u32 g = A.gslot[r];
    if ((u64)g < A.group_cap) {
      const u32 w = (u32)(~A.best[g]);
      if (w != (u32)r && (u64)w < n) {
        loser = true;
        const u32 a = A.arm[r].z, b = A.arm[w].z;
        compared = a != b && (a > b ? a - b : b - a) <= A.max_edits;
      }
    }
  }
  const u64 skipped = __ballot(loser && !compared), listed = __ballot(compared);
  if (lane == 0u && skipped) atomicAdd(counter_slot(A.ind, IND_C_SKIPPED), (u64)__popcll(skipped));
  if (!listed) return;
  u64 base = 0;
  if (lane == 0u) base = atomicAdd(A.ind + IND_APPENDED, (u64)__popcll(listed));
  base = __shfl(base, 0, 64);
  const u64 at = base + (u64)__popcll(listed & ((1ull << lane) - 1ull));
  if (compared && at < n) A.pairs[at] = (u32)r;
}

// the two windows of a pair, as bytes: X the loser's, Y the winner's
struct IndelSh {
  unsigned char x[IND_MAX_SPAN], y[IND_MAX_SPAN];
};

// One wave (one workgroup of 64) per appended pair, the grid striding over the list (at most n_reads / W + 1 turns).  Both windows are
// staged in LDS through arm_base, one bisection per base.  Then the furthest-reaching recurrence over diagonals (Landau-Vishkin):
// lane l owns diagonal d = l - E of the (loser, winner) matrix, column - row = d, and after turn e holds the furthest row that at most e
// edits reach on it, or a negative value where none does.  A turn takes the two neighbours' reach by shuffles, keeps what stays
// inside the matrix, and slides while the bytes agree (at most Lb steps).  At most E + 1 turns; the distance is the first e at which
// diagonal b - a reaches row a.  Popped iff ed <= E and ed * 1000 <= De * min(bases(L), bases(W)).
__global__ __launch_bounds__(64) void k_ind_compare(UnitigIndelArgs A) {
  __shared__ IndelSh sh;
  if (idle_round<2>(A)) return;
  const u64 n = A.n_reads;
  const u32 lane = threadIdx.x & 63u;
  const int E = (int)(A.max_edits < (u32)IND_MAX_EDITS ? A.max_edits : (u32)IND_MAX_EDITS);
  const int NONE = -0x40000000;
  u64 appended = A.ind[IND_APPENDED];
  if (appended > n) appended = n;
  const u64 src_end = A.offs[n];
  u64 popped = 0, kept = 0;
  for (u64 i = blockIdx.x; i < appended; i += gridDim.x) {  // (every value that decides a branch here is the same in all lanes)
    const u32 h = A.pairs[i];
    if ((u64)h >= n) continue;
    const u32 g = A.gslot[h];
    if ((u64)g >= A.group_cap) continue;
    const u32 w = (u32)(~A.best[g]);
    if ((u64)w >= n) continue;
    const uint4 al = A.arm[h], aw = A.arm[w];
    const u32 sl = A.aside[h], sw = A.aside[w];
    if (al.z == 0u || aw.z == 0u || al.z > (u32)IND_MAX_SPAN || aw.z > (u32)IND_MAX_SPAN) continue;
    const int a = (int)al.z, b = (int)aw.z;
    if (a - b > E || b - a > E) continue;
    for (u32 t = lane; t < al.z; t += 64) sh.x[t] = (unsigned char)arm_base(A, h, al, sl, t, src_end);
    for (u32 t = lane; t < aw.z; t += 64) sh.y[t] = (unsigned char)arm_base(A, w, aw, sw, t, src_end);
    __syncthreads();
    const int d = (int)lane - E, lim = a < b - d ? a : b - d;  // rows of diagonal d end at lim
    int fr = NONE;
    u32 ed = (u32)E + 1u;
    for (int e = 0; e <= E; ++e) {
      int t;
      if (e == 0) {
        t = d == 0 ? 0 : NONE;
      } else {
        int up = __shfl_up(fr, 1, 64), dn = __shfl_down(fr, 1, 64);  // diagonals d - 1 and d + 1
        if (lane == 0u) up = NONE;
        if (lane == 63u) dn = NONE;
        t = fr >= 0 && fr < lim ? fr + 1 : fr;             // a substitution
        if (up >= 0 && up + d <= b && up > t) t = up;      // a base the winner has and the loser lacks
        if (dn >= 0 && dn < a && dn + 1 > t) t = dn + 1;   // a base the loser has and the winner lacks
      }
      if (lane > 2u * (u32)E) t = NONE;
      if (t >= 0)
        while (t < lim && (u32)(t + d) < (u32)b && sh.x[t] == sh.y[t + d]) ++t;
      fr = t;
      if (__shfl(fr, b - a + E, 64) >= a) {
        ed = (u32)e;
        break;
      }
    }
    __syncthreads();  // (the next pair's bytes go where these lie)
    const u64 bl = unit_bases(A, h), bw = unit_bases(A, w);
    if (ed <= (u32)E && (u64)ed * 1000ull <= (u64)A.max_edit_permille * (bl < bw ? bl : bw)) {
      if (lane == 0u) A.verdict[h] = 1u;
      ++popped;
    } else {
      ++kept;
    }
  }
  if (lane == 0u) {
    if (popped) atomicAdd(counter_slot<1>(A.ind, IND_C_POPPED), popped);
    if (kept) atomicAdd(counter_slot<1>(A.ind, IND_C_KEPT), kept);
  }
}

__global__ void k_ind_status(UnitigIndelArgs A) {
  if (threadIdx.x != 0u || blockIdx.x != 0u) return;
  A.status[24] = counter_total(A.ind, IND_C_POPPED);
  A.status[25] = counter_total(A.ind, IND_C_READS);
  A.status[26] = rounds_ran(A.ind, IND_ROUND0);
  A.status[27] = counter_total(A.ind, IND_C_KEPT);
  A.status[28] = counter_total(A.ind, IND_C_SKIPPED);
  A.status[29] = A.status[30] = A.status[31] = 0ull;
}

// ---- transitive reduction: one pass (the rules in include/sigax.h; nothing of it is in the reference, whose
// TransitiveReductionVisitor is empty) ----
// a pass after a round that changed nothing has nothing to do: the flags of the pass before still hold
__device__ __forceinline__ bool red_idle(const UnitigReduceArgs& A) {
  return A.red_prev >= 1u && A.red_prev <= (u32)TRIM_MAX_ROUNDS && A.trim[TRIM_ROUND0 + A.red_prev] == 0ull;
}
// a participant of a pass: kept, both reads alive, not cut in an earlier round (k_red_clear has taken bit 31 off), neither a
// containment nor a self edge -> its two read ends and its length
__device__ __forceinline__ bool red_participant(const UnitigReduceArgs& A, u64 i, u32& a, u32& b, u32& len) {
  const uint4 rec = reinterpret_cast<const uint4*>(A.edges)[i];
  const RecClass c = classify(rec, A);
  a = c.sq;
  b = c.st;
  len = rec.z;
  return c.kind == 2u && !c.contain && !c.self && A.cut[i] == 0u && live_pair<2>(A, c);
}
// The table's key is (the smaller state, the larger state, overlap): 96 bits, so a slot names a participant record and a probe
// compares against that record's own fields.  A record that went in was classified: its states follow from q, t and af alone.
__device__ __forceinline__ u64 red_hash(u32 lo, u32 hi, u32 len) { return key_hash((((u64)lo << 32) | hi) ^ ((u64)len * 0x9E3779B97F4A7C15ull)); }
__device__ __forceinline__ bool red_same(const UnitigReduceArgs& A, u32 j, u32 lo, u32 hi, u32 len) {
  if ((u64)j >= A.n_edges) return false;
  const uint4 rec = reinterpret_cast<const uint4*>(A.edges)[j];
  if (rec.z != len) return false;
  const u32 sq = 2u * rec.x + ((rec.w & 1u) ? 0u : 1u), st = 2u * rec.y + ((rec.w & 2u) ? 1u : 0u);
  return (sq == lo && st == hi) || (sq == hi && st == lo);
}
__device__ __forceinline__ void red_insert(const UnitigReduceArgs& A, u32 i, u32 s, u32 t, u32 len) {
  const u32 lo = s < t ? s : t, hi = s < t ? t : s;
  const u64 mask = A.red_cap - 1ull;
  u64 at = red_hash(lo, hi, len) & mask;
  for (u64 p = 0; p < A.red_cap; ++p, at = (at + 1ull) & mask) {  // (never more than red_cap probes; at most a quarter of the table fills)
    const u32 was = atomicCAS(&A.rtable[at], NIL, i);
    if (was == NIL || was == i || red_same(A, was, lo, hi, len)) return;  // (a second record of the same key: the key is there)
  }
}
__device__ __forceinline__ bool red_there(const UnitigReduceArgs& A, u32 s, u32 t, u32 len) {
  const u32 lo = s < t ? s : t, hi = s < t ? t : s;
  const u64 mask = A.red_cap - 1ull;
  u64 at = red_hash(lo, hi, len) & mask;
  for (u64 p = 0; p < A.red_cap; ++p, at = (at + 1ull) & mask) {
    const u32 is = A.rtable[at];
    if (is == NIL) return false;
    if (red_same(A, is, lo, hi, len)) return true;
  }
  return false;
}

// Before a pass: bit 31 off every cut[i], no participant counted, no entry written, the table empty, the pass's counters zero.  A
// kernel and no memset, so that an idle pass writes nothing and the flags of the pass before hold.
__global__ __launch_bounds__(256) void k_red_clear(UnitigReduceArgs A) {
  if (red_idle(A)) return;
  const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
  if (i < A.n_edges) {
    const u32 c = A.cut[i];
    if (c & CUT_TRANSITIVE) A.cut[i] = c & ~CUT_TRANSITIVE;
  }
  if (i <= 2 * A.n_reads) A.rcnt[i] = 0u;
  if (i < 2 * A.n_reads) A.rfill[i] = 0u;
  if (i < A.red_cap) A.rtable[i] = NIL;
  if (i < (u64)RED_FIRST) A.red[i] = 0ull;
}

// One lane per record: a participant counts at both its states.
__global__ __launch_bounds__(256) void k_red_count(UnitigReduceArgs A) {
  if (red_idle(A)) return;
  const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
  u32 a, b, len;
  if (i >= A.n_edges || !red_participant(A, i, a, b, len)) return;
  atomicAdd(&A.rcnt[a], 1u);
  atomicAdd(&A.rcnt[b], 1u);
}

// One lane per record: a participant writes {other state, extension towards it} into the segments of both its states (the order
// inside a segment is whatever the atomics give; no verdict depends on it) and its key into the table.
__global__ __launch_bounds__(256) void k_red_fill(UnitigReduceArgs A) {
  if (red_idle(A)) return;
  const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
  u32 a, b, len;
  if (i >= A.n_edges || !red_participant(A, i, a, b, len)) return;
  const u64 cap = 2 * A.n_edges;
  const u64 ka = A.roff[a] + atomicAdd(&A.rfill[a], 1u), kb = A.roff[b] + atomicAdd(&A.rfill[b], 1u);
  if (ka < cap) A.radj[ka] = make_uint2(b, A.lengths[b >> 1] - len);
  if (kb < cap) A.radj[kb] = make_uint2(a, A.lengths[a >> 1] - len);
  red_insert(A, (u32)i, a, b, len);
}

// Is the participant of overlap len between a and b, ext = ext(a -> b), explained seen from a?  Over the segment of a: a state w of a
// third read with ext(a -> w) < ext, and then the one key that closes the triangle: (w ^ 1, b, len + ext(a -> w)), since
// ext(a -> w) + (L[b] - len_k) == L[b] - len  <=>  len_k == len + ext(a -> w).  The trip count is a's degree; each probe is bounded by
// the table's capacity.
__device__ __forceinline__ bool red_explained(const UnitigReduceArgs& A, u32 a, u32 b, u32 ext, u32 len) {
  const u64 cap = 2 * A.n_edges;
  u64 k = A.roff[a], end = A.roff[a + 1u];
  if (end > cap) end = cap;
  for (; k < end; ++k) {
    const uint2 e = A.radj[k];
    if (e.y >= ext || (e.x >> 1) == (b >> 1) || (e.x >> 1) == (a >> 1)) continue;
    if (red_there(A, e.x ^ 1u, b, len + e.y)) return true;
  }
  return false;
}

// One lane per record: a participant is flagged iff it is explained seen from either of its ends.  Witnesses are looked up in what
// k_red_fill left, which no lane of this kernel writes: the verdicts do not depend on each other.
__global__ __launch_bounds__(256) void k_red_walk(UnitigReduceArgs A) {
  if (red_idle(A)) return;
  const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
  u32 part = 0, flagged = 0;
  u32 a, b, len;
  if (i < A.n_edges && red_participant(A, i, a, b, len)) {
    part = 1;
    if (red_explained(A, a, b, A.lengths[b >> 1] - len, len) || red_explained(A, b, a, A.lengths[a >> 1] - len, len)) {
      A.cut[i] = CUT_TRANSITIVE;  // (a participant's cut[i] was 0)
      flagged = 1;
    }
  }
  const u64 tp = wave_sum(part), tf = wave_sum(flagged);
  if ((threadIdx.x & 63u) == 0u) {
    if (tp) atomicAdd(counter_slot(A.red, RED_C_PART), tp);
    if (tf) atomicAdd(counter_slot(A.red, RED_C_FLAGGED), tf);
  }
}

// After a pass that ran: its counts become the call's "latest", and the call's "first" if none ran before.
__global__ void k_red_note(UnitigReduceArgs A) {
  if (threadIdx.x != 0u || blockIdx.x != 0u || red_idle(A)) return;
  const u64 f = counter_total(A.red, RED_C_FLAGGED);
  if (A.red[RED_PASSES] == 0ull) A.red[RED_FIRST] = f;
  A.red[RED_LAST] = f;
  A.red[RED_LAST_PART] = counter_total(A.red, RED_C_PART);
  A.red[RED_PASSES] += 1ull;
}

__global__ void k_red_status(UnitigReduceArgs A) {
  if (threadIdx.x != 0u || blockIdx.x != 0u) return;
  A.status[32] = A.red[RED_FIRST];
  A.status[33] = A.red[RED_LAST];
  A.status[34] = A.red[RED_PASSES];
  A.status[35] = A.red[RED_LAST_PART];
  A.status[36] = A.status[37] = A.status[38] = A.status[39] = 0ull;
}

// degrees, links, ranking, ring cut, ranking again -> which of the two ranking buffers holds the result
template <int TRIM>
unsigned launch_graph(const ArgsOf<TRIM>& a, hipStream_t st) {
  const u64 n = a.n_reads, ns = 2 * n;
  if (a.n_edges) {
    hipLaunchKernelGGL(k_uni_degree<TRIM>, dim3(blocks_of(a.n_edges)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_uni_links<TRIM>, dim3(blocks_of(a.n_edges)), dim3(256), 0, st, a);
  }
  const unsigned rounds = unitig_rounds(n);
  uint4* rk[2] = {reinterpret_cast<uint4*>(a.rank[0]), reinterpret_cast<uint4*>(a.rank[1])};
  for (int pass = 0; pass < 2; ++pass) {
    hipLaunchKernelGGL(k_uni_init<TRIM>, dim3(blocks_of(ns)), dim3(256), 0, st, a, rk[0], a.dist[0], pass);
    for (unsigned r = 0; r < rounds; ++r)
      hipLaunchKernelGGL(k_uni_jump<TRIM>, dim3(blocks_of(ns)), dim3(256), 0, st, a, (const uint4*)rk[r & 1], (const u64*)a.dist[r & 1], rk[(r & 1) ^ 1],
                         a.dist[(r & 1) ^ 1], pass);
    if (pass == 0) hipLaunchKernelGGL(k_uni_cut<TRIM>, dim3(blocks_of(n)), dim3(256), 0, st, a, (const uint4*)rk[rounds & 1]);
  }
  return rounds & 1;
}

template <int TRIM>
void launch_unitigs_t(const ArgsOf<TRIM>& a, hipStream_t st) {
  const u64 n = a.n_reads;
  const unsigned f = launch_graph<TRIM>(a, st);
  const uint4* fin = reinterpret_cast<const uint4*>(a.rank[f]);
  const u64* fdist = a.dist[f];
  hipLaunchKernelGGL(k_uni_heads<TRIM>, dim3(blocks_of(n)), dim3(256), 0, st, a, fin, fdist);
  for (int k = 0; k < 4; ++k) launch_scan(a.cnt + (u64)k * (n + 1), n, a.partial, a.scan + (u64)k * (n + 1), a.scan_total, st);
  hipLaunchKernelGGL(k_uni_place<TRIM>, dim3(blocks_of(n)), dim3(256), 0, st, a, fin, fdist);
  if (a.useqs) hipLaunchKernelGGL(k_uni_bases<TRIM>, dim3(blocks_of(n)), dim3(256), 0, st, a);
}

// what every step of a round asks of its block: reads, removed[], and a round the flags have a word for
bool step_ok(const UnitigTrimArgs& a) { return a.n_reads != 0 && a.removed && a.round != 0u && a.round <= TRIM_MAX_ROUNDS; }

// how every step of a round begins: the graph of the live records and the heads of its unitigs -> the final rank buffer and the
// distances that go with it
struct StepGraph {
  const uint4* rk;
  const u64* dist;
};
template <int TRIM>
StepGraph launch_step_graph(const ArgsOf<TRIM>& a, hipStream_t st) {
  const unsigned f = launch_graph<TRIM>(a, st);
  const StepGraph g = {reinterpret_cast<const uint4*>(a.rank[f]), a.dist[f]};
  hipLaunchKernelGGL(k_uni_heads<TRIM>, dim3(blocks_of(a.n_reads)), dim3(256), 0, st, a, g.rk, g.dist);
  return g;
}

// a round's trim step: TRIM = 1 over the trim block, TRIM = 2 over the records that are not cut (never with a.maxlen set: that is a cut step)
template <int TRIM>
void launch_trim_round_t(const ArgsOf<TRIM>& a, hipStream_t st) {
  const u64 n = a.n_reads;
  if (!step_ok(a)) return;
  if constexpr (TRIM == 2)
    if (a.maxlen) return;
  const uint4* fin = launch_step_graph<TRIM>(a, st).rk;
  hipLaunchKernelGGL(k_trim_decide, dim3(blocks_of(n)), dim3(256), 0, st, static_cast<const UnitigTrimArgs&>(a), fin);
  hipLaunchKernelGGL(k_step_mark<TrimStep>, dim3(blocks_of(n)), dim3(256), 0, st, static_cast<const UnitigTrimArgs&>(a), fin);
}

// a step's status words, by its one-lane kernel
template <class K, class ArgsT>
void launch_status(K kernel, const ArgsT& a, hipStream_t st) {
  if (a.n_reads == 0 || !a.removed) return;
  hipLaunchKernelGGL(kernel, dim3(1), dim3(64), 0, st, a);
}

// the lifted records and status[6 .. 11]; TRIM = 2: without the cut records, and status[12 .. 15]
template <int TRIM>
void launch_lift_t(const ArgsOf<TRIM>& a, hipStream_t st) {
  if (a.n_reads == 0 || !a.removed) return;
  if (a.uedges && a.n_edges) {
    hipLaunchKernelGGL(k_lift_flag<TRIM>, dim3(blocks_of(a.n_edges)), dim3(256), 0, st, a);
    launch_scan(a.eflag, a.n_edges, a.epartial, a.escan, a.trim + TRIM_LIFTED, st);
    hipLaunchKernelGGL(k_lift_write, dim3(blocks_of(a.n_edges)), dim3(256), 0, st, static_cast<const UnitigTrimArgs&>(a));
  }
  hipLaunchKernelGGL(k_trim_status, dim3(1), dim3(64), 0, st, static_cast<const UnitigTrimArgs&>(a));
  if constexpr (TRIM == 2) hipLaunchKernelGGL(k_prune_status, dim3(1), dim3(64), 0, st, a);
}
}  // namespace

unsigned unitig_rounds(unsigned long long n_reads) {
  unsigned r = 0;
  while ((1ull << r) < n_reads) ++r;  // ceil(log2 n)
  return r + 1;
}

void launch_unitigs(const UnitigArgs& a, hipStream_t st) {
  if (a.n_reads) launch_unitigs_t<0>(a, st);
}

void launch_unitigs_trim(const UnitigTrimArgs& a, hipStream_t st) {
  if (a.n_reads && a.removed) launch_unitigs_t<1>(a, st);
}

void launch_unitig_bases(const UnitigArgs& a, hipStream_t st) {
  if (a.n_reads && a.useqs) hipLaunchKernelGGL(k_uni_bases<0>, dim3(blocks_of(a.n_reads)), dim3(256), 0, st, a);
}

void launch_trim_round(const UnitigTrimArgs& a, hipStream_t st) { launch_trim_round_t<1>(a, st); }

void launch_unitig_lift(const UnitigTrimArgs& a, hipStream_t st) { launch_lift_t<1>(a, st); }

void launch_prune_cut_round(const UnitigPruneArgs& a, hipStream_t st) {
  const u64 n = a.n_reads;
  if (!step_ok(a) || !a.maxlen) return;
  const u64 lanes = a.careful && a.key_cap > 2 * n ? a.key_cap : 2 * n;
  hipLaunchKernelGGL(k_prune_clear, dim3(blocks_of(lanes)), dim3(256), 0, st, a);
  const uint4* fin = launch_step_graph<2>(a, st).rk;
  hipLaunchKernelGGL(k_prune_unique, dim3(blocks_of(n)), dim3(256), 0, st, a);
  if (a.n_edges == 0) return;  // (unitigs are scored and counted all the same)
  if (a.careful) hipLaunchKernelGGL(k_prune_keys, dim3(blocks_of(a.n_edges)), dim3(256), 0, st, a, fin);
  hipLaunchKernelGGL(k_prune_cut, dim3(blocks_of(a.n_edges)), dim3(256), 0, st, a, fin);
}

void launch_prune_trim_round(const UnitigPruneArgs& a, hipStream_t st) { launch_trim_round_t<2>(a, st); }

void launch_unitigs_prune(const UnitigPruneArgs& a, hipStream_t st) {
  if (a.n_reads && a.removed && !a.maxlen) launch_unitigs_t<2>(a, st);
}

void launch_unitig_prune_lift(const UnitigPruneArgs& a, hipStream_t st) { launch_lift_t<2>(a, st); }

void launch_chimeric_round(const UnitigChimericArgs& a, hipStream_t st) {
  const u64 n = a.n_reads;
  if (!step_ok(a) || a.maxlen || !a.nbr) return;
  hipLaunchKernelGGL(k_chim_clear, dim3(blocks_of(2 * n)), dim3(256), 0, st, a);
  const uint4* fin = launch_step_graph<2>(a, st).rk;
  UnitigPruneArgs score = a;  // the cut step's scoring kernel, under the chimeric threshold, counting aside
  score.uniq_threshold = a.chimeric_threshold;
  score.prune = a.prune_aside;
  hipLaunchKernelGGL(k_prune_unique, dim3(blocks_of(n)), dim3(256), 0, st, score);
  if (a.n_edges) {
    hipLaunchKernelGGL(k_chim_minima, dim3(blocks_of(a.n_edges)), dim3(256), 0, st, a, fin, 0);
    hipLaunchKernelGGL(k_chim_minima, dim3(blocks_of(a.n_edges)), dim3(256), 0, st, a, fin, 1);
  }
  hipLaunchKernelGGL(k_chim_decide, dim3(blocks_of(n)), dim3(256), 0, st, a, fin);
  hipLaunchKernelGGL(k_step_mark<ChimStep>, dim3(blocks_of(n)), dim3(256), 0, st, a, fin);
}

void launch_chimeric_status(const UnitigChimericArgs& a, hipStream_t st) { launch_status(k_chim_status, a, st); }

void launch_bubble_round(const UnitigBubbleArgs& a, hipStream_t st) {
  const u64 n = a.n_reads;
  if (!step_ok(a) || a.maxlen || !a.bnbr || !a.where || a.max_bubble_span == 0u) return;
  hipLaunchKernelGGL(k_arm_clear<BubStep>, dim3(blocks_of(a.group_cap > 2 * n ? a.group_cap : 2 * n)), dim3(256), 0, st, a);
  const StepGraph g = launch_step_graph<2>(a, st);
  const uint4* fin = g.rk;
  if (a.n_edges) hipLaunchKernelGGL(k_bub_ends, dim3(blocks_of(a.n_edges)), dim3(256), 0, st, a);
  const bool bases_test = a.max_divergence_permille != BUBBLE_NO_BASES;
  if (bases_test) {  // where each unitig's placements begin (the scan has no idle form: after an idle round nothing reads its result)
    launch_scan(a.cnt + (n + 1), n, a.partial, a.scan + (n + 1), a.scan_total, st);
    hipLaunchKernelGGL(k_bub_place, dim3(blocks_of(n)), dim3(256), 0, st, a, fin, g.dist);
  }
  hipLaunchKernelGGL(k_bub_arms, dim3(blocks_of(n)), dim3(256), 0, st, a, fin);
  hipLaunchKernelGGL((k_arm_group<UnitigBubbleArgs, true>), dim3(blocks_of(n)), dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_bub_losers, dim3(blocks_of(n)), dim3(256), 0, st, a);
  if (bases_test) {
    const u32 waves = (u32)(n < BUB_COMPARE_WAVES ? n : BUB_COMPARE_WAVES);
    hipLaunchKernelGGL(k_bub_compare, dim3((waves + 3u) / 4u), dim3(256), 0, st, a);
  }
  hipLaunchKernelGGL(k_step_mark<BubStep>, dim3(blocks_of(n)), dim3(256), 0, st, a, fin);
}

void launch_bubble_status(const UnitigBubbleArgs& a, hipStream_t st) { launch_status(k_bub_status, a, st); }

void launch_indel_round(const UnitigIndelArgs& a, hipStream_t st) {
  const u64 n = a.n_reads;
  if (!step_ok(a) || a.maxlen || !a.bnbr || !a.where || !a.pairs || !a.ind || a.max_bubble_span == 0u || a.max_bubble_span > (u32)IND_MAX_SPAN ||
      a.max_edits == 0u || a.max_edits > (u32)IND_MAX_EDITS)
    return;
  hipLaunchKernelGGL(k_arm_clear<IndStep>, dim3(blocks_of(a.group_cap > 2 * n ? a.group_cap : 2 * n)), dim3(256), 0, st, a);
  const UnitigBubbleArgs& ba = a;  // the bubble step's own kernels, over the block they know
  const StepGraph g = launch_step_graph<2>(a, st);
  const uint4* fin = g.rk;
  if (a.n_edges) hipLaunchKernelGGL(k_bub_ends, dim3(blocks_of(a.n_edges)), dim3(256), 0, st, ba);
  launch_scan(a.cnt + (n + 1), n, a.partial, a.scan + (n + 1), a.scan_total, st);  // (no idle form, as in the bubble step)
  hipLaunchKernelGGL(k_bub_place, dim3(blocks_of(n)), dim3(256), 0, st, ba, fin, g.dist);
  hipLaunchKernelGGL(k_bub_arms, dim3(blocks_of(n)), dim3(256), 0, st, ba, fin);
  hipLaunchKernelGGL((k_arm_group<UnitigIndelArgs, false>), dim3(blocks_of(n)), dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_ind_losers, dim3(blocks_of(n)), dim3(256), 0, st, a);
  hipLaunchKernelGGL(k_ind_compare, dim3((unsigned)(n < BUB_COMPARE_WAVES ? n : BUB_COMPARE_WAVES)), dim3(64), 0, st, a);
  hipLaunchKernelGGL(k_step_mark<IndStep>, dim3(blocks_of(n)), dim3(256), 0, st, a, fin);
}

void launch_indel_status(const UnitigIndelArgs& a, hipStream_t st) {
  if (a.ind) launch_status(k_ind_status, a, st);
}

void launch_reduce_pass(const UnitigReduceArgs& a, hipStream_t st) {
  const u64 n = a.n_reads, ne = a.n_edges;
  if (n == 0 || !a.removed || a.maxlen || !a.red || !a.rcnt || !a.rfill || !a.roff || !a.rpartial || !a.rtotal || !a.rtable || a.red_cap < 16 ||
      (a.red_cap & (a.red_cap - 1)) || a.red_cap < 4 * ne || ne >= (1ull << 32) || (ne && (!a.cut || !a.radj)) || a.red_prev > TRIM_MAX_ROUNDS)
    return;
  u64 lanes = a.red_cap > 2 * n + 1 ? a.red_cap : 2 * n + 1;
  if (lanes < (u64)RED_FIRST) lanes = RED_FIRST;
  hipLaunchKernelGGL(k_red_clear, dim3(blocks_of(lanes)), dim3(256), 0, st, a);
  if (ne) {
    hipLaunchKernelGGL(k_red_count, dim3(blocks_of(ne)), dim3(256), 0, st, a);
    launch_scan(a.rcnt, 2 * n, a.rpartial, a.roff, a.rtotal, st);  // (no idle form: after an idle pass's launch nothing reads its result)
    hipLaunchKernelGGL(k_red_fill, dim3(blocks_of(ne)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_red_walk, dim3(blocks_of(ne)), dim3(256), 0, st, a);
  }
  hipLaunchKernelGGL(k_red_note, dim3(1), dim3(64), 0, st, a);
}

void launch_reduce_status(const UnitigReduceArgs& a, hipStream_t st) {
  if (a.red) launch_status(k_red_status, a, st);
}
