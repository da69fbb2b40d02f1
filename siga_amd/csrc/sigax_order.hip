// siga_amd/csrc/sigax_order.hip -- the edge records of key-sharded runs back in read order.
//
// Under key-range sharding a batch runs its reads under their own ids (sigax_batch_*_read_ids), so the records a batch emits
// follow the batch's order of reads, not the file's, and the concatenation of several batches' records (one process after
// the other, or sigax_gather_edges) is a permutation of the one-batch ED list.  What it keeps: every read is run in exactly
// one batch, and a batch emits all records of one query contiguously, in hits order.  So every query owns ONE contiguous run
// of the list, and the one-batch order is the stable sort of the list by `query` -- which needs no sort:
//   runs    one lane per record: a record whose predecessor has another query is the HEAD of its query's run, one whose
//           successor has another is its TAIL; head and tail note their positions in the query's table entry {first, last};
//   counts  run lengths last - first + 1 (0 for a query without records), scanned over the read ids by the library's scan
//           (launch_scan) into query_offs[n_reads + 1];
//   move    record i of query q goes to out[query_offs[q] + (i - first[q])]: the lanes of a run write neighbouring records.
// Input that breaks the two rules is counted, never followed: a record whose query is no indexed read touches no table and
// is not moved; a query's second run loses the compare-and-swap for the table entry and is not moved; and whatever the
// tables hold, no record is written outside out[0 .. n_edges).  Positions are 64 bits throughout (n_edges may reach 2^32).
// The restatement the tests hold this against is siga_amd/sharding.py::restore_order (numpy, stable argsort).
// No counterpart in the reference (one process, reads in file order: src/overlap_builder.cpp:466-483).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/sigax.h"
#include "sigax_kernels.h"

int sigax_fail(int code, const char* fmt, ...);  // sigax_index.cpp

namespace {
typedef unsigned long long u64;
typedef uint32_t u32;

constexpr u64 RUN_EMPTY = ~0ull;  // a query's `first` before any head has claimed it (no position: n_edges <= 2^32)

// one table entry per read id; 16 bytes, so that move fetches both ends with one vector load
struct __attribute__((aligned(16))) RunEnds {
  u64 first, last;
};

// where the pieces of the caller's scratch lie
struct OrderWork {
  u64 tab, offs, partial, total, cnt, bytes;
};
OrderWork order_work(u64 n_reads) {
  OrderWork w;
  u64 at = 0;
  w.tab = at;
  at += n_reads * sizeof(RunEnds);
  w.offs = at;
  at += (n_reads + 1) * 8;
  w.partial = at;
  at += scan_partials_needed(n_reads) * 8;
  w.total = at;
  at += 8;
  w.cnt = at;
  at += (n_reads + 1) * 4;
  w.bytes = (at + 15) & ~15ull;
  return w;
}

// status[0] += records whose query is no read, status[1] += runs beyond a query's first.  Every lane of a wave stays in the
// kernel to its end: its neighbours read its query through cross-lane moves; only the wave's edge lanes go to memory for the
// record before or after the wave's 64.
__global__ __launch_bounds__(256) void k_order_runs(const uint4* __restrict__ in, u64 n_edges, u64 n_reads, RunEnds* __restrict__ tab,
                                                    u64* __restrict__ status) {
  const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
  const u32 lane = threadIdx.x & 63u;
  const bool live = i < n_edges;
  u32 q = 0;
  if (live) q = in[i].x;  // (this pass needs a record's query alone)
  u32 before = __shfl_up(q, 1, 64), after = __shfl_down(q, 1, 64);
  if (!live) return;
  bool head = i == 0, tail = i + 1 == n_edges;
  if (!head) {
    if (lane == 0) before = in[i - 1].x;
    head = before != q;
  }
  if (!tail) {
    if (lane == 63) after = in[i + 1].x;
    tail = after != q;
  }
  if (q >= n_reads) {
    atomicAdd(&status[0], 1ull);
    return;
  }
  bool mine = true;  // (a tail that is its run's head too leaves `last` alone when the run lost)
  if (head) {
    mine = atomicCAS(&tab[q].first, RUN_EMPTY, i) == RUN_EMPTY;
    if (!mine) atomicAdd(&status[1], 1ull);
  }
  if (tail && mine) tab[q].last = i;
}

__global__ __launch_bounds__(256) void k_order_counts(const RunEnds* __restrict__ tab, u64 n_reads, u32* __restrict__ cnt) {
  const u64 q = (u64)blockIdx.x * 256u + threadIdx.x;
  if (q >= n_reads) return;
  const ulonglong2 e = *reinterpret_cast<const ulonglong2*>(tab + q);
  cnt[q] = e.x == RUN_EMPTY ? 0u : (u32)(e.y - e.x + 1);
}

__global__ __launch_bounds__(256) void k_order_move(const uint4* __restrict__ in, u64 n_edges, u64 n_reads, const RunEnds* __restrict__ tab,
                                                    const u64* __restrict__ offs, uint4* __restrict__ out) {
  const u64 i = (u64)blockIdx.x * 256u + threadIdx.x;
  if (i >= n_edges) return;
  const uint4 rec = in[i];
  const u32 q = rec.x;
  if (q >= n_reads) return;
  const ulonglong2 e = *reinterpret_cast<const ulonglong2*>(tab + q);
  if (i < e.x || i > e.y) return;  // (an empty entry has first = 2^64 - 1: nothing passes)
  const u64 to = offs[q] + (i - e.x);
  if (to < n_edges) out[to] = rec;  // holds for every input that kept the rules; the rest is not written
}

__global__ __launch_bounds__(256) void k_flags_by_id(const uint8_t* __restrict__ flags, const u32* __restrict__ ids, u64 n, u64 n_reads,
                                                     uint8_t* __restrict__ out, u64* __restrict__ status) {
  const u64 r = (u64)blockIdx.x * 256u + threadIdx.x;
  if (r >= n) return;
  const u32 id = ids[r];
  if (id >= n_reads) {
    atomicAdd(status, 1ull);
    return;
  }
  out[id] = flags[r];
}

bool overlap(const void* a, u64 na, const void* b, u64 nb) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return na && nb && x < y + nb && y < x + na;
}
unsigned blocks_of(u64 n) { return (unsigned)((n + 255) / 256); }
}  // namespace

extern "C" int sigax_edges_order_workspace(uint64_t n_edges, uint64_t n_reads, uint64_t* bytes) {
  if (!bytes) return sigax_fail(SIGAX_E_ARG, "NULL argument");
  if (n_edges > (1ull << 32) || n_reads > (1ull << 32)) return sigax_fail(SIGAX_E_ARG, "more than 2^32 records or reads");
  *bytes = order_work(n_reads).bytes;
  return SIGAX_OK;
}

extern "C" int sigax_edges_restore_order(int device, const sigax_edge* d_in, uint64_t n_edges, uint64_t n_reads, sigax_edge* d_out,
                                         uint64_t* d_query_offs, void* d_work, uint64_t work_bytes, void* d_status, void* stream) {
  if (!d_status) return sigax_fail(SIGAX_E_ARG, "NULL d_status");
  if (n_edges > (1ull << 32) || n_reads > (1ull << 32)) return sigax_fail(SIGAX_E_ARG, "more than 2^32 records or reads");
  if (n_edges && (!d_in || !d_out)) return sigax_fail(SIGAX_E_ARG, "NULL record buffer");
  if (n_edges && (((uintptr_t)d_in | (uintptr_t)d_out) & 15)) return sigax_fail(SIGAX_E_ARG, "record buffers must be 16-byte aligned");
  if (overlap(d_in, n_edges * sizeof(sigax_edge), d_out, n_edges * sizeof(sigax_edge))) return sigax_fail(SIGAX_E_ARG, "d_out overlaps d_in");
  const OrderWork w = order_work(n_reads);
  if (n_edges) {
    if (!d_work) return sigax_fail(SIGAX_E_ARG, "NULL d_work");
    if ((uintptr_t)d_work & 15) return sigax_fail(SIGAX_E_ARG, "d_work must be 16-byte aligned");
    if (work_bytes < w.bytes) return sigax_fail(SIGAX_E_ARG, "workspace of %llu bytes, %llu needed (sigax_edges_order_workspace)", (u64)work_bytes, w.bytes);
  }
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) return sigax_fail(SIGAX_E_DEVICE, "hipSetDevice(%d): %s", device, hipGetErrorString(e));
  hipStream_t st = (hipStream_t)stream;
  e = hipMemsetAsync(d_status, 0, 16, st);
  if (e == hipSuccess && n_edges == 0 && d_query_offs) e = hipMemsetAsync(d_query_offs, 0, (n_reads + 1) * 8, st);
  if (e != hipSuccess) return sigax_fail(SIGAX_E_DEVICE, "hipMemsetAsync: %s", hipGetErrorString(e));
  if (n_edges == 0) return SIGAX_OK;
  char* base = (char*)d_work;
  RunEnds* tab = (RunEnds*)(base + w.tab);
  u64* offs = d_query_offs ? (u64*)d_query_offs : (u64*)(base + w.offs);
  u32* cnt = (u32*)(base + w.cnt);
  if (n_reads) {
    e = hipMemsetAsync(tab, 0xFF, n_reads * sizeof(RunEnds), st);
    if (e != hipSuccess) return sigax_fail(SIGAX_E_DEVICE, "hipMemsetAsync: %s", hipGetErrorString(e));
  }
  hipLaunchKernelGGL(k_order_runs, dim3(blocks_of(n_edges)), dim3(256), 0, st, (const uint4*)d_in, (u64)n_edges, (u64)n_reads, tab, (u64*)d_status);
  if (n_reads) hipLaunchKernelGGL(k_order_counts, dim3(blocks_of(n_reads)), dim3(256), 0, st, (const RunEnds*)tab, (u64)n_reads, cnt);
  launch_scan(cnt, n_reads, (u64*)(base + w.partial), offs, (u64*)(base + w.total), st);
  hipLaunchKernelGGL(k_order_move, dim3(blocks_of(n_edges)), dim3(256), 0, st, (const uint4*)d_in, (u64)n_edges, (u64)n_reads, (const RunEnds*)tab,
                     (const u64*)offs, (uint4*)d_out);
  e = hipGetLastError();
  if (e != hipSuccess) return sigax_fail(SIGAX_E_DEVICE, "sigax_edges_restore_order: %s", hipGetErrorString(e));
  return SIGAX_OK;
}

extern "C" int sigax_flags_by_read_id(int device, const uint8_t* d_flags, const uint32_t* d_ids, uint64_t n, uint64_t n_reads, uint8_t* d_out,
                                      void* d_status, void* stream) {
  if (!d_status) return sigax_fail(SIGAX_E_ARG, "NULL d_status");
  if (n && (!d_flags || !d_ids || !d_out)) return sigax_fail(SIGAX_E_ARG, "NULL argument");
  if (n_reads > (1ull << 32)) return sigax_fail(SIGAX_E_ARG, "more than 2^32 reads");
  if (overlap(d_flags, n, d_out, n_reads)) return sigax_fail(SIGAX_E_ARG, "d_out overlaps d_flags");
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) return sigax_fail(SIGAX_E_DEVICE, "hipSetDevice(%d): %s", device, hipGetErrorString(e));
  hipStream_t st = (hipStream_t)stream;
  e = hipMemsetAsync(d_status, 0, 8, st);
  if (e != hipSuccess) return sigax_fail(SIGAX_E_DEVICE, "hipMemsetAsync: %s", hipGetErrorString(e));
  if (n == 0) return SIGAX_OK;
  hipLaunchKernelGGL(k_flags_by_id, dim3(blocks_of(n)), dim3(256), 0, st, d_flags, d_ids, (u64)n, (u64)n_reads, d_out, (u64*)d_status);
  e = hipGetLastError();
  if (e != hipSuccess) return sigax_fail(SIGAX_E_DEVICE, "k_flags_by_id: %s", hipGetErrorString(e));
  return SIGAX_OK;
}

namespace {
struct Freer {
  std::vector<void*> ptrs;
  ~Freer() {
    for (void* p : ptrs) hipFree(p);
  }
  hipError_t alloc(void** out, size_t bytes) {
    *out = nullptr;
    hipError_t e = hipMalloc(out, bytes ? bytes : 16);
    if (e == hipSuccess) ptrs.push_back(*out);
    return e;
  }
};
}  // namespace

#define ORDER_TRY(expr)                                                                                                  \
  do {                                                                                                                   \
    hipError_t e_ = (expr);                                                                                              \
    if (e_ != hipSuccess) return sigax_fail(SIGAX_E_DEVICE, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

extern "C" int sigax_edges_restore_order_host(int device, const sigax_edge* in, uint64_t n_edges, uint64_t n_reads, sigax_edge* out,
                                              uint64_t* query_offs) {
  if (n_edges && (!in || !out)) return sigax_fail(SIGAX_E_ARG, "NULL record buffer");
  if (overlap(in, n_edges * sizeof(sigax_edge), out, n_edges * sizeof(sigax_edge))) return sigax_fail(SIGAX_E_ARG, "out overlaps in");
  uint64_t wb = 0;
  int rc = sigax_edges_order_workspace(n_edges, n_reads, &wb);
  if (rc != SIGAX_OK) return rc;
  if (n_edges == 0) {
    if (query_offs) memset(query_offs, 0, (n_reads + 1) * 8);
    return SIGAX_OK;
  }
  ORDER_TRY(hipSetDevice(device));
  Freer g;
  void *d_in, *d_out, *d_offs = nullptr, *d_work, *d_status;
  const size_t bytes = (size_t)n_edges * sizeof(sigax_edge);
  ORDER_TRY(g.alloc(&d_in, bytes));
  ORDER_TRY(g.alloc(&d_out, bytes));
  if (query_offs) ORDER_TRY(g.alloc(&d_offs, (n_reads + 1) * 8));
  ORDER_TRY(g.alloc(&d_work, wb));
  ORDER_TRY(g.alloc(&d_status, 16));
  ORDER_TRY(hipMemcpy(d_in, in, bytes, hipMemcpyHostToDevice));
  rc = sigax_edges_restore_order(device, (const sigax_edge*)d_in, n_edges, n_reads, (sigax_edge*)d_out, (uint64_t*)d_offs, d_work, wb, d_status, nullptr);
  if (rc != SIGAX_OK) return rc;
  u64 status[2] = {0, 0};
  ORDER_TRY(hipMemcpy(status, d_status, 16, hipMemcpyDeviceToHost));  // (waits for the null stream's kernels)
  if (status[0]) return sigax_fail(SIGAX_E_ARG, "%llu records with a query beyond the %llu reads", status[0], (u64)n_reads);
  if (status[1]) return sigax_fail(SIGAX_E_ARG, "%llu runs beyond the first of their query: some query's records are not contiguous", status[1]);
  ORDER_TRY(hipMemcpy(out, d_out, bytes, hipMemcpyDeviceToHost));
  if (query_offs) ORDER_TRY(hipMemcpy(query_offs, d_offs, (n_reads + 1) * 8, hipMemcpyDeviceToHost));
  return SIGAX_OK;
}
