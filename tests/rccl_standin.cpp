// tests/rccl_standin.cpp -- a stand-in for RCCL whose ranks are host threads of ONE process on ONE GPU, so that the exchange
// step of siga_amd/csrc/sigax_comm.cpp (count all-gather, grouped Send / Recv, the root's displacements) runs with a world
// above one on a one-GPU box.  Loaded through SIGAX_RCCL_LIB; built at test time (tests/test_gpu_comm_ranks.py).
//
// It exports the nine entry points sigax_comm.cpp binds, with the types of <rccl/rccl.h>, and keeps of their semantics what
// that file relies on:
//   * communicators made from the same ncclUniqueId form one world; ncclCommInitRank returns once all ranks have joined;
//   * ncclAllGather: every rank's recvbuff holds all ranks' sendbuff in rank order;
//   * ncclSend / ncclRecv move `count` elements from the sender's buffer to the receiver's; between ncclGroupStart and
//     ncclGroupEnd they are only noted and posted together at ncclGroupEnd, so the Recvs of one group complete whatever
//     order the senders arrive in;
//   * stream order: a call waits for its stream before it publishes or overwrites a buffer (everything enqueued earlier has
//     run), and the copy is done on the receiving rank's stream and waited for before the call returns (everything enqueued
//     later sees it).  That is stronger than RCCL's (which stays asynchronous) and never weaker.
// What RCCL does not give and this does: a Send and its Recv that disagree in count or type are an error on BOTH sides
// (a wrong counts[] on one rank becomes visible), and no wait is endless -- every rendezvous has a deadline
// (RCCL_STANDIN_DEADLINE_MS, default 20 000), after which the world is marked broken and every later call on it fails at once.
//
// With -DRCCL_STANDIN_ONE_SYMBOL only ncclGetUniqueId is exported: the library that "lacks entry points".
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

namespace {
std::atomic<unsigned long long> g_next_id{1};
}

extern "C" ncclResult_t ncclGetUniqueId(ncclUniqueId* id) {
  if (!id) return ncclInvalidArgument;
  memset(id, 0, sizeof(*id));
  const unsigned long long k = g_next_id.fetch_add(1);
  snprintf(id->internal, sizeof(id->internal), "rccl-standin-%llu-%p", k, (void*)&g_next_id);
  return ncclSuccess;
}

#ifndef RCCL_STANDIN_ONE_SYMBOL
namespace {
using Clock = std::chrono::steady_clock;

Clock::duration deadline_span() {
  const char* e = getenv("RCCL_STANDIN_DEADLINE_MS");
  long ms = e ? atol(e) : 0;
  return std::chrono::milliseconds(ms > 0 ? ms : 20000);
}

thread_local std::string t_detail;  // what the last failing call of this thread has to say
ncclResult_t fail(ncclResult_t code, const std::string& what) {
  t_detail = "stand-in: " + what;
  return code;
}

size_t type_size(ncclDataType_t t) {
  switch (t) {
    case ncclInt8:
    case ncclUint8:
      return 1;
    case ncclFloat16:
    case ncclBfloat16:
      return 2;
    case ncclInt32:
    case ncclUint32:
    case ncclFloat32:
      return 4;
    case ncclInt64:
    case ncclUint64:
    case ncclFloat64:
      return 8;
    default:
      return 0;
  }
}

// one Send, from the moment it is posted until the receiver has copied it (or either side gave up)
struct Msg {
  const void* buf;
  size_t count;
  ncclDataType_t type;
  enum { POSTED, CLAIMED, DONE, CANCELLED } state = POSTED;
  ncclResult_t result = ncclSuccess;
  std::string detail;
};

struct World {
  int size = 0;
  std::mutex mu;
  std::condition_variable cv;
  bool broken = false;  // a deadline ran out: nothing on this world can be trusted to pair up any more
  std::vector<char> joined;
  int n_joined = 0, n_alive = 0;
  // all-gather: two barriers per call (buffers published / copies done)
  std::vector<const void*> ag_send;
  int bar_count = 0;
  unsigned long long bar_gen = 0;
  std::vector<std::deque<std::shared_ptr<Msg>>> chan;  // [src * size + dst], in posting order
  std::string key;
};

std::mutex g_worlds_mu;
std::map<std::string, std::shared_ptr<World>> g_worlds;

// (w.mu held) all ranks arrive, or the deadline passes and the world breaks
bool barrier(World& w, std::unique_lock<std::mutex>& lock) {
  if (w.broken) return false;
  const unsigned long long gen = w.bar_gen;
  if (++w.bar_count == w.size) {
    w.bar_count = 0;
    ++w.bar_gen;
    w.cv.notify_all();
    return true;
  }
  const auto until = Clock::now() + deadline_span();
  while (w.bar_gen == gen && !w.broken)
    if (w.cv.wait_until(lock, until) == std::cv_status::timeout && w.bar_gen == gen) {
      w.broken = true;
      w.cv.notify_all();
    }
  return w.bar_gen != gen;
}

struct Op {
  bool send;
  void* buf;
  size_t count;
  ncclDataType_t type;
  int peer;
  ncclComm* comm;
  hipStream_t stream;
};
thread_local int t_group_depth = 0;
thread_local std::vector<Op> t_ops;
}  // namespace

struct ncclComm {
  std::shared_ptr<World> world;
  int rank;
};

namespace {
ncclResult_t run_ops(std::vector<Op>& ops) {
  ncclResult_t first = ncclSuccess;
  std::string first_detail;
  auto note = [&](ncclResult_t r, const std::string& d) {
    if (r != ncclSuccess && first == ncclSuccess) {
      first = r;
      first_detail = d;
    }
  };
  // everything enqueued earlier on the ops' streams has run before a buffer is published or overwritten
  for (const Op& op : ops) {
    hipError_t e = hipStreamSynchronize(op.stream);
    if (e != hipSuccess) return fail(ncclUnhandledCudaError, std::string("hipStreamSynchronize: ") + hipGetErrorString(e));
  }
  // post every Send of the group, then serve every Recv, then wait for the Sends
  std::vector<std::shared_ptr<Msg>> sent(ops.size());
  for (size_t i = 0; i < ops.size(); ++i) {
    const Op& op = ops[i];
    if (!op.send) continue;
    World& w = *op.comm->world;
    std::lock_guard<std::mutex> lock(w.mu);
    if (w.broken) {
      note(ncclInternalError, "the world is broken (an earlier rendezvous ran out of time)");
      continue;
    }
    auto m = std::make_shared<Msg>();
    m->buf = op.buf;
    m->count = op.count;
    m->type = op.type;
    w.chan[(size_t)op.comm->rank * w.size + op.peer].push_back(m);
    sent[i] = m;
    w.cv.notify_all();
  }
  for (const Op& op : ops) {
    if (op.send) continue;
    World& w = *op.comm->world;
    std::shared_ptr<Msg> m;
    {
      std::unique_lock<std::mutex> lock(w.mu);
      auto& q = w.chan[(size_t)op.peer * w.size + op.comm->rank];
      const auto until = Clock::now() + deadline_span();
      for (;;) {
        while (!q.empty() && q.front()->state == Msg::CANCELLED) q.pop_front();
        if (!q.empty() || w.broken) break;
        if (w.cv.wait_until(lock, until) == std::cv_status::timeout && q.empty()) {
          w.broken = true;
          w.cv.notify_all();
        }
      }
      if (q.empty()) {
        char t[160];
        snprintf(t, sizeof(t), "rank %d: no Send from rank %d met this Recv of %zu elements before the deadline", op.comm->rank, op.peer, op.count);
        note(ncclInternalError, t);
        continue;
      }
      m = q.front();
      q.pop_front();
      m->state = Msg::CLAIMED;
    }
    ncclResult_t r = ncclSuccess;
    std::string d;
    if (m->count != op.count || m->type != op.type) {
      char t[200];
      snprintf(t, sizeof(t), "mismatch: rank %d sends %zu elements of type %d, rank %d receives %zu of type %d", op.peer, m->count, (int)m->type,
               op.comm->rank, op.count, (int)op.type);
      r = ncclInvalidArgument;
      d = t;
    } else if (op.count) {
      hipError_t e = hipMemcpyAsync(op.buf, m->buf, op.count * type_size(op.type), hipMemcpyDeviceToDevice, op.stream);
      if (e == hipSuccess) e = hipStreamSynchronize(op.stream);
      if (e != hipSuccess) {
        r = ncclUnhandledCudaError;
        d = std::string("device copy of a Recv: ") + hipGetErrorString(e);
      }
    }
    {
      std::lock_guard<std::mutex> lock(w.mu);
      m->result = r;
      m->detail = d;
      m->state = Msg::DONE;
      w.cv.notify_all();
    }
    note(r, d);
  }
  for (size_t i = 0; i < ops.size(); ++i) {
    if (!sent[i]) continue;
    const Op& op = ops[i];
    World& w = *op.comm->world;
    Msg& m = *sent[i];
    std::unique_lock<std::mutex> lock(w.mu);
    const auto until = Clock::now() + deadline_span();
    while (m.state != Msg::DONE) {
      if (m.state == Msg::POSTED && w.broken) m.state = Msg::CANCELLED;
      if (m.state == Msg::CANCELLED) break;
      // (a claimed message is being copied: that ends by itself)
      if (w.cv.wait_until(lock, until) == std::cv_status::timeout && m.state == Msg::POSTED) {
        m.state = Msg::CANCELLED;
        w.broken = true;
        w.cv.notify_all();
      }
    }
    if (m.state == Msg::CANCELLED) {
      char t[160];
      snprintf(t, sizeof(t), "rank %d: no Recv on rank %d met this Send of %zu elements before the deadline", op.comm->rank, op.peer, op.count);
      note(ncclInternalError, t);
    } else {
      note(m.result, m.detail);
    }
  }
  if (first != ncclSuccess) return fail(first, first_detail);
  return ncclSuccess;
}

ncclResult_t enqueue(bool send, const void* buf, size_t count, ncclDataType_t type, int peer, ncclComm_t comm, hipStream_t stream) {
  if (!comm) return fail(ncclInvalidArgument, "NULL communicator");
  if (peer < 0 || peer >= comm->world->size || peer == comm->rank) return fail(ncclInvalidArgument, "peer outside the world, or the rank itself");
  if (!type_size(type)) return fail(ncclInvalidArgument, "unknown data type");
  if (count && !buf) return fail(ncclInvalidArgument, "NULL buffer");
  t_ops.push_back(Op{send, const_cast<void*>(buf), count, type, peer, comm, stream});
  if (t_group_depth) return ncclSuccess;
  std::vector<Op> ops;
  ops.swap(t_ops);
  return run_ops(ops);
}
}  // namespace

extern "C" ncclResult_t ncclCommInitRank(ncclComm_t* comm, int nranks, ncclUniqueId id, int rank) {
  if (!comm || nranks < 1 || rank < 0 || rank >= nranks) return fail(ncclInvalidArgument, "ncclCommInitRank: bad argument");
  *comm = nullptr;
  const std::string key(id.internal, sizeof(id.internal));
  std::shared_ptr<World> w;
  {
    std::lock_guard<std::mutex> lock(g_worlds_mu);
    auto& slot = g_worlds[key];
    if (!slot) {
      slot = std::make_shared<World>();
      slot->size = nranks;
      slot->key = key;
      slot->joined.assign(nranks, 0);
      slot->ag_send.assign(nranks, nullptr);
      slot->chan.resize((size_t)nranks * nranks);
    }
    w = slot;
  }
  std::unique_lock<std::mutex> lock(w->mu);
  if (w->size != nranks) return fail(ncclInvalidArgument, "ncclCommInitRank: the ranks of one id disagree about the world's size");
  if (w->joined[rank]) return fail(ncclInvalidArgument, "ncclCommInitRank: this rank has joined already");
  if (w->broken) return fail(ncclInternalError, "ncclCommInitRank: the world is broken");
  w->joined[rank] = 1;
  ++w->n_joined;
  ++w->n_alive;
  w->cv.notify_all();
  const auto until = Clock::now() + deadline_span();
  while (w->n_joined < w->size && !w->broken)
    if (w->cv.wait_until(lock, until) == std::cv_status::timeout && w->n_joined < w->size) {
      w->broken = true;
      w->cv.notify_all();
    }
  if (w->n_joined < w->size) {
    --w->n_alive;
    return fail(ncclInternalError, "ncclCommInitRank: not every rank of the world joined before the deadline");
  }
  *comm = new ncclComm{w, rank};
  return ncclSuccess;
}

extern "C" ncclResult_t ncclCommDestroy(ncclComm_t comm) {
  if (!comm) return ncclSuccess;
  std::shared_ptr<World> w = comm->world;
  delete comm;
  bool last;
  {
    std::lock_guard<std::mutex> lock(w->mu);
    last = --w->n_alive == 0;
  }
  if (last) {
    std::lock_guard<std::mutex> lock(g_worlds_mu);
    g_worlds.erase(w->key);
  }
  return ncclSuccess;
}

extern "C" ncclResult_t ncclAllGather(const void* sendbuff, void* recvbuff, size_t sendcount, ncclDataType_t datatype, ncclComm_t comm,
                                      hipStream_t stream) {
  if (!comm || !sendbuff || !recvbuff) return fail(ncclInvalidArgument, "ncclAllGather: NULL argument");
  const size_t bytes = sendcount * type_size(datatype);
  if (!type_size(datatype)) return fail(ncclInvalidArgument, "ncclAllGather: unknown data type");
  World& w = *comm->world;
  hipError_t e = hipStreamSynchronize(stream);  // what was enqueued before has filled sendbuff
  if (e != hipSuccess) return fail(ncclUnhandledCudaError, std::string("hipStreamSynchronize: ") + hipGetErrorString(e));
  std::vector<const void*> from;
  {
    std::unique_lock<std::mutex> lock(w.mu);
    w.ag_send[comm->rank] = sendbuff;
    if (!barrier(w, lock)) return fail(ncclInternalError, "ncclAllGather: not every rank arrived before the deadline");
    from = w.ag_send;
  }
  for (int r = 0; r < w.size && e == hipSuccess; ++r)
    if (bytes) e = hipMemcpyAsync((char*)recvbuff + (size_t)r * bytes, from[r], bytes, hipMemcpyDeviceToDevice, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  {
    // (nobody's sendbuff may change before every rank has read it; the barrier is passed even after a failed copy, so that
    // the other ranks do not wait for this one)
    std::unique_lock<std::mutex> lock(w.mu);
    if (!barrier(w, lock)) return fail(ncclInternalError, "ncclAllGather: not every rank finished before the deadline");
  }
  if (e != hipSuccess) return fail(ncclUnhandledCudaError, std::string("device copy of ncclAllGather: ") + hipGetErrorString(e));
  return ncclSuccess;
}

extern "C" ncclResult_t ncclSend(const void* sendbuff, size_t count, ncclDataType_t datatype, int peer, ncclComm_t comm, hipStream_t stream) {
  return enqueue(true, sendbuff, count, datatype, peer, comm, stream);
}

extern "C" ncclResult_t ncclRecv(void* recvbuff, size_t count, ncclDataType_t datatype, int peer, ncclComm_t comm, hipStream_t stream) {
  return enqueue(false, recvbuff, count, datatype, peer, comm, stream);
}

extern "C" ncclResult_t ncclGroupStart() {
  ++t_group_depth;
  return ncclSuccess;
}

extern "C" ncclResult_t ncclGroupEnd() {
  if (t_group_depth == 0) return fail(ncclInvalidUsage, "ncclGroupEnd without ncclGroupStart");
  if (--t_group_depth) return ncclSuccess;
  std::vector<Op> ops;
  ops.swap(t_ops);
  return ops.empty() ? ncclSuccess : run_ops(ops);
}

extern "C" const char* ncclGetErrorString(ncclResult_t result) {
  if (result == ncclSuccess) return "no error";
  if (!t_detail.empty()) return t_detail.c_str();
  return "stand-in: error";
}
#endif  // RCCL_STANDIN_ONE_SYMBOL
