// siga_amd/host/overlap_builder.cpp -- FMIndex (the handle of the index on the GPU) and OverlapBuilder: `siga overlap`, `siga rmdup`.
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <mutex>
#include <thread>

#include "asqg_text.hpp"
#include "host_util.hpp"
#include "out_file.hpp"
#include "reads.hpp"
#include "siga_host.hpp"

namespace sigah {

// ------------------------------------------------------------------------------------------------------
// FMIndex handle
// ------------------------------------------------------------------------------------------------------
FMIndex::~FMIndex() {
  if (_h) sigax_index_close(_h);
}

bool FMIndex::load(const std::string& prefix, FMIndex& fmi, int device) {
  if (fmi._h) {
    sigax_index_close(fmi._h);
    fmi._h = nullptr;
  }
  int rc = sigax_index_open((prefix + ".bwt").c_str(), (prefix + ".rbwt").c_str(), (prefix + ".sai").c_str(),
                            (prefix + ".rsai").c_str(), device, &fmi._h);
  return rc == SIGAX_OK;
}
// the forward index alone: FMIndex::load(prefix + ".bwt") of src/correct.cpp:41-47 (`siga index --no-reverse` writes no more)
bool FMIndex::loadForward(const std::string& prefix, FMIndex& fmi, int device) {
  if (fmi._h) {
    sigax_index_close(fmi._h);
    fmi._h = nullptr;
  }
  return sigax_index_open((prefix + ".bwt").c_str(), nullptr, nullptr, nullptr, device, &fmi._h) == SIGAX_OK;
}
// ... with <prefix>.sai beside it: the table that names the reads of `siga locate`'s hits
bool FMIndex::loadForwardSai(const std::string& prefix, FMIndex& fmi, int device) {
  if (fmi._h) {
    sigax_index_close(fmi._h);
    fmi._h = nullptr;
  }
  return sigax_index_open((prefix + ".bwt").c_str(), nullptr, (prefix + ".sai").c_str(), nullptr, device, &fmi._h) == SIGAX_OK;
}

uint64_t FMIndex::length() const {
  sigax_index_info inf;
  if (!_h || sigax_index_info_get(_h, &inf) != SIGAX_OK) return 0;
  return inf.n_symbols;
}

// ------------------------------------------------------------------------------------------------------
// OverlapBuilder::build (src/overlap_builder.cpp:423-509).  The reference reads items in batches of threads x batch-size,
// runs overlap() on them under OpenMP and post-processes the batch serially in input order (parallel::foreach,
// src/parallel_framework.h:16-59).  Here: the reads are parsed once (in parallel), cut into device batches sized from
// free HBM, and every GPU of the run keeps two batch objects in flight (upload / kernels / download overlap); the main
// thread takes finished batches in input order, formats their VT lines on the host threads and feeds the block-parallel
// gzip writer; the ED lines follow in hits order from the collected 16-byte edge records.  With --gpus N the index is
// replicated device to device and batches go to whichever GPU is free: the output does not depend on N.
// ------------------------------------------------------------------------------------------------------
struct OverlapBuilder::Preloaded {
  std::string path;
  ReadStore reads;
  std::vector<uint32_t> lengths, ranks;
  bool ok = false;
  std::unique_ptr<VtAhead> ahead;  // (after `reads`: gone before them)
};

void OverlapBuilder::preload(const std::string& input, size_t threads, long minOverlap, const std::string& output) const {
  const HostSettings hs;
  const unsigned nt = host_threads(threads, hs);
  auto p = std::make_shared<Preloaded>();
  p->path = input;
  PhaseTimer pt(hs.timing);
  p->ok = LoadReads(input, &p->reads, nt, hs);
  pt.lap("  reads parsed");
  if (p->ok) name_ranks(p->reads, nt, &p->lengths, &p->ranks);
  pt.lap("  names ranked");
  // (an option) the VT lines start now, while the index is still on its way to the GPU
  if (p->ok && minOverlap >= 0 && !output.empty() && hs.vt_ahead_wanted())
    p->ahead.reset(new VtAhead(&p->reads, nt, asqg_header((size_t)minOverlap), OutFile::gz_name(output), hs));
  _pre = p;
}

namespace {

std::vector<int> device_list(int first, int count, const HostSettings& hs) {
  const std::vector<int>& map = hs.device_map;
  std::vector<int> d;
  for (int k = 0; k < std::max(count, 1); ++k) d.push_back((size_t)k < map.size() ? map[k] : first + k);
  return d;
}

// the GPUs of a run: the loaded index on the first, device-to-device replicas (closed with this object) on the others
struct Replicas {
  std::vector<int> devs;
  std::vector<sigax_index*> idx;
  Replicas(sigax_index* loaded, std::vector<int> devices) : devs(std::move(devices)), idx(devs.size(), nullptr) { idx[0] = loaded; }
  Replicas(const Replicas&) = delete;
  Replicas& operator=(const Replicas&) = delete;
  ~Replicas() {
    for (size_t k = 1; k < idx.size(); ++k)
      if (idx[k]) sigax_index_close(idx[k]);
  }
  bool clone(std::string* error) {
    for (size_t k = 1; k < devs.size(); ++k) {
      if (sigax_index_clone(idx[0], devs[k], &idx[k]) != SIGAX_OK) {
        *error = std::string("failed to replicate the index on GPU ") + std::to_string(devs[k]) + ": " + sigax_last_error();
        return false;
      }
    }
    return true;
  }
};

// what every device worker of a run shares
struct Run {
  const ReadStore& reads;
  size_t n, per, nbatch;  // reads, reads per device batch, batches
  uint32_t minOverlap, flags, maxLen;
  bool one_chain;  // a batch object runs as one launch chain (see DeviceWorker::run)
  bool timing;
};

// device batches: as many reads as the free memory of a GPU takes with two batches in flight, at most 2^20, and no
// more than an even share of the input; the reference's threads x batch-size is a lower bound
// (asked of every replica: two batch objects per replica, and replicas that share a physical device -- SIGA_DEVICE_MAP
// rehearsals -- share its memory; the smallest answer sizes the batches of all)
bool reads_per_batch(const Replicas& gpus, const Run& r, size_t threads, size_t batch, const HostSettings& hs, size_t* per_out) {
  uint32_t hint = 1u << 20;
  for (size_t k = 0; r.n > 0 && k < gpus.devs.size(); ++k) {
    uint32_t sharing = 0, h = 0;
    for (int d : gpus.devs) sharing += d == gpus.devs[k] ? 1u : 0u;
    if (sigax_batch_size_hint(gpus.idx[k], std::max(r.maxLen, 1u), r.minOverlap, r.flags, 2 * sharing, &h) != SIGAX_OK) return false;
    hint = k == 0 ? h : std::min(hint, h);
  }
  size_t per = std::min<size_t>(hint, 1u << 20);
  if (hs.batch_reads) per = std::min<size_t>(hint, hs.batch_reads);
  per = std::min(per, std::max<size_t>((r.n + gpus.devs.size() - 1) / gpus.devs.size(), 1));
  if (!hs.batch_reads) per = std::max(per, std::min<size_t>(std::max<size_t>(threads, 1) * std::max<size_t>(batch, 1), hint));
  *per_out = std::max<size_t>(per, 1);
  return true;
}

struct BatchOut {
  std::vector<uint8_t> substring;
  sigax_edge* edges = nullptr;
  uint64_t n_edges = 0;
  bool ready = false;
};
struct Pipeline {
  std::mutex mu;
  std::condition_variable cv;
  std::vector<BatchOut> out;
  std::atomic<size_t> next{0};
  std::atomic<bool> failed{false};
  std::string error;
  ~Pipeline() {  // (batches nobody took: a run that failed)
    for (auto& o : out)
      if (o.edges) sigax_free(o.edges);
  }
  void fail(const std::string& e) {
    std::lock_guard<std::mutex> g(mu);
    if (!failed.exchange(true)) error = e;
    cv.notify_all();
  }
  // batch b, once it is back; false: the run has failed
  bool take(size_t b, BatchOut* r) {
    std::unique_lock<std::mutex> g(mu);
    cv.wait(g, [&] { return out[b].ready || failed; });
    if (!out[b].ready) return false;
    *r = std::move(out[b]);
    out[b].edges = nullptr;  // the taker's from here on
    return true;
  }
};

// One GPU of the run: two batch objects in flight (upload / kernels / download overlap), batches taken from the pipeline's
// counter, results left in its slots.
struct DeviceWorker {
  const Run& r;
  Pipeline& pl;
  sigax_index* ix;
  int dev;
  sigax_batch* bt[2] = {nullptr, nullptr};
  void* st[2] = {nullptr, nullptr};
  size_t cur[2] = {0, 0};
  bool busy[2] = {false, false};
  std::vector<uint64_t> loffs[2];

  DeviceWorker(const Run& run, Pipeline& pipeline, sigax_index* index, int device) : r(run), pl(pipeline), ix(index), dev(device) {}
  DeviceWorker(const DeviceWorker&) = delete;
  DeviceWorker& operator=(const DeviceWorker&) = delete;
  ~DeviceWorker() {
    for (int k = 0; k < 2; ++k) {
      if (bt[k]) sigax_batch_destroy(bt[k]);
      if (st[k]) sigax_stream_destroy(dev, st[k]);
    }
  }
  bool fail() {
    pl.fail(std::string("overlap failed: ") + sigax_last_error());
    return false;
  }
  bool submit(int k) {
    const size_t b = pl.next.fetch_add(1);
    if (b >= r.nbatch || pl.failed) return false;
    PhaseTimer clock(false);
    const size_t lo = b * r.per, cnt = std::min(r.per, r.n - lo);
    loffs[k].resize(cnt + 1);
    const uint64_t base = r.reads.offs[lo];
    for (size_t i = 0; i <= cnt; ++i) loffs[k][i] = r.reads.offs[lo + i] - base;
    int rc = sigax_batch_upload(bt[k], r.reads.seqs.data() + base, loffs[k].data(), (uint32_t)cnt, st[k]);
    if (rc == SIGAX_OK) rc = sigax_batch_run(bt[k], (uint32_t)lo, r.minOverlap, r.flags, st[k]);
    if (rc != SIGAX_OK) return fail();
    cur[k] = b;
    busy[k] = true;
    if (r.timing) fprintf(stderr, "[siga]   gpu %d batch %zu: upload + enqueue %.3f s\n", dev, b, clock.split());
    return true;
  }
  bool collect(int k) {
    BatchOut o;
    const size_t lo = cur[k] * r.per, cnt = std::min(r.per, r.n - lo);
    o.substring.resize(cnt);
    PhaseTimer clock(false);
    int rc = sigax_batch_finish(bt[k], st[k], nullptr);
    const double wait_s = clock.split();
    if (rc == SIGAX_OK) rc = sigax_batch_download_edges(bt[k], o.substring.data(), &o.edges, &o.n_edges);
    if (r.timing) fprintf(stderr, "[siga]   gpu %d batch %zu: wait %.3f s, download %.3f s\n", dev, cur[k], wait_s, clock.split());
    busy[k] = false;
    if (rc != SIGAX_OK) return fail();
    o.ready = true;
    {
      std::lock_guard<std::mutex> g(pl.mu);
      pl.out[cur[k]] = std::move(o);
    }
    pl.cv.notify_all();
    return true;
  }
  void run() {
    for (int k = 0; k < 2; ++k) {
      if (sigax_stream_create(dev, &st[k]) != SIGAX_OK || sigax_batch_create(ix, (uint32_t)r.per, 0, r.maxLen, &bt[k]) != SIGAX_OK) {
        fail();
        return;
      }
      // with two runs in flight per device the finder of one overlaps the filter/extract of the other: one launch chain
      // per run is then faster than the library's sub-batches (bench.py: 112 vs 106 M reads/s at BASELINE configs[1])
      if (r.one_chain) sigax_batch_set_subbatches(bt[k], 1);
    }
    submit(0);
    submit(1);
    int k = 0;  // the older of the two runs
    while (busy[k] && !pl.failed) {
      if (!collect(k)) break;
      submit(k);
      k ^= 1;
    }
  }
};

// the reference's progress line (OverlapPostProcess, src/overlap_builder.cpp:319-321: every threads x batch reads)
void progress_lines(size_t lo, size_t cnt, size_t n, size_t stepn) {
  for (size_t at = (lo / stepn + 1) * stepn; at <= lo + cnt; at += stepn)
    if (at % (stepn * 64) == 0 || at + stepn > n) fprintf(stderr, "processed %zu sequences\n", at);  // (every 64th: a device batch is a million reads)
}

}  // namespace

bool OverlapBuilder::build(const std::string& input, size_t minOverlap, const std::string& output, size_t threads,
                           size_t batch, size_t* processed) const {
  (void)processed;  // accepted and never written, like the reference (src/overlap_builder.cpp:423-424)
  const HostSettings hs;
  PhaseTimer pt(hs.timing);
  _error.clear();
  auto fail = [&](const std::string& e) { return _error = e, false; };
  if (!_fmi || !_fmi->handle()) return fail("FMIndex not loaded");
  // inputs: the reads (parsed by preload(), or here), the output file with its header, the read table on the device
  const unsigned nt = host_threads(threads, hs);
  std::shared_ptr<Preloaded> pre = _pre;
  _pre.reset();
  if (!pre || pre->path != input) {
    pre = std::make_shared<Preloaded>();
    pre->path = input;
    pre->ok = LoadReads(input, &pre->reads, nt, hs);
    if (pre->ok) name_ranks(pre->reads, nt, &pre->lengths, &pre->ranks);
  }
  if (!pre->ok) return fail("Failed to read file " + input);
  pt.lap("parse reads + name ranks");
  OutFile out(output, nt);
  if (!out.ok()) return fail("Failed to create ASQG " + output);
  const std::string header = asqg_header(minOverlap);
  out.write(header);
  const size_t n = pre->reads.size();
  // the VT lines ahead of the batches (started by preload() when it knew the header; from here otherwise)
  std::unique_ptr<VtAhead> ahead = std::move(pre->ahead);
  if (ahead && (ahead->header() != header || ahead->gz() != out.gz())) ahead.reset();
  if (!ahead && hs.vt_ahead_wanted() && n > 0) ahead.reset(new VtAhead(&pre->reads, nt, header, out.gz(), hs));
  if (!hs.vt_ahead_wanted()) ahead.reset();
  if (n > 0 && sigax_index_set_reads(_fmi->handle(), pre->lengths.data(), pre->ranks.data(), n) != SIGAX_OK)
    return fail(std::string("failed to load suffix array index: ") + sigax_last_error());
  pt.lap("read info to the device");
  // devices
  sigax_index_info inf;
  sigax_index_info_get(_fmi->handle(), &inf);
  Replicas gpus(_fmi->handle(), device_list(inf.device, _gpus, hs));
  if (!gpus.clone(&_error)) return false;
  if (gpus.devs.size() > 1) pt.lap("index replicas");
  // batch size
  const uint32_t flags = SIGAX_EDGES | (_irreducible ? SIGAX_IRREDUCIBLE : 0u) | (_rc ? SIGAX_RC : 0u);
  Run run{pre->reads, n, 0, 0, (uint32_t)minOverlap, flags, 0, false, hs.timing};
  for (uint32_t l : pre->lengths) run.maxLen = std::max(run.maxLen, l);
  if (!reads_per_batch(gpus, run, threads, batch, hs, &run.per)) return fail(std::string("overlap failed: ") + sigax_last_error());
  run.nbatch = (n + run.per - 1) / run.per;
  run.one_chain = run.nbatch >= 2 * gpus.devs.size() && !hs.subbatches_set;
  // device workers
  Pipeline pl;
  pl.out.resize(run.nbatch);
  std::vector<std::thread> workers;  // (a worker's batch objects and streams go with its thread)
  for (size_t w = 0; w < gpus.devs.size(); ++w) workers.emplace_back([&, w] { DeviceWorker(run, pl, gpus.idx[w], gpus.devs[w]).run(); });
  // ordered output: batch b's VT lines, its ED text started behind them
  AsqgWriter writer(out, pre->reads, pre->lengths, nt, hs, std::move(ahead), 16384, sigax_free, run.nbatch);
  BatchOut r;
  PhaseTimer wait(false);
  for (size_t b = 0; b < run.nbatch && pl.take(b, &r); ++b) {
    const size_t lo = b * run.per, cnt = std::min(run.per, n - lo);
    writer.add_batch(lo, cnt, r.substring.data(), r.edges, r.n_edges, wait.split());
    if (pt.on) progress_lines(lo, cnt, n, std::max<size_t>(threads, 1) * std::max<size_t>(batch, 1));
    wait.split();
  }
  // finish
  for (auto& t : workers) t.join();
  if (pl.failed) return fail(pl.error);
  pt.lap("GPU batches + VT lines");
  if (!writer.finish()) return fail("Failed to write ASQG " + output);
  pt.lap("ED lines + close");
  if (_keep_reads) _pre = pre;
  return true;
}

bool OverlapBuilder::rmdup(const std::string& input, const std::string& output, const std::string& duplicates, size_t threads,
                           size_t* processed) const {
  (void)processed;
  _error.clear();
  if (!_fmi || !_fmi->handle()) {
    _error = "FMIndex not loaded";
    return false;
  }
  // the chunk-parallel loader of build() (the reference reads record by record: src/overlap_builder.cpp:511-530); reads stay
  // packed, a piece of them goes to the device at a time
  const HostSettings hs;
  const unsigned nt = (unsigned)std::max<size_t>(threads, 1);
  ReadStore reads;
  if (!LoadReads(input, &reads, nt, hs)) {
    _error = "Failed to create DNASeqReader " + input;
    return false;
  }
  OutFile fasta(output), dups(duplicates);
  if (!fasta.ok() || !dups.ok()) {
    _error = "Failed to create FASTA " + output;
    return false;
  }
  const size_t n = reads.size();
  {
    std::vector<uint32_t> lengths, ranks;
    name_ranks(reads, nt, &lengths, &ranks);
    if (n > 0 && sigax_index_set_reads(_fmi->handle(), lengths.data(), ranks.data(), n) != SIGAX_OK) {
      _error = std::string("failed to load suffix array index: ") + sigax_last_error();
      return false;
    }
  }
  const size_t per = 1u << 20;
  std::string text;
  std::vector<uint64_t> offs;
  for (size_t base = 0; base < n; base += per) {
    const size_t cnt = std::min(per, n - base);
    offs.resize(cnt + 1);
    for (size_t i = 0; i <= cnt; ++i) offs[i] = reads.offs[base + i] - reads.offs[base];
    sigax_result res;
    if (sigax_overlap_batch(_fmi->handle(), reads.seqs.data() + reads.offs[base], offs.data(), (uint32_t)cnt, (uint32_t)base, 0,
                            SIGAX_DUPLICATE | SIGAX_EDGES, &res) != SIGAX_OK) {
      _error = std::string("rmdup failed: ") + sigax_last_error();
      return false;
    }
    // Hits2FastaConverter::convert (src/overlap_builder.cpp:578-616).  A kept overlap of a duplicate block is a
    // containment of the query with containedIdx() == 0 (both reads contained and id[0] > id[1], coord.h:185-194).
    std::vector<uint8_t> hasEdge(cnt, 0);
    for (uint64_t e = 0; e < res.n_edges; ++e) hasEdge[res.edges[e].query - base] = 1;
    for (size_t i = 0; i < cnt; ++i) {
      const std::string_view name = reads.name(base + i), seq = reads.seq(base + i);
      uint64_t numCopies = 0;
      for (uint64_t k = res.block_offs[i]; k < res.block_offs[i + 1]; ++k)
        numCopies += res.blocks[k].capped0_hi - res.blocks[k].capped0_lo + 1;
      bool contained = res.substring[i] != 0 || hasEdge[i] != 0;
      text.clear();
      text += '>';
      text.append(name.data(), name.size());
      if (contained) {
        text += ",seqrank=";
        append_u64(text, base + i);
      }
      text += ' ';
      text.append(name.data(), name.size());
      text += " NumDuplicates=";
      append_u64(text, numCopies);
      text += '\n';
      text.append(seq.data(), seq.size());
      text += '\n';
      (contained ? dups : fasta).write(text);
    }
    sigax_result_free(&res);
  }
  bool ok1 = fasta.close(), ok2 = dups.close();
  if (!ok1 || !ok2) {
    _error = "Failed to write rmdup output";
    return false;
  }
  return true;
}

}  // namespace sigah
