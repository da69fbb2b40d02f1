// siga_amd/csrc/sigax_index.cpp -- include/sigax.h: error text, streams, the index files' readers, index open / clone /
// close, and the one-shot queries (Occ, k-mer counts, order check).  The index's optional tables: sigax_tables.cpp.
#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <string>

#include "sigax_internal.h"

// ------------------------------------------------------------------------------------------------------
// errors, settings
// ------------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

// the library's one error setter (sigax_internal.h)
int sigax_fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

extern "C" const char* sigax_last_error(void) { return g_err; }

const Settings& settings() {
  static const Settings s;
  return s;
}

extern "C" int sigax_stream_create(int device, void** stream) {
  if (!stream) return sigax_fail(SIGAX_E_ARG, "NULL argument");
  *stream = nullptr;
  HIP_TRY(hipSetDevice(device));
  hipStream_t s = nullptr;
  HIP_TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  *stream = (void*)s;
  return SIGAX_OK;
}

extern "C" void sigax_stream_destroy(int device, void* stream) {
  if (!stream) return;
  if (hipSetDevice(device) == hipSuccess) hipStreamDestroy((hipStream_t)stream);
}

extern "C" int sigax_device_count(int* n) {
  if (!n) return sigax_fail(SIGAX_E_ARG, "n is NULL");
  int c = 0;
  hipError_t e = hipGetDeviceCount(&c);
  if (e != hipSuccess) {
    *n = 0;
    return sigax_fail(SIGAX_E_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
  }
  *n = c;
  return SIGAX_OK;
}

// Whole file into memory; files of 64 MiB and more in slices on several threads (pread): one thread copies out of the
// page cache at 2 GB/s, and BASELINE configs[2]'s four index files are 3 GB.
static int read_file(const char* path, std::vector<uint8_t>* out) {
  const int fd = open(path, O_RDONLY);
  if (fd < 0) return sigax_fail(SIGAX_E_IO, "cannot open %s", path);
  struct stat st;
  if (fstat(fd, &st) != 0) {
    close(fd);
    return sigax_fail(SIGAX_E_IO, "cannot stat %s", path);
  }
  const size_t n = st.st_size > 0 ? (size_t)st.st_size : 0;
  try {
    out->resize(n);
  } catch (...) {  // no exception crosses the C boundary
    close(fd);
    return sigax_fail(SIGAX_E_IO, "%s: no memory for its %zu bytes", path, n);
  }
  const unsigned nt = n >= (64u << 20) ? std::min<unsigned>(std::max(1u, std::thread::hardware_concurrency()), 8u) : 1u;
  std::vector<int> shortread(nt, 0);
  auto slice = [&](unsigned k) {
    size_t at = n * k / nt;
    const size_t end = n * (k + 1) / nt;
    while (at < end) {
      const ssize_t got = pread(fd, out->data() + at, std::min<size_t>(end - at, (size_t)1 << 30), (off_t)at);
      if (got <= 0) {
        if (got < 0 && errno == EINTR) continue;
        shortread[k] = 1;
        return;
      }
      at += (size_t)got;
    }
  };
  std::vector<std::thread> th;
  for (unsigned k = 1; k < nt; ++k) th.emplace_back(slice, k);
  slice(0);
  for (auto& t : th) t.join();
  close(fd);
  for (unsigned k = 0; k < nt; ++k)
    if (shortread[k]) return sigax_fail(SIGAX_E_IO, "short read on %s", path);
  return SIGAX_OK;
}

// src/bwt.cpp:59-98: u16 magic 0xCACA, u64 nStrings, u64 nSymbols, u64 nRuns, i32 flag, then the RL units
static int parse_bwt(const std::vector<uint8_t>& buf, const char* path, u64* nstrings, u64* nsym, const uint8_t** runs,
                     u64* nruns) {
  if (buf.size() < 30) return sigax_fail(SIGAX_E_IO, "%s: truncated .bwt header", path);
  uint16_t magic;
  memcpy(&magic, buf.data(), 2);
  if (magic != 0xCACA) return sigax_fail(SIGAX_E_IO, "%s: bad .bwt magic", path);
  memcpy(nstrings, buf.data() + 2, 8);
  memcpy(nsym, buf.data() + 10, 8);
  memcpy(nruns, buf.data() + 18, 8);
  if (buf.size() < 30 + *nruns) return sigax_fail(SIGAX_E_IO, "%s: truncated .bwt payload", path);
  *runs = buf.data() + 30;
  return SIGAX_OK;
}

// src/suffix_array.cpp:57-95: "51914\n<strings>\n<elems>\n" then elems lines "<readIdx> <j>".  Tables of a million rows and
// more are parsed in chunks on the host's threads (BASELINE configs[2]: 2 x 20 M lines were 3 of the 3.9 s of `siga overlap`'s
// index load): chunks cut at line ends, lines counted, then every chunk parsed to its place.
static int parse_sai(const std::vector<uint8_t>& buf, const char* path, std::vector<uint32_t>* out) {
  const char* p = (const char*)buf.data();
  const char* e = p + buf.size();
  auto next = [&](const char*& q, const char* end, u64* v) -> bool {
    while (q < end && (*q < '0' || *q > '9')) ++q;
    if (q >= end) return false;
    u64 x = 0;
    while (q < end && *q >= '0' && *q <= '9') x = x * 10 + (u64)(*q++ - '0');
    *v = x;
    return true;
  };
  u64 magic = 0, strings = 0, elems = 0;
  if (!next(p, e, &magic) || magic != 0xCACA) return sigax_fail(SIGAX_E_IO, "%s: bad .sai magic", path);
  if (!next(p, e, &strings) || !next(p, e, &elems)) return sigax_fail(SIGAX_E_IO, "%s: truncated .sai header", path);
  if (elems > (u64)(e - p)) return sigax_fail(SIGAX_E_IO, "%s: truncated .sai body", path);  // every line takes bytes
  try {
    out->resize(elems);
  } catch (...) {
    return sigax_fail(SIGAX_E_IO, "%s: no memory for %llu rows", path, elems);
  }
  // one chunk, or as many as there are threads: [cut[k], cut[k+1]) starts right after a line end
  unsigned nt = elems >= (1u << 18) ? std::min<unsigned>(std::max(1u, std::thread::hardware_concurrency()), 16u) : 1u;
  if (p < e && *p == '\n') ++p;  // the header's own line end
  std::vector<const char*> cut(nt + 1, e);
  cut[0] = p;
  for (unsigned k = 1; k < nt; ++k) {
    const char* q = p + (u64)(e - p) * k / nt;
    q = (const char*)memchr(q, '\n', (size_t)(e - q));
    cut[k] = q ? q + 1 : e;
    if (cut[k] < cut[k - 1]) cut[k] = cut[k - 1];
  }
  std::vector<u64> lines(nt + 1, 0);
  auto count = [&](unsigned k) {
    u64 c = 0;
    for (const char* q = cut[k]; q < cut[k + 1];) {  // a line = something up to '\n' (or the end) holding a digit
      const char* nl = (const char*)memchr(q, '\n', (size_t)(cut[k + 1] - q));
      const char* le = nl ? nl : cut[k + 1];
      bool digit = false;
      for (const char* t = q; t < le && !digit; ++t) digit = *t >= '0' && *t <= '9';
      c += digit ? 1 : 0;
      q = le + 1;
    }
    lines[k + 1] = c;
  };
  std::vector<int> bad(nt, 0);
  std::vector<u64> badrow(nt, 0), badid(nt, 0);
  auto parse = [&](unsigned k) {
    const char* q = cut[k];
    for (u64 i = lines[k]; i < lines[k + 1] && i < elems; ++i) {
      u64 a = 0, b2 = 0;
      if (!next(q, cut[k + 1], &a) || !next(q, cut[k + 1], &b2)) { bad[k] = 1; badrow[k] = i; return; }
      if (a >= strings) { bad[k] = 2; badrow[k] = i; badid[k] = a; return; }
      (*out)[i] = (uint32_t)a;
    }
    // one pair per line is what `siga index` writes; a chunk with numbers left over is some other layout: parse serially
    u64 extra = 0;
    if (nt > 1 && !bad[k] && next(q, cut[k + 1], &extra)) bad[k] = 3;
  };
  auto run = [&](auto fn) {
    std::vector<std::thread> th;
    for (unsigned k = 1; k < nt; ++k) th.emplace_back(fn, k);
    fn(0u);
    for (auto& t : th) t.join();
  };
  for (;;) {
    if (nt > 1) {
      run(count);
      for (unsigned k = 0; k < nt; ++k) lines[k + 1] += lines[k];
    } else {
      lines[1] = elems;  // one chunk: the token stream as it comes, whatever the line layout
    }
    bool irregular = nt > 1 && lines[nt] != elems;
    if (!irregular) {
      run(parse);
      // numbers left over in a chunk, or a chunk that ran dry (pairs split across lines with the line count intact): some
      // other layout of a token stream that operator>> (src/suffix_array.cpp:57-95) may still accept -- the serial parse decides
      for (unsigned k = 0; k < nt; ++k) irregular = irregular || bad[k] == 3 || (nt > 1 && bad[k] == 1);
    }
    if (!irregular) break;
    nt = 1;  // once more, serially
    cut.assign(2, e);
    cut[0] = p;
    lines.assign(2, 0);
    bad.assign(1, 0);
    badrow.assign(1, 0);
    badid.assign(1, 0);
  }
  for (unsigned k = 0; k < nt; ++k) {
    if (bad[k] == 1) return sigax_fail(SIGAX_E_IO, "%s: truncated .sai body", path);
    if (bad[k] == 2) return sigax_fail(SIGAX_E_IO, "%s: read id %llu at row %llu, the table declares %llu strings", path, badid[k], badrow[k], strings);
  }
  return SIGAX_OK;
}

// Binary image of a parsed .sai beside the text file (<path>.bin: magic, size and mtime (ns) of the text, a checksum of its
// first and last 64 KiB, count, ids): parsing 5e7 decimal lines takes seconds, reading 200 MB does not.  A .sai is a
// permutation of 0..n-1, so every read set of n reads gives a text of the same size: the checksum is what tells a re-indexed
// prefix from the one the image was made of.  Stale or unreadable images are ignored and rewritten.
static const u64 SAI_IMAGE_MAGIC = 0x5349474153414932ull;  // "SIGASAI2"
static bool sai_text_stamp(const char* path, u64 stamp[3]) {
  struct stat st;
  if (stat(path, &st) != 0) return false;
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  u64 h = 1469598103934665603ull;  // FNV-1a over the head and the tail
  std::vector<unsigned char> buf(65536);
  auto eat = [&](size_t n) {
    for (size_t i = 0; i < n; ++i) h = (h ^ buf[i]) * 1099511628211ull;
  };
  eat(fread(buf.data(), 1, buf.size(), f));
  if ((u64)st.st_size > buf.size() && fseek(f, -(long)std::min<u64>(buf.size(), (u64)st.st_size - buf.size()), SEEK_END) == 0)
    eat(fread(buf.data(), 1, buf.size(), f));
  fclose(f);
  stamp[0] = (u64)st.st_size;
  stamp[1] = (u64)st.st_mtim.tv_sec * 1000000000ull + (u64)st.st_mtim.tv_nsec;
  stamp[2] = h;
  return true;
}
static bool sai_cache_load(const char* path, std::vector<uint32_t>* out) {
  u64 stamp[3];
  if (!sai_text_stamp(path, stamp)) return false;
  std::string cp = std::string(path) + ".bin";
  FILE* f = fopen(cp.c_str(), "rb");
  if (!f) return false;
  struct stat ist;
  u64 hdr[5];
  bool ok = fstat(fileno(f), &ist) == 0 && fread(hdr, 8, 5, f) == 5 && hdr[0] == SAI_IMAGE_MAGIC && hdr[1] == stamp[0] && hdr[2] == stamp[1] &&
            hdr[3] == stamp[2];
  // the count must be what the image file holds (a corrupt header must not size a vector) and a text of that size can hold
  // (every line is at least "0 0\n")
  ok = ok && hdr[4] <= 0xFFFFFFFFull && (u64)ist.st_size == 40 + 4 * hdr[4] && 4 * hdr[4] <= stamp[0];
  if (ok) {
    try {
      out->resize(hdr[4]);
      ok = hdr[4] == 0 || fread(out->data(), 4, hdr[4], f) == hdr[4];
    } catch (...) {
      ok = false;
    }
  }
  fclose(f);
  if (!ok) out->clear();
  return ok;
}
static void sai_cache_store(const char* path, const std::vector<uint32_t>& ids) {
  if (settings().no_sai_cache) return;
  u64 stamp[3];
  if (!sai_text_stamp(path, stamp)) return;
  // a temporary name of this process and thread: ranks of one job, or two runs on one prefix, write their own file and the
  // rename puts a complete one in place
  char uniq[64];
  snprintf(uniq, sizeof(uniq), ".tmp.%ld.%zx", (long)getpid(), std::hash<std::thread::id>()(std::this_thread::get_id()));
  std::string cp = std::string(path) + ".bin", tmp = cp + uniq;
  FILE* f = fopen(tmp.c_str(), "wbx");
  if (!f) return;  // read-only directory (or a leftover of this very name): no cache
  u64 hdr[5] = {SAI_IMAGE_MAGIC, stamp[0], stamp[1], stamp[2], (u64)ids.size()};
  bool ok = fwrite(hdr, 8, 5, f) == 5 && (ids.empty() || fwrite(ids.data(), 4, ids.size(), f) == ids.size());
  ok = fclose(f) == 0 && ok;
  if (ok) ok = rename(tmp.c_str(), cp.c_str()) == 0;
  if (!ok) remove(tmp.c_str());
}
static int load_sai(const char* path, std::vector<uint32_t>* out) {
  if (sai_cache_load(path, out)) return SIGAX_OK;
  std::vector<uint8_t> buf;
  int rc = read_file(path, &buf);
  if (rc == SIGAX_OK) rc = parse_sai(buf, path, out);
  if (rc == SIGAX_OK && out->size() >= (1u << 20)) sai_cache_store(path, *out);
  return rc;
}

static int upload(const void* src, size_t bytes, void** dst, u64* acct) {
  *dst = nullptr;
  size_t alloc = bytes ? bytes : 16;
  HIP_TRY(hipMalloc(dst, alloc));
  if (bytes) HIP_TRY(hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice));
  if (acct) *acct += alloc;
  return SIGAX_OK;
}

extern "C" void sigax_index_close(sigax_index* ix) {
  if (!ix) return;
  hipSetDevice(ix->device);
  if (ix->tab_thread) {
    ix->tab_thread->join();
    delete ix->tab_thread;
  }
  delete ix->tab_state;
  if (ix->deep_thread) {
    ix->deep_thread->join();
    delete ix->deep_thread;
  }
  delete ix->deep_state;
  for (int s = 0; s < 2; ++s) {
    if (ix->d_deep[s]) hipFree(ix->d_deep[s]);
    if (ix->deep_new[s]) hipFree(ix->deep_new[s]);
    if (ix->d_slen[s]) hipFree(ix->d_slen[s]);
    if (ix->d_gran[s]) hipFree(ix->d_gran[s]);
    if (ix->d_gran2[s]) hipFree(ix->d_gran2[s]);
    if (ix->d_super2[s]) hipFree(ix->d_super2[s]);
    if (ix->d_sa[s]) hipFree(ix->d_sa[s]);
    if (ix->d_text[s]) hipFree(ix->d_text[s]);
    if (ix->d_xmap[s]) hipFree(ix->d_xmap[s]);
    if (ix->d_start[s]) hipFree(ix->d_start[s]);
    if (ix->d_super[s]) hipFree(ix->d_super[s]);
    if (ix->d_sai[s]) hipFree(ix->d_sai[s]);
  }
  if (ix->d_read_len) hipFree(ix->d_read_len);
  if (ix->d_name_rank) hipFree(ix->d_name_rank);
  if (ix->d_ptab) hipFree(ix->d_ptab);
  if (ix->ptab_ev) hipEventDestroy(ix->ptab_ev);
  if (ix->d_ktab) hipFree(ix->d_ktab);
  if (ix->d_csa) hipFree(ix->d_csa);
  if (ix->d_ctext) hipFree(ix->d_ctext);
  if (ix->d_cslen) hipFree(ix->d_cslen);
  if (ix->s_find) hipStreamDestroy(ix->s_find);
  if (ix->s_fx) hipStreamDestroy(ix->s_fx);
  if (ix->s_tail) hipStreamDestroy(ix->s_tail);
  if (ix->s_ord) hipStreamDestroy(ix->s_ord);
  delete ix->enqueue_mu;
  delete ix->cap_seen;
  delete ix;
}

// The index's own streams.  The finder is the critical path of a step: its stream gets the higher priority.
// SIGAX_CU_SPLIT=K (an experiment, off by default): the finder's stream is confined to all but K of the CUs and the
// filter/extract and tail streams to those K (CU mask bits interleave over XCDs and shader engines, so a run of mask
// bits is an even share of every XCD) -- no priorities then, hipExtStreamCreateWithCUMask takes none.
static hipError_t pipeline_streams(sigax_index* ix) {
  const int k = settings().cu_split;
  if (k > 0 && k < ix->n_cu) {
    const int words = (ix->n_cu + 31) / 32;
    std::vector<uint32_t> lo((size_t)words, 0u), hi((size_t)words, 0u);
    for (int c = 0; c < ix->n_cu; ++c) (c < ix->n_cu - k ? lo : hi)[(size_t)c / 32] |= 1u << (c % 32);
    hipError_t e = hipExtStreamCreateWithCUMask(&ix->s_find, (uint32_t)words, lo.data());
    if (e == hipSuccess) e = hipExtStreamCreateWithCUMask(&ix->s_fx, (uint32_t)words, hi.data());
    if (e == hipSuccess) e = hipExtStreamCreateWithCUMask(&ix->s_tail, (uint32_t)words, hi.data());
    if (e == hipSuccess) e = hipExtStreamCreateWithCUMask(&ix->s_ord, (uint32_t)words, hi.data());
    return e;
  }
  int prio_least = 0, prio_greatest = 0;
  hipError_t e = hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
  if (e == hipSuccess) e = hipStreamCreateWithPriority(&ix->s_find, hipStreamNonBlocking, prio_greatest);
  if (e == hipSuccess) e = hipStreamCreateWithPriority(&ix->s_fx, hipStreamNonBlocking, prio_least);
  if (e == hipSuccess) e = hipStreamCreateWithPriority(&ix->s_tail, hipStreamNonBlocking, prio_greatest);
  if (e == hipSuccess) e = hipStreamCreateWithPriority(&ix->s_ord, hipStreamNonBlocking, prio_greatest);
  return e;
}

// SIGAX_VERBOSE: where the time of opening an index goes
struct OpenClock {
  std::chrono::steady_clock::time_point t;
  OpenClock() : t(std::chrono::steady_clock::now()) {}
  void lap(const char* what) {
    const auto n = std::chrono::steady_clock::now();
    if (settings().verbose) fprintf(stderr, "[sigax] open: %-34s %7.3f s\n", what, std::chrono::duration<double>(n - t).count());
    t = n;
  }
};

extern "C" int sigax_index_open_mem(const uint8_t* runs, uint64_t n_runs, const uint8_t* rruns, uint64_t n_rruns,
                                    uint64_t n_symbols, uint64_t n_strings, const uint32_t* sai, const uint32_t* rsai,
                                    int device, sigax_index** out) {
  if (!out || (!runs && n_runs) || (!rruns && n_rruns)) return sigax_fail(SIGAX_E_ARG, "NULL argument");
  *out = nullptr;
  // Forward strand only (rruns == NULL, n_rruns == 0): the index `siga index --no-reverse` writes and `siga correct` reads
  // (src/correct.cpp:41-47 loads <prefix>.bwt alone; examples/siga-ecoli-miseq.sh:64-70).  Serves Occ, k-mer counts and the
  // corrector; overlap runs need both strands and fail with SIGAX_E_STATE.
  const bool fwd_only = rruns == nullptr && n_rruns == 0 && n_symbols > 0;
  const int nst = fwd_only ? 1 : 2;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return sigax_fail(SIGAX_E_DEVICE, "no HIP device visible: the overlap path has no CPU fallback");
  if (device < 0 || device >= ndev) return sigax_fail(SIGAX_E_ARG, "device %d out of range (%d visible)", device, ndev);
  HIP_TRY(hipSetDevice(device));
  OpenClock clk;
  sigax_index* ix = new sigax_index();
  memset(ix, 0, sizeof(*ix));
  ix->device = device;
  ix->enqueue_mu = new std::mutex();
  ix->cap_seen = new std::atomic<uint32_t>(0);
  if (hipDeviceGetAttribute(&ix->n_cu, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || ix->n_cu <= 0) ix->n_cu = 256;
  {
    const hipError_t e = pipeline_streams(ix);
    if (e != hipSuccess) {
      sigax_index_close(ix);
      return sigax_fail(SIGAX_E_DEVICE, "creating the pipeline streams: %s", hipGetErrorString(e));
    }
  }
  ix->n_symbols = n_symbols;
  ix->n_strings = n_strings;
  ix->fwd_only = fwd_only;
  // 64-bit positions when the BWT does not fit 32 bits (SIGAX_FORCE_WIDE=1 exercises that path on small inputs)
  ix->wide = n_symbols >= 0xFFFFFFF0ull || settings().force_wide;
  const uint8_t* rr[2] = {runs, rruns};
  u64 nr[2] = {n_runs, n_rruns};
  {
    // The second strand is decoded in the first one's scratch memory.  The session spans the two decodes only: its parked
    // scratch blocks are invisible to hipMemGetInfo, and the optional tables below are planned from the free memory.
    struct DecodeSession {
      DecodeSession() { sigax_build_session(1); }
      ~DecodeSession() { sigax_build_session(0); }
    } decode_session;
    for (int s = 0; s < nst; ++s) {
      u64 C[5], total[5], gb = 0, sb = 0;
      int rc = sigax_decode_strand(rr[s], nr[s], n_symbols, ix->wide, &ix->d_gran[s], &gb, &ix->d_super[s], &sb, C, total);
      if (rc != SIGAX_OK) {
        sigax_index_close(ix);
        return rc;
      }
      ix->device_bytes += gb + sb;
      ix->st[s].granules = (const uint32_t*)ix->d_gran[s];
      ix->st[s].super = (const u64*)ix->d_super[s];
      ix->st[s].n = n_symbols;
      for (int k = 0; k < 5; ++k) {
        ix->st[s].C[k] = C[k];
        ix->st[s].total[k] = total[k];
      }
    }
  }
  clk.lap("streams, upload + decode");
  for (int k = 0; k < 5 && !fwd_only; ++k) {
    if (ix->st[0].total[k] != ix->st[1].total[k]) {
      sigax_index_close(ix);
      return sigax_fail(SIGAX_E_IO, "forward and reverse BWT hold different symbol counts: not a .bwt/.rbwt pair");
    }
  }
  // Two-step tables for the block finder (2 bytes per symbol and strand), built on the device from the granules just
  // uploaded.  The finder then runs one launch per strand (chains 0,1 / 2,3): gathering from one table at a time keeps
  // the randomly accessed footprint small -- measured on MI355X per 1 M reads, index of 0.15 / 0.6 / 1.2 G symbols:
  // one-step finder 10.6 / 11.5 / 13.9 ms, two-step with both tables in one launch 7.3 / 9.1 / 17.4 ms (one lane per
  // 128-byte granule runs into address translation once more than ~4 GB are gathered from: tools/gather_probe3.hip),
  // two-step with one launch per strand 6.8 / 8.5 / 9.2 ms.  Up to 1.6 G symbols (u32 byte offsets into the table).
  // SIGAX_TWO_STEP=0 turns the tables off, SIGAX_TWO_STEP_MAX_SYMBOLS moves the limit (never beyond 2^31).
  {
    // every index with 32-bit positions: below SIGAX_COOP_MIN_SYMBOLS (2^31) the finder gathers per lane with u32 byte
    // offsets (k_find_n2, tables under 4 GiB), above it lines come cooperatively through LDS with 64-bit addresses (k_find_c2)
    // 64-bit-position indexes too: the lines' counters are then relative to 2^32-row superblocks (fm_layout.h)
    const bool want2 = n_symbols < settings().two_step_max_symbols && !settings().two_step_off;
    if (want2) {
      const u64 ng2 = n_symbols / SIGAX_GRAN2_SYMS + 1;
      void *cnt = nullptr, *offs = nullptr, *partial = nullptr, *total = nullptr;
      hipError_t e = hipMalloc(&cnt, 20 * ng2 * 4);
      if (e == hipSuccess) e = hipMalloc(&offs, (ng2 + 2) * 8);
      if (e == hipSuccess) e = hipMalloc(&partial, scan_partials_needed(ng2) * 8);
      if (e == hipSuccess) e = hipMalloc(&total, 8);
      const u64 nsup2 = ((ng2 - 1) >> (SIGAX_SUPER_SHIFT - 6)) + 1;
      for (int s = 0; s < nst && e == hipSuccess; ++s) {
        e = hipMalloc(&ix->d_gran2[s], ng2 * SIGAX_GRAN2_WORDS * 4);
        if (e != hipSuccess) break;
        ix->device_bytes += ng2 * SIGAX_GRAN2_WORDS * 4;
        if (ix->wide) {
          e = hipMalloc(&ix->d_super2[s], nsup2 * 20 * 8);
          if (e != hipSuccess) break;
        }
        launch_build2(ix->st[s], ix->wide, (uint32_t*)ix->d_gran2[s], (u64*)ix->d_super2[s], (uint32_t*)cnt, (u64*)offs, (u64*)partial,
                      (u64*)total, nullptr);
        e = hipDeviceSynchronize();
        if (e == hipSuccess) e = hipGetLastError();
        ix->st[s].gran2 = (const uint32_t*)ix->d_gran2[s];
        ix->st[s].super2 = (const u64*)ix->d_super2[s];
      }
      ix->split_strands = true;
      if (cnt) hipFree(cnt);
      if (offs) hipFree(offs);
      if (partial) hipFree(partial);
      if (total) hipFree(total);
      if (e != hipSuccess) {
        // the tables are an accelerator, not a requirement: without them the one-step finder runs
        (void)hipGetLastError();
        for (int s = 0; s < 2; ++s) {
          if (ix->d_gran2[s]) {
            hipFree(ix->d_gran2[s]);
            ix->device_bytes -= ng2 * SIGAX_GRAN2_WORDS * 4;
          }
          if (ix->d_super2[s]) hipFree(ix->d_super2[s]);
          ix->d_gran2[s] = ix->d_super2[s] = nullptr;
          ix->st[s].gran2 = nullptr;
          ix->st[s].super2 = nullptr;
        }
        ix->split_strands = false;
        if (settings().verbose) fprintf(stderr, "[sigax] two-step tables not built (%s): one-step finder\n", hipGetErrorString(e));
      }
    }
  }
  clk.lap("two-step tables");
  // Start tables of the finder (fm_layout.h): from 2^22 symbols on (the 2 x 268 MB and 20 ms are out of proportion for
  // less; SIGAX_FIND_START=1 forces them, =0 turns them off), an accelerator like the others.
  {
    const bool want = settings().find_start.value_or(n_symbols >= (1ull << 22));
    if (want && n_symbols > 0 && !fwd_only) {
      hipError_t e = hipSuccess;
      for (int s = 0; s < 2 && e == hipSuccess; ++s) {
        e = hipMalloc(&ix->d_start[s], start_table_bytes(ix->wide));
        if (e != hipSuccess) break;
        launch_start_build(ix->st[s], ix->st[1 - s], ix->wide, ix->d_start[s], nullptr);
        e = hipGetLastError();
      }
      if (e == hipSuccess) e = hipDeviceSynchronize();
      if (e != hipSuccess) {
        (void)hipGetLastError();
        for (int s = 0; s < 2; ++s) {
          if (ix->d_start[s]) hipFree(ix->d_start[s]);
          ix->d_start[s] = nullptr;
        }
      } else {
        for (int s = 0; s < 2; ++s) ix->st[s].start = ix->d_start[s];
        ix->device_bytes += 2 * start_table_bytes(ix->wide);
      }
    }
  }
  clk.lap("start tables");
  if (sai && rsai && !fwd_only) {
    const uint32_t* ss[2] = {sai, rsai};
    for (int s = 0; s < 2; ++s)  // k_edges indexes the read tables with these ids
      for (u64 i = 0; i < n_strings; ++i)
        if (ss[s][i] >= n_strings) {
          sigax_index_close(ix);
          return sigax_fail(SIGAX_E_IO, "%s table: read id %u at row %llu, the index holds %llu strings", s ? ".rsai" : ".sai", ss[s][i], i,
                      (u64)n_strings);
        }
    for (int s = 0; s < 2; ++s) {
      int rc = upload(ss[s], n_strings * 4, (void**)&ix->d_sai[s], &ix->device_bytes);
      if (rc != SIGAX_OK) {
        sigax_index_close(ix);
        return rc;
      }
    }
    ix->n_sai = n_strings;
  } else if (sai && fwd_only) {
    // the forward table alone: what sigax_locate_* names the reads with
    for (u64 i = 0; i < n_strings; ++i)
      if (sai[i] >= n_strings) {
        sigax_index_close(ix);
        return sigax_fail(SIGAX_E_IO, ".sai table: read id %u at row %llu, the index holds %llu strings", sai[i], i, (u64)n_strings);
      }
    int rc = upload(sai, n_strings * 4, (void**)&ix->d_sai[0], &ix->device_bytes);
    if (rc != SIGAX_OK) {
      sigax_index_close(ix);
      return rc;
    }
    ix->n_sai = n_strings;
  }
  clk.lap(".sai check + upload");
  if (fwd_only) {
    ix->tab_state = new std::atomic<int>(0);  // no extractor, no row tables
    ix->deep_state = new std::atomic<int>(0);
  } else {
    build_rowend(ix);  // after the .sai tables: with them the extractor's tables are direct maps (fm_layout.h)
  }
  clk.lap("row tables (plan, start of build)");
  *out = ix;
  return SIGAX_OK;
}

extern "C" int sigax_index_open(const char* bwt_path, const char* rbwt_path, const char* sai_path, const char* rsai_path,
                                int device, sigax_index** out) {
  if (!bwt_path || !out) return sigax_fail(SIGAX_E_ARG, "NULL argument");
  if (!rbwt_path || !rbwt_path[0]) {  // forward strand only (sigax_index_open_mem says what that serves)
    std::vector<uint8_t> fb;
    int rc = read_file(bwt_path, &fb);
    if (rc != SIGAX_OK) return rc;
    u64 ns = 0, nsym = 0, nruns = 0;
    const uint8_t* runs = nullptr;
    if ((rc = parse_bwt(fb, bwt_path, &ns, &nsym, &runs, &nruns)) != SIGAX_OK) return rc;
    std::vector<uint32_t> sai;  // with the forward .sai table the index also serves sigax_locate_*
    if (sai_path && sai_path[0]) {
      if ((rc = load_sai(sai_path, &sai)) != SIGAX_OK) return rc;
      if (sai.size() != ns) return sigax_fail(SIGAX_E_IO, ".sai table (%zu entries) does not match the %llu strings of the .bwt", sai.size(), ns);
    }
    return sigax_index_open_mem(runs, nruns, nullptr, 0, nsym, ns, sai.empty() ? nullptr : sai.data(), nullptr, device, out);
  }
  std::vector<uint8_t> fb, rb;
  std::vector<uint32_t> sai, rsai;
  const bool have_sai = sai_path && rsai_path && sai_path[0] && rsai_path[0];
  // the four files side by side (.sai text: tens of millions of lines at BASELINE configs[2] and [4]); the error text is
  // thread-local, so every side thread hands its own over
  int rcs[4] = {SIGAX_OK, SIGAX_OK, SIGAX_OK, SIGAX_OK};
  std::string errs[4];
  auto side = [&](int k, auto fn) {
    return std::thread([&rcs, &errs, k, fn] {
      rcs[k] = fn();
      if (rcs[k] != SIGAX_OK) errs[k] = g_err;
    });
  };
  std::vector<std::thread> sides;
  // the HIP runtime comes up (0.2-0.3 s in a fresh process) while the files are read, not after them
  sides.push_back(std::thread([device] {
    if (hipSetDevice(device) == hipSuccess) (void)hipFree(nullptr);
    (void)hipGetLastError();
  }));
  sides.push_back(side(1, [&] { return read_file(rbwt_path, &rb); }));
  if (have_sai) {
    sides.push_back(side(2, [&] { return load_sai(sai_path, &sai); }));
    sides.push_back(side(3, [&] { return load_sai(rsai_path, &rsai); }));
  }
  OpenClock clk;
  rcs[0] = read_file(bwt_path, &fb);
  if (rcs[0] != SIGAX_OK) errs[0] = g_err;
  clk.lap(".bwt read");
  for (auto& t : sides) t.join();
  clk.lap(".rbwt read, .sai tables parsed");
  for (int k = 0; k < 2; ++k)
    if (rcs[k] != SIGAX_OK) return sigax_fail(rcs[k], "%s", errs[k].c_str());
  int rc;
  u64 ns[2], nsym[2], nruns[2];
  const uint8_t* runs[2];
  if ((rc = parse_bwt(fb, bwt_path, &ns[0], &nsym[0], &runs[0], &nruns[0])) != SIGAX_OK) return rc;
  if ((rc = parse_bwt(rb, rbwt_path, &ns[1], &nsym[1], &runs[1], &nruns[1])) != SIGAX_OK) return rc;
  if (ns[0] != ns[1] || nsym[0] != nsym[1]) return sigax_fail(SIGAX_E_IO, "%s and %s describe different read sets", bwt_path, rbwt_path);
  for (int k = 2; k < 4; ++k)  // what is wrong with the .bwt files is said first, as when the files were read one by one
    if (rcs[k] != SIGAX_OK) return sigax_fail(rcs[k], "%s", errs[k].c_str());
  if (have_sai && (sai.size() != ns[0] || rsai.size() != ns[0]))
    return sigax_fail(SIGAX_E_IO, ".sai tables (%zu, %zu entries) do not match the %llu strings of the .bwt", sai.size(), rsai.size(), ns[0]);
  return sigax_index_open_mem(runs[0], nruns[0], runs[1], nruns[1], nsym[0], ns[0], have_sai ? sai.data() : nullptr,
                              have_sai ? rsai.data() : nullptr, device, out);
}

// Replica of an open index on another GPU of the node, copied device to device (xGMI between MI355X peers) instead of
// being decoded and uploaded again: SURVEY.md 8(e) "index broadcast at start-up".
extern "C" int sigax_index_clone(const sigax_index* src, int device, sigax_index** out) {
  if (!src || !out) return sigax_fail(SIGAX_E_ARG, "NULL argument");
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return sigax_fail(SIGAX_E_DEVICE, "no HIP device visible");
  if (device < 0 || device >= ndev) return sigax_fail(SIGAX_E_ARG, "device %d out of range (%d visible)", device, ndev);
  HIP_TRY(hipSetDevice(device));
  if (device != src->device) {
    int can = 0;
    if (hipDeviceCanAccessPeer(&can, device, src->device) == hipSuccess && can) (void)hipDeviceEnablePeerAccess(src->device, 0);
    (void)hipGetLastError();  // already enabled is fine; hipMemcpyPeer works either way (staged when there is no direct path)
  }
  sigax_index* ix = new sigax_index();
  memset(ix, 0, sizeof(*ix));
  ix->device = device;
  ix->enqueue_mu = new std::mutex();
  ix->cap_seen = new std::atomic<uint32_t>(src->cap_seen->load());
  ix->n_cu = src->n_cu;
  (void)hipDeviceGetAttribute(&ix->n_cu, hipDeviceAttributeMultiprocessorCount, device);
  {
    const hipError_t e = pipeline_streams(ix);
    if (e != hipSuccess) {
      sigax_index_close(ix);
      return sigax_fail(SIGAX_E_DEVICE, "creating the pipeline streams: %s", hipGetErrorString(e));
    }
  }
  ix->wide = src->wide;
  ix->n_symbols = src->n_symbols;
  ix->n_strings = src->n_strings;
  ix->n_sai = src->n_sai;
  ix->n_meta = src->n_meta;
  ix->max_read_len = src->max_read_len;
  ix->split_strands = src->split_strands;
  ix->fwd_only = src->fwd_only;
  const u64 ngran = src->n_symbols / SIGAX_GRANULE_SYMS + 1;
  const u64 nsuper = ((ngran - 1) >> (SIGAX_SUPER_SHIFT - 7)) + 1;
  const u64 ng2 = src->n_symbols / SIGAX_GRAN2_SYMS + 1;
  auto copy = [&](void** dst, const void* from, size_t bytes) -> int {
    *dst = nullptr;
    if (!from) return SIGAX_OK;
    HIP_TRY(hipMalloc(dst, bytes ? bytes : 16));
    if (bytes) HIP_TRY(hipMemcpyPeer(*dst, device, from, src->device, bytes));
    ix->device_bytes += bytes;
    return SIGAX_OK;
  };
  int rc = SIGAX_OK;
  for (int s = 0; s < 2 && rc == SIGAX_OK; ++s) {
    rc = copy(&ix->d_gran[s], src->d_gran[s], ngran * 64);
    if (rc == SIGAX_OK) rc = copy(&ix->d_super[s], src->d_super[s], nsuper * 32);
    if (rc == SIGAX_OK) rc = copy(&ix->d_gran2[s], src->d_gran2[s], ng2 * SIGAX_GRAN2_WORDS * 4);
    if (rc == SIGAX_OK) rc = copy(&ix->d_super2[s], src->d_super2[s], (((ng2 - 1) >> (SIGAX_SUPER_SHIFT - 6)) + 1) * 20 * 8);
    if (rc == SIGAX_OK) rc = copy((void**)&ix->d_sai[s], src->d_sai[s], src->n_sai * 4);
    if (rc == SIGAX_OK) rc = copy(&ix->d_start[s], src->d_start[s], start_table_bytes(src->wide));
    ix->st[s] = src->st[s];
    ix->st[s].sa = nullptr;
    ix->st[s].xmap = nullptr;
    ix->st[s].text = nullptr;
    ix->st[s].deep = nullptr;  // the replica builds its own (sigax_index_prepare_overlap, or once it is reused)
    ix->st[s].deep_slots = 0;
    ix->st[s].deep_k = 0;
    ix->st[s].granules = (const uint32_t*)ix->d_gran[s];
    ix->st[s].super = (const u64*)ix->d_super[s];
    ix->st[s].gran2 = (const uint32_t*)ix->d_gran2[s];
    ix->st[s].super2 = (const u64*)ix->d_super2[s];
    ix->st[s].start = ix->d_start[s];
  }
  if (rc == SIGAX_OK) rc = copy((void**)&ix->d_read_len, src->d_read_len, src->n_meta * 4);
  if (rc == SIGAX_OK) rc = copy((void**)&ix->d_name_rank, src->d_name_rank, src->n_meta * 4);
  if (rc != SIGAX_OK) {
    sigax_index_close(ix);
    return rc;
  }
  if (ix->fwd_only) {
    ix->tab_state = new std::atomic<int>(0);
    ix->deep_state = new std::atomic<int>(0);
  } else {
    build_rowend(ix);  // plans its own row tables; built on this device once it is reused (or prepared)
  }
  *out = ix;
  return SIGAX_OK;
}

extern "C" int sigax_index_info_get(const sigax_index* ix, sigax_index_info* out) {
  if (!ix || !out) return sigax_fail(SIGAX_E_ARG, "NULL argument");
  out->n_symbols = ix->n_symbols;
  out->n_strings = ix->n_strings;
  out->device_bytes = ix->device_bytes;
  for (int k = 0; k < 5; ++k) out->pred[k] = ix->st[0].C[k];
  out->device = ix->device;
  out->wide = ix->wide ? 1 : 0;
  return SIGAX_OK;
}

extern "C" int sigax_index_set_reads(sigax_index* ix, const uint32_t* lengths, const uint32_t* name_rank, uint64_t n) {
  if (!ix || !lengths || !name_rank) return sigax_fail(SIGAX_E_ARG, "NULL argument");
  if (n != ix->n_strings) return sigax_fail(SIGAX_E_ARG, "%llu reads given, index holds %llu", (u64)n, ix->n_strings);
  HIP_TRY(hipSetDevice(ix->device));
  if (ix->d_read_len) hipFree(ix->d_read_len);
  if (ix->d_name_rank) hipFree(ix->d_name_rank);
  ix->d_read_len = ix->d_name_rank = nullptr;
  int rc = upload(lengths, n * 4, (void**)&ix->d_read_len, &ix->device_bytes);
  if (rc == SIGAX_OK) rc = upload(name_rank, n * 4, (void**)&ix->d_name_rank, &ix->device_bytes);
  if (rc == SIGAX_OK) {
    ix->n_meta = n;
    uint32_t mx = 0;
    for (uint64_t i = 0; i < n; ++i) mx = std::max(mx, lengths[i]);
    ix->max_read_len = mx;
    if (ix->tab_plan) plan_row_tables(ix);  // planned with an estimate of the longest stretch, not started yet: now with the bound
  }
  return rc;
}

// Are the BWT rows of strand `which` in the suffix order of record?  Checked on the device from the row table and the
// stretch text (built now if they were only planned): every pair of adjacent rows.  For tests of the index builder at
// sizes no second suffix sorter reaches in reasonable time.
extern "C" int sigax_index_check_order(sigax_index* ix, int which, uint64_t* n_bad, uint64_t* first_bad, uint64_t* n_undecided) {
  if (!ix || which < 0 || which > 1 || !n_bad) return sigax_fail(SIGAX_E_ARG, "bad argument");
  HIP_TRY(hipSetDevice(ix->device));
  if (!ix->d_sai[which] || !ix->d_read_len) return sigax_fail(SIGAX_E_STATE, "the order check needs the .sai tables and sigax_index_set_reads()");
  if (ix->st[which].C[1] != ix->n_strings) return sigax_fail(SIGAX_E_STATE, "reads with non-ACGT bases: stretches are not reads, order not checkable");
  {
    std::lock_guard<std::mutex> lock(*ix->enqueue_mu);
    row_tables_now(ix);
  }
  if (!ix->st[which].text) return sigax_fail(SIGAX_E_STATE, "no extractor tables on this index (memory short or turned off)");
  // The check reads the suffix array.  An index that runs on direct maps has none: a bare row table of this strand is
  // built for the duration of the call (two LF walks over the strand).
  FmStrand cs = ix->st[which];
  DevGuard tg;
  if (!cs.sa) {
    const u64 n_stretch = cs.C[1];
    void* info = nullptr;
    u32* d_max = nullptr;
    HIP_TRY(tg.alloc(&info, std::max<u64>(n_stretch, 1) * 8));
    HIP_TRY(tg.alloc((void**)&d_max, 8));
    HIP_TRY(hipMemset(d_max, 0, 8));
    launch_stretch_scan(cs, ix->wide, n_stretch, (u64*)info, d_max, nullptr);
    HIP_TRY(hipGetLastError());
    u32 maxlen = 0;
    HIP_TRY(hipMemcpy(&maxlen, d_max, 4, hipMemcpyDeviceToHost));
    const RowTabGeom g = row_tab_geom(ix, maxlen, 0);
    if (g.sa_bits > 57) return sigax_fail(SIGAX_E_STATE, "stretches too long for a row table");
    void* sa = nullptr;
    HIP_TRY(tg.alloc(&sa, g.sa_bytes));
    HIP_TRY(hipMemset(sa, 0, g.sa_bytes));
    launch_rows_fill(cs, ix->wide, n_stretch, (const u64*)info, (unsigned char*)sa, g.sa_bits, g.ld_bits, g.t_bits, nullptr, g.text_stride, nullptr,
                     nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipDeviceSynchronize());
    cs.sa = (const unsigned char*)sa;
    cs.sa_bits = g.sa_bits;
    cs.ld_bits = g.ld_bits;
    cs.t_bits = g.t_bits;
  }
  DevGuard g;
  uint32_t* isai = nullptr;
  u64* bad = nullptr;
  HIP_TRY(g.alloc((void**)&isai, ix->n_strings * 4));
  HIP_TRY(g.alloc((void**)&bad, 32));
  const u64 init[4] = {0, ~0ull, 0, 0};
  HIP_TRY(hipMemcpy(bad, init, 32, hipMemcpyHostToDevice));
  launch_suffix_order_check(cs, ix->d_sai[which], isai, ix->d_read_len, ix->n_strings, bad, nullptr);
  HIP_TRY(hipGetLastError());
  u64 out[4];
  HIP_TRY(hipMemcpy(out, bad, 32, hipMemcpyDeviceToHost));
  *n_bad = out[0];
  if (first_bad) *first_bad = out[1];
  if (n_undecided) *n_undecided = out[2];
  return SIGAX_OK;
}

extern "C" int sigax_occ_batch(sigax_index* ix, int which, const uint64_t* positions, uint64_t n, uint64_t* counts5) {
  if (!ix || (n && (!positions || !counts5)) || which < 0 || which > 1) return sigax_fail(SIGAX_E_ARG, "bad argument");
  if (which == 1 && ix->fwd_only) return sigax_fail(SIGAX_E_STATE, "the index was opened without its reverse strand");
  HIP_TRY(hipSetDevice(ix->device));
  if (n == 0) return SIGAX_OK;
  u64 *d_pos = nullptr, *d_out = nullptr;
  DevGuard g;
  HIP_TRY(g.alloc((void**)&d_pos, n * 8));
  HIP_TRY(g.alloc((void**)&d_out, n * 40));
  HIP_TRY(hipMemcpy(d_pos, positions, n * 8, hipMemcpyHostToDevice));
  launch_occ_batch(ix->st[which], ix->wide, d_pos, n, d_out, 0);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(counts5, d_out, n * 40, hipMemcpyDeviceToHost));
  return SIGAX_OK;
}

extern "C" int sigax_kmer_count_batch(sigax_index* ix, const char* kmers, uint32_t k, uint64_t n, uint64_t* counts) {
  if (!ix || k == 0 || (n && (!kmers || !counts))) return sigax_fail(SIGAX_E_ARG, "bad argument");
  HIP_TRY(hipSetDevice(ix->device));
  if (n == 0) return SIGAX_OK;
  unsigned char* d_k = nullptr;
  u64* d_out = nullptr;
  DevGuard g;
  HIP_TRY(g.alloc((void**)&d_k, n * k));
  HIP_TRY(g.alloc((void**)&d_out, n * 8));
  HIP_TRY(hipMemcpy(d_k, kmers, n * k, hipMemcpyHostToDevice));
  launch_kmer_count(ix->st[0], ix->wide, d_k, k, n, d_out, 0);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpy(counts, d_out, n * 8, hipMemcpyDeviceToHost));
  return SIGAX_OK;
}
