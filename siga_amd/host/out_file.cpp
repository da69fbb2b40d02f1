// siga_amd/host/out_file.cpp -- see out_file.hpp.
#include "out_file.hpp"

#include <algorithm>
#include <cstring>

#include "host_util.hpp"
#include "line_deflate.hpp"

namespace sigah {

OutFile::OutFile(const std::string& path, unsigned threads) : _f(nullptr), _gz(false), _bad(false), _crc(0), _total(0), _nt(threads) {
  const HostSettings hs;
  _async = !hs.sync_write;
  _level = hs.gzip_level;
  _gz = path.size() >= 3 && path.compare(path.size() - 3, 3, ".gz") == 0;
  _f = fopen(path.c_str(), "wb");
  // deflate at level 6 makes ~12 MB/s per thread on read text: the writer takes up to 128 threads whatever -t says
  _nt = std::max(_nt, std::min<unsigned>(std::max(1u, std::thread::hardware_concurrency()), 128));
  if (hs.host_threads_set) _nt = std::max(1, hs.host_threads);
  if (_f && _gz) {
    static const unsigned char hdr[10] = {0x1f, 0x8b, 8, 0, 0, 0, 0, 0, 0, 3};
    put(hdr, 10);
    _crc = crc32(0L, Z_NULL, 0);
  }
}

void OutFile::write(const char* p, size_t n) {
  _buf.append(p, n);
  if (_buf.size() >= kFlush) {
    std::vector<std::string> none;
    write_parts(none);
  }
}

void OutFile::write_parts(const std::vector<std::string>& parts, SpecBlocks* spec) {
  if (!_f) return;
  if (!_gz) {
    if (!_buf.empty()) put(_buf.data(), _buf.size());
    _buf.clear();
    for (const std::string& p : parts)
      if (!p.empty()) put(p.data(), p.size());
    return;
  }
  std::vector<const std::string*> segs;
  std::vector<size_t> start;  // offset of each segment in the pending text
  size_t total = 0;
  auto add = [&](const std::string* x) {
    if (x->empty()) return;
    segs.push_back(x);
    start.push_back(total);
    total += x->size();
  };
  add(&_buf);
  for (const std::string& p : parts) add(&p);
  const size_t nfull = total / kBlock;
  auto gather = [&](size_t off, size_t len, char* dst) {
    size_t k = (size_t)(std::upper_bound(start.begin(), start.end(), off) - start.begin()) - 1;
    while (len) {
      const size_t in = off - start[k], take = std::min(len, segs[k]->size() - in);
      memcpy(dst, segs[k]->data() + in, take);
      dst += take;
      off += take;
      len -= take;
      ++k;
    }
  };
  if (nfull) {
    std::vector<std::string> outs(nfull);
    std::vector<uLong> crcs(nfull, 0);
    const size_t first_block = (size_t)(_total / kBlock);
    parallel_for(nfull, _nt, [&](size_t i) {
      const size_t J = first_block + i;
      if (spec && J < spec->n && spec->state[J].load() == 1) {
        outs[i].swap(spec->out[J]);
        crcs[i] = spec->crc[J];
        return;
      }
      const size_t off = i * kBlock, k = (size_t)(std::upper_bound(start.begin(), start.end(), off) - start.begin()) - 1;
      if (off - start[k] + kBlock <= segs[k]->size()) {  // the block lies in one segment: no copy
        deflate_block(segs[k]->data() + (off - start[k]), kBlock, false, _level, &outs[i], &crcs[i]);
        return;
      }
      std::string tmp(kBlock, '\0');
      gather(off, kBlock, &tmp[0]);
      deflate_block(tmp.data(), kBlock, false, _level, &outs[i], &crcs[i]);
    });
    for (size_t i = 0; i < nfull; ++i) {
      put_owned(std::move(outs[i]));
      _crc = crc32_combine(_crc, crcs[i], (z_off_t)kBlock);
    }
    _total += nfull * kBlock;
  }
  std::string rest(total - nfull * kBlock, '\0');
  if (!rest.empty()) gather(nfull * kBlock, rest.size(), &rest[0]);
  _buf.swap(rest);
}

bool OutFile::close() {
  if (!_f) return true;
  std::vector<std::string> none;
  write_parts(none);
  if (_gz) {
    std::string out;
    uLong crc = 0;
    deflate_block(_buf.data(), _buf.size(), true, _level, &out, &crc);  // the last (possibly empty) block ends the deflate stream
    put(out.data(), out.size());
    _crc = crc32_combine(_crc, crc, (z_off_t)_buf.size());
    _total += _buf.size();
    _buf.clear();
    unsigned char tail[8];
    uint32_t c = (uint32_t)_crc, n = (uint32_t)_total;
    for (int i = 0; i < 4; ++i) { tail[i] = (unsigned char)(c >> (8 * i)); tail[4 + i] = (unsigned char)(n >> (8 * i)); }
    put(tail, 8);
  }
  finish_writes();
  // a short write (disk full, I/O error) leaves the stream's error flag set while fclose may still return 0
  bool ok = !_bad && ferror(_f) == 0;
  ok = fclose(_f) == 0 && ok;
  _f = nullptr;
  return ok;
}

// On read text (four-letter sequences with little to match inside a 32 KiB window) zlib's level 6, what the
// reference's gzip filter uses, makes 10 MB/s per thread, level 4 62 MB/s for a file 5 % larger; with the kernels done
// in milliseconds the deflate of the VT lines was the longest phase of `siga overlap`.  The writer's own coder
// (line_deflate.hpp: matches against the line above, field by field) makes 650 MB/s per thread on VT lines for a
// stream 9 % SMALLER than level 6, and 300 MB/s on ED lines at level 4's size.
// SIGA_GZIP_LEVEL=<1..9> sends every block through zlib at that level instead (6 = the reference's setting).
void OutFile::deflate_block(const char* in, size_t n, bool last, int level, std::string* out, uLong* crc) {
  *crc = ldef::crc32_fast(0, (const unsigned char*)in, n,
                          [](uint32_t c, const unsigned char* p, size_t k) { return (uint32_t)crc32(c, (const Bytef*)p, (uInt)k); });
  if (level == 0) {
    ldef::deflate_lines((const unsigned char*)in, n, last, out);
    return;
  }
  z_stream z;
  memset(&z, 0, sizeof(z));
  deflateInit2(&z, level, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY);
  out->resize(deflateBound(&z, (uLong)n) + 16);
  z.next_in = (Bytef*)in;
  z.avail_in = (uInt)n;
  z.next_out = (Bytef*)&(*out)[0];
  z.avail_out = (uInt)out->size();
  deflate(&z, last ? Z_FINISH : Z_SYNC_FLUSH);
  out->resize(out->size() - z.avail_out);
  deflateEnd(&z);
}
// The bytes go to the file from a thread of their own (1.2 GB of deflate blocks at BASELINE configs[2]: 0.26 s of
// fwrite that the thread formatting the next batch's lines used to spend between two batches); at most 1 GiB waits.
// SIGA_SYNC_WRITE=1: written by the caller.
void OutFile::put(const void* p, size_t n) {
  if (!n) return;
  if (!_async) {
    if (fwrite(p, 1, n, _f) != n) _bad = true;
    return;
  }
  put_owned(std::string((const char*)p, n));
}
void OutFile::put_owned(std::string&& s) {
  if (s.empty()) return;
  if (!_async) {
    if (fwrite(s.data(), 1, s.size(), _f) != s.size()) _bad = true;
    return;
  }
  std::unique_lock<std::mutex> g(_wmu);
  if (!_wt.joinable()) _wt = std::thread([this] { drain(); });
  _wcv.wait(g, [&] { return _wq_bytes <= ((size_t)1 << 30); });
  _wq_bytes += s.size();
  _wq.push_back(std::move(s));
  _wcv.notify_all();
}
void OutFile::drain() {
  std::unique_lock<std::mutex> g(_wmu);
  for (;;) {
    _wcv.wait(g, [&] { return !_wq.empty() || _wdone; });
    if (_wq.empty()) return;
    std::deque<std::string> mine;
    mine.swap(_wq);
    g.unlock();
    size_t bytes = 0;
    for (const std::string& x : mine) {
      if (!_bad && fwrite(x.data(), 1, x.size(), _f) != x.size()) _bad = true;
      bytes += x.size();
    }
    mine.clear();
    g.lock();
    _wq_bytes -= bytes;
    _wcv.notify_all();
  }
}
void OutFile::finish_writes() {
  {
    std::lock_guard<std::mutex> g(_wmu);
    _wdone = true;
  }
  _wcv.notify_all();
  if (_wt.joinable()) _wt.join();
}

}  // namespace sigah
