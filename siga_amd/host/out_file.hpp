// siga_amd/host/out_file.hpp -- internal: the output stream of the host library (plain, or block-parallel gzip by name).
#ifndef SIGA_AMD_HOST_OUT_FILE_HPP_
#define SIGA_AMD_HOST_OUT_FILE_HPP_

#include <zlib.h>

#include <atomic>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

namespace sigah {

// Utils::ofstream (src/utils.cpp:92-126): gzip when the name ends with .gz.  The gzip stream is ONE member (what any
// gzip reader, boost's gzip_decompressor included, accepts) whose deflate data is produced block-wise by a pool of
// threads: every 1 MiB of the text, counted from the start of the stream, is deflated on its own as raw deflate ending in
// a sync flush, the blocks are concatenated in order and the CRC-32s are combined (the pigz scheme, without dictionary
// priming).  Block boundaries depend on the text alone, so the file's bytes do not depend on how many threads, batches
// or GPUs produced it.
// Blocks of the stream deflated ahead of their turn (VtAhead below): block J = bytes [J, J + 1) MiB of the text.  state: 0 not
// there, 1 ready (out/crc hold what deflate_block gives for the block's text), 2 the text has changed since.
// (a block whose text changes may still be on its way in the thread that deflates ahead: that thread only ever turns a 0 into
// a 1, so the 2 stays whichever of the two comes first)
struct SpecBlocks {
  std::vector<std::string> out;
  std::vector<uLong> crc;
  std::unique_ptr<std::atomic<uint8_t>[]> state;
  size_t n = 0;
  void resize(size_t k) {
    out.resize(k);
    crc.resize(k, 0);
    state.reset(new std::atomic<uint8_t>[k]);
    for (size_t i = 0; i < k; ++i) state[i].store(0);
    n = k;
  }
  void made(size_t J) {
    uint8_t none = 0;
    state[J].compare_exchange_strong(none, 1);
  }
};

class OutFile {
 public:
  explicit OutFile(const std::string& path, unsigned threads = 0);  // reads its own HostSettings
  ~OutFile() { close(); }
  bool ok() const { return _f != nullptr; }
  void write(const char* p, size_t n);
  void write(const std::string& s) { write(s.data(), s.size()); }
  // the concatenation of `parts` goes out next; whole blocks are deflated now (in parallel), the rest waits in _buf
  // (spec: blocks of this stream that were deflated ahead; the caller vouches that a block in state 1 holds the deflate of
  // exactly the text that arrives here for it)
  void write_parts(const std::vector<std::string>& parts, SpecBlocks* spec = nullptr);
  static size_t block_bytes() { return kBlock; }
  // one whole block of text deflated as write_parts would (level: HostSettings::gzip_level)
  static void deflate_ahead(const char* in, int level, std::string* out, uLong* crc) { deflate_block(in, kBlock, false, level, out, crc); }
  bool gz() const { return _gz; }
  static bool gz_name(const std::string& path) { return path.size() >= 3 && path.compare(path.size() - 3, 3, ".gz") == 0; }
  bool close();

 private:
  static const size_t kBlock = 1 << 20, kFlush = 64u << 20;
  static void deflate_block(const char* in, size_t n, bool last, int level, std::string* out, uLong* crc);
  void put(const void* p, size_t n);
  void put_owned(std::string&& s);
  void drain();
  void finish_writes();
  FILE* _f;
  bool _gz;
  std::atomic<bool> _bad;
  bool _async;
  int _level;  // SIGA_GZIP_LEVEL, 0: the writer's own coder
  std::thread _wt;
  std::mutex _wmu;
  std::condition_variable _wcv;
  std::deque<std::string> _wq;
  size_t _wq_bytes = 0;
  bool _wdone = false;
  uLong _crc;
  uint64_t _total;
  unsigned _nt;
  std::string _buf;
};

}  // namespace sigah

#endif
