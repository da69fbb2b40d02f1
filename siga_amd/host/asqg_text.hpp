// siga_amd/host/asqg_text.hpp -- internal: the text of an ASQG file (HT, VT, ED lines) from parsed reads, substring flags and
// edge records.  AsqgWriter is the one writer of OverlapBuilder::build() and of the CPU test hook sigah_format_asqg.
#ifndef SIGA_AMD_HOST_ASQG_TEXT_HPP_
#define SIGA_AMD_HOST_ASQG_TEXT_HPP_

#include <condition_variable>
#include <memory>
#include <mutex>
#include <string>
#include <string_view>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/sigax.h"
#include "host_util.hpp"
#include "out_file.hpp"
#include "reads.hpp"

namespace sigah {

std::string asqg_header(size_t minOverlap);
// one ED line, as the writer below formats a record, over two vertices given by name and length (the unitig graph of `siga unitig`)
void append_edge_line(std::string& o, const sigax_edge& e, std::string_view qn, std::string_view tn, uint64_t ql, uint64_t tl);

// ReadInfo{name,length} of the edge converter (src/overlap_builder.cpp:333-343) as lengths + rank of each name under
// std::string operator< (equal names, equal rank).  A sample sort on the host threads: names enter as (first eight bytes,
// big endian; index) pairs -- the file image is only gone back to on a tie --, splitters from a sample cut them into
// buckets of equal names' ranges, the buckets are sorted side by side, and the ranks follow from the distinct names
// counted per bucket.  (Round 2 merged sorted runs pairwise: the last merges ran on one thread, 1.3 s for 20 M names.)
void name_ranks(const ReadStore& rs, unsigned nt, std::vector<uint32_t>* lengths, std::vector<uint32_t>* ranks);

// VT lines ahead of the GPU.  A VT line is known from the reads file but for one character, the digit of SS:i: (is the read
// a substring of another: the device's answer), and in a set that went through `siga rmdup` -- what the extractor asks for,
// src/overlap_builder.cpp:755-756 -- that digit is 0.  So the text of every VT line is written with SS:i:0 as soon as the
// reads are parsed, and the 1 MiB blocks of the output stream (fixed offsets of the TEXT, whose length the digit does not
// change) are deflated, by threads of this object, while the index is still on its way to the GPU and while the batches
// run.  build() takes the chunks in input order once the batches that cover them are back: a chunk with a substring read
// is formatted again and the blocks it touches are deflated again by the writer; every other block goes to the file as
// it is.  The bytes of the file are the ones the in-order path writes.  An option (SIGA_VT_AHEAD=1), see HostSettings::vt_ahead_wanted().
class VtAhead {
 public:
  static constexpr size_t kChunk = 4096;  // reads per chunk of text
  VtAhead(const ReadStore* reads, unsigned nt, const std::string& header, bool gz, const HostSettings& hs);
  ~VtAhead();
  VtAhead(const VtAhead&) = delete;
  VtAhead& operator=(const VtAhead&) = delete;
  const std::string& header() const { return _header; }
  bool gz() const { return _gz; }
  size_t chunks() const { return _nchunks; }
  // The chunks [from, to) -- formatted, their blocks deflated -- with the substring flags of their reads applied; `parts`
  // takes their text.  Call with from = the previous call's to.
  void take(size_t from, size_t to, const uint8_t* substring, std::vector<std::string>* parts);
  SpecBlocks* blocks() { return _gz ? &_spec : nullptr; }
  // the text of chunks below `to` has left: the threads may run further ahead
  void taken(size_t to);

 private:
  void run();
  const ReadStore& _reads;
  unsigned _nt;
  std::string _header;
  bool _gz;
  int _level;  // HostSettings::gzip_level, for the blocks deflated ahead
  size_t _n, _nchunks = 0;
  std::vector<std::string> _text;
  std::vector<uint64_t> _off;  // _off[c]: where chunk c starts in the stream (the header first)
  SpecBlocks _spec;
  uint64_t _cap;  // text held ahead of the writer at most (SIGA_VT_AHEAD_BYTES)
  std::mutex _mu;
  std::condition_variable _cv;
  size_t _done = 0, _want = 0;
  uint64_t _taken_off = 0;
  bool _stop = false;
  std::thread _thread;
};

// The VT and ED lines of one ASQG file, batch by batch: what OverlapBuilder::build() does with the batches that come back from the
// GPUs, in input order (OverlapPostProcess, src/overlap_builder.cpp:291-329), and what the test hook does with the arrays it is given.
// The ED lines come after the last VT line, but their TEXT does not have to wait: while the GPUs work on the batches
// that follow, the host threads have time, so a batch's edge records are formatted as soon as its VT lines are out
// (up to 4 GiB of text held; beyond that the records wait and are formatted at the end, 16 bytes against ~45 each).
class AsqgWriter {
 public:
  // `out` has the header already.  ahead: the VT lines made ahead, or none (then they are formatted batch by batch).  ed_chunk: ED
  // lines per piece of text.  release: what gives a batch's edge records back (sigax_free), nullptr: they stay the caller's.
  // nbatch: the add_batch() calls to come at most.
  AsqgWriter(OutFile& out, const ReadStore& reads, const std::vector<uint32_t>& lengths, unsigned nt, const HostSettings& hs,
             std::unique_ptr<VtAhead> ahead, size_t ed_chunk, void (*release)(void*), size_t nbatch);
  ~AsqgWriter();  // joins the ED job, releases the records still held
  AsqgWriter(const AsqgWriter&) = delete;
  AsqgWriter& operator=(const AsqgWriter&) = delete;
  // The VT lines of reads [lo, lo + cnt) (substring: their flags, or nullptr for none set); the batch's edge records are taken
  // over and, under the hold limit, their ED text is started.  Batches come in input order.  wait_s: how long the caller
  // waited for the batch (for the SIGA_TIMING line).  num_diff: the last column of the records' ED lines (`siga overlap -e`), the
  // caller's until finish() has returned; nullptr: 0, as for every exact overlap.
  void add_batch(size_t lo, size_t cnt, const uint8_t* substring, const sigax_edge* edges, uint64_t n_edges, double wait_s = 0,
                 const uint32_t* num_diff = nullptr);
  // ED lines in hits order (Hit2OverlapConverter, src/overlap_builder.cpp:345-375 + :474-483), then the file is closed; false: a
  // write failed
  bool finish();

 private:
  void format_edges(size_t k);
  void join_ed() {
    if (_ed_job.joinable()) _ed_job.join();
  }
  OutFile& _out;
  const ReadStore& _reads;
  const uint32_t* _read_len;
  unsigned _nt;
  bool _timing;
  uint32_t _maxLen = 0, _max_name = 0;
  std::unique_ptr<VtAhead> _ahead;
  std::vector<uint8_t> _sub_all;  // (VT lines ahead) the substring flags of the reads whose chunk is not out yet
  size_t _ahead_from = 0;
  std::vector<std::string> _vt_parts;
  std::vector<std::pair<const sigax_edge*, uint64_t>> _edges;
  std::vector<const uint32_t*> _num_diff;  // per batch, or nullptr
  std::vector<std::vector<std::string>> _ed_text;
  size_t _ed_held = 0;
  const size_t _ed_hold_max, _ed_chunk;
  const bool _ed_inline;
  void (*_release)(void*);
  std::thread _ed_job;
};

}  // namespace sigah

#endif
