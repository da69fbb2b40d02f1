// siga_amd/host/reads.cpp -- reading the reads: the bzip2 shim, the record-at-a-time readers of siga_host.hpp and the
// chunk-parallel loader of reads.hpp.
#include "reads.hpp"

#include <zlib.h>

#include <dlfcn.h>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstring>

#include "siga_host.hpp"

namespace sigah {

// ------------------------------------------------------------------------------------------------------
// bzip2 input (Utils::ifstream, src/utils.cpp:50-126: ".bz2" goes through a bzip2 filter).  The image has libbz2's shared
// library but not its header: the three entry points of its streaming interface are bound at run time (the bz_stream layout
// is libbz2's documented public one); without the library a .bz2 input fails to open.
// ------------------------------------------------------------------------------------------------------
namespace {
struct BzStream {
  char* next_in;
  unsigned int avail_in, total_in_lo32, total_in_hi32;
  char* next_out;
  unsigned int avail_out, total_out_lo32, total_out_hi32;
  void* state;
  void* (*bzalloc)(void*, int, int);
  void (*bzfree)(void*, void*);
  void* opaque;
};
struct Bz2Lib {
  int (*init)(BzStream*, int, int) = nullptr;
  int (*run)(BzStream*) = nullptr;
  int (*end)(BzStream*) = nullptr;
  Bz2Lib() {
    void* h = dlopen("libbz2.so.1.0", RTLD_NOW);
    if (!h) h = dlopen("libbz2.so.1", RTLD_NOW);
    if (!h) return;
    init = (int (*)(BzStream*, int, int))dlsym(h, "BZ2_bzDecompressInit");
    run = (int (*)(BzStream*))dlsym(h, "BZ2_bzDecompress");
    end = (int (*)(BzStream*))dlsym(h, "BZ2_bzDecompressEnd");
    if (!init || !run || !end) init = nullptr;
  }
};
}  // namespace
static bool is_bz2(const unsigned char* magic, ssize_t got) { return got >= 3 && magic[0] == 'B' && magic[1] == 'Z' && magic[2] == 'h'; }
// the whole of a (possibly multi-stream) bzip2 file, decompressed; false on a corrupt or truncated stream
static bool bz2_expand(const std::vector<char>& in, std::vector<char>* out) {
  static const Bz2Lib lib;
  if (!lib.init) return false;
  out->resize(std::max<size_t>(in.size() * 5, 1 << 20));
  size_t len = 0, pos = 0;
  while (pos < in.size()) {
    BzStream z;
    memset(&z, 0, sizeof(z));
    if (lib.init(&z, 0, 0) != 0) return false;
    int rc = 0;
    while (rc == 0) {
      if (out->size() - len < (1u << 20)) out->resize(out->size() * 2);
      z.next_in = const_cast<char*>(in.data()) + pos;
      z.avail_in = (unsigned)std::min<size_t>(in.size() - pos, 1u << 30);
      z.next_out = out->data() + len;
      z.avail_out = (unsigned)std::min<size_t>(out->size() - len, 1u << 30);
      const unsigned in0 = z.avail_in, out0 = z.avail_out;
      rc = lib.run(&z);
      pos += in0 - z.avail_in;
      len += out0 - z.avail_out;
      if (rc == 0 && in0 == z.avail_in && out0 == z.avail_out) rc = -1;  // no progress: truncated
    }
    lib.end(&z);
    if (rc != 4) return false;  // BZ_STREAM_END
  }
  out->resize(len);
  return true;
}

// ------------------------------------------------------------------------------------------------------
// line source / sequence readers
// ------------------------------------------------------------------------------------------------------
class LineSource {
 public:
  explicit LineSource(const std::string& path) : _f(nullptr), _pos(0), _len(0), _eof(false), _err(false), _mpos(0), _ismem(false) {
    unsigned char magic[3] = {0, 0, 0};
    int fd = open(path.c_str(), O_RDONLY);
    if (fd < 0) return;
    const ssize_t got = pread(fd, magic, 3, 0);
    if (is_bz2(magic, got)) {  // expanded in memory, then served like a file
      std::vector<char> raw;
      struct stat st;
      bool ok = fstat(fd, &st) == 0;
      if (ok) {
        raw.resize((size_t)st.st_size);
        size_t n = 0;
        while (n < raw.size()) {
          ssize_t k = read(fd, raw.data() + n, raw.size() - n);
          if (k <= 0) break;
          n += (size_t)k;
        }
        ok = n == raw.size() && bz2_expand(raw, &_mem);
      }
      close(fd);
      _ismem = ok;
      return;
    }
    close(fd);
    _f = gzopen(path.c_str(), "rb");
  }
  ~LineSource() {
    if (_f) gzclose(_f);
  }
  bool ok() const { return _f != nullptr || _ismem; }
  bool failed() const { return _err; }  // a read error (corrupt .gz), as opposed to the end of the file
  int peek() {
    if (_pos >= _len && !fill()) return -1;
    return (unsigned char)_buf[_pos];
  }
  // std::getline semantics: false only when nothing at all could be read
  bool getline(std::string& line) {
    line.clear();
    bool any = false;
    while (true) {
      if (_pos >= _len && !fill()) return any;
      any = true;
      const char* b = _buf + _pos;
      const char* nl = (const char*)memchr(b, '\n', _len - _pos);
      if (nl) {
        line.append(b, nl - b);
        _pos += (nl - b) + 1;
        return true;
      }
      line.append(b, _len - _pos);
      _pos = _len;
    }
  }
  void rewind() {
    if (_f) gzrewind(_f);
    _mpos = 0;
    _pos = _len = 0;
    _eof = false;
  }

 private:
  bool fill() {
    if (_eof) return false;
    if (_ismem) {
      const size_t n = std::min(sizeof(_buf), _mem.size() - _mpos);
      if (n == 0) {
        _eof = true;
        return false;
      }
      memcpy(_buf, _mem.data() + _mpos, n);
      _mpos += n;
      _pos = 0;
      _len = n;
      return true;
    }
    int n = gzread(_f, _buf, sizeof(_buf));
    if (n <= 0) {
      if (n < 0) _err = true;  // a corrupt or truncated .gz is not the end of the reads
      _eof = true;
      return false;
    }
    _pos = 0;
    _len = (size_t)n;
    return true;
  }
  gzFile _f;
  char _buf[1 << 16];
  size_t _pos, _len;
  bool _eof, _err;
  std::vector<char> _mem;  // a .bz2 input, expanded
  size_t _mpos;
  bool _ismem;
};

static bool slurp(const std::string& path, FileImage* img) {
  std::vector<char>* out = &img->owned;
  int fd = open(path.c_str(), O_RDONLY);
  if (fd < 0) return false;
  unsigned char magic[3] = {0, 0, 0};
  ssize_t got = pread(fd, magic, 3, 0);
  struct stat st;
  if (fstat(fd, &st) != 0) {
    close(fd);
    return false;
  }
  if (is_bz2(magic, got)) {  // bzip2 (Utils::ifstream, src/utils.cpp:91-126)
    std::vector<char> raw((size_t)st.st_size);
    size_t n = 0;
    while (n < raw.size()) {
      ssize_t k = read(fd, raw.data() + n, raw.size() - n);
      if (k <= 0) break;
      n += (size_t)k;
    }
    close(fd);
    return n == raw.size() && bz2_expand(raw, out);
  }
  if (got >= 2 && magic[0] == 0x1f && magic[1] == 0x8b) {  // gzip (Utils::ifstream, src/utils.cpp:50-90)
    close(fd);
    gzFile f = gzopen(path.c_str(), "rb");
    if (!f) return false;
    gzbuffer(f, 1 << 20);
    out->resize(std::max<size_t>((size_t)st.st_size * 4, 1 << 20));
    size_t len = 0;
    for (;;) {
      if (out->size() - len < (1u << 20)) out->resize(out->size() * 2);
      int n = gzread(f, out->data() + len, (unsigned)std::min<size_t>(out->size() - len, 1u << 30));
      if (n < 0) {  // a corrupt or truncated .gz must not be taken for a shorter read set
        gzclose(f);
        return false;
      }
      if (n == 0) break;
      len += (size_t)n;
    }
    const bool whole = gzclose(f) == Z_OK;  // Z_BUF_ERROR: the stream ended inside a member
    out->resize(len);
    return whole;
  }
  if (S_ISREG(st.st_mode) && st.st_size >= (1 << 20)) {
    void* m = mmap(nullptr, (size_t)st.st_size, PROT_READ, MAP_PRIVATE, fd, 0);
    if (m != MAP_FAILED) {
      (void)madvise(m, (size_t)st.st_size, MADV_WILLNEED);
      img->map = (const char*)m;
      img->map_size = (size_t)st.st_size;
      close(fd);
      return true;
    }
  }
  out->resize((size_t)st.st_size);
  size_t len = 0;
  while (len < out->size()) {
    ssize_t n = read(fd, out->data() + len, out->size() - len);
    if (n <= 0) break;
    len += (size_t)n;
  }
  close(fd);
  out->resize(len);
  return true;
}

namespace {
struct ChunkOut {
  std::vector<uint64_t> head_off, seq_len, qual_off;
  std::vector<uint64_t> seq_off;  // by_ref: where the record's one sequence line starts in the file image
  std::vector<uint32_t> head_len;
  std::vector<char> seqs;
  bool by_ref = false;    // every record of the chunk has its bases on ONE line: they stay in the file image until the join
  size_t n_bases = 0;     // bases of the chunk's records (by_ref: nothing was copied; else seqs.size())
  bool stopped = false;   // the reader returned false inside this chunk: nothing after it is read
  bool nameless = false;  // a header with no text: its sequence lines leak into the next record (serial semantics only)
  bool open_empty = false;  // the chunk ends in a named record without sequence
};
}  // namespace

// FASTAReader::read over [b, e) of the file image (src/kseq.cpp:187-228); the chunk starts at a header line.
// by_ref: the bases are not copied here -- a record's sequence is remembered as a span of the file image, which works as
// long as every record has its bases on one line (reads: always); returns false at the first record that has not, and the
// caller parses the chunk again the copying way.  (BASELINE configs[2]'s 20 M reads: the chunk buffers were 3 GB written,
// read once by the join and unmapped again.)
static bool parse_fasta_chunk(const char* base, size_t b, size_t e, bool last_chunk, ChunkOut* o, bool by_ref) {
  bool have_name = false;
  uint64_t hoff = 0;
  uint32_t hlen = 0;
  o->by_ref = by_ref;
  if (!by_ref) o->seqs.reserve(o->seqs.size() + (e - b));  // a chunk's bases are fewer than its bytes: no regrowth
  size_t seq_start = o->seqs.size();
  uint64_t cur_off = 0, cur_len = 0;  // by_ref: the open record's sequence line
  unsigned cur_lines = 0;
  size_t p = b;
  auto cur_seq = [&]() -> size_t { return by_ref ? (size_t)cur_len : o->seqs.size() - seq_start; };
  auto emit = [&] {
    o->head_off.push_back(hoff);
    o->head_len.push_back(hlen);
    o->seq_len.push_back(cur_seq());
    if (by_ref) {
      o->seq_off.push_back(cur_off);
      o->n_bases += cur_len;
      cur_len = 0;
      cur_lines = 0;
    }
    seq_start = o->seqs.size();
  };
  while (p < e) {
    const char* nl = (const char*)memchr(base + p, '\n', e - p);
    size_t le = nl ? (size_t)(nl - base) : e;
    size_t ls = p;
    p = nl ? le + 1 : e;
    while (ls < le && is_space(base[ls])) ++ls;
    while (le > ls && is_space(base[le - 1])) --le;
    if (ls == le) continue;
    if (base[ls] == '>') {
      const size_t have = cur_seq();
      if (have > 0 && have_name && hlen > 0) {
        emit();
      } else if (have_name && hlen > 0) {  // a named record without sequence: the reader gives up here
        o->stopped = true;
        if (!by_ref) o->n_bases = o->seqs.size();
        return true;
      }
      if (have_name && hlen == 0) o->nameless = true;
      have_name = true;
      hoff = ls + 1;
      hlen = (uint32_t)(le - ls - 1);
    } else if (by_ref) {
      if (cur_lines != 0) return false;  // a second sequence line: not a span of the file
      cur_off = ls;
      cur_len = le - ls;
      cur_lines = 1;
    } else {
      o->seqs.insert(o->seqs.end(), base + ls, base + le);
    }
  }
  const size_t have = cur_seq();
  if (have_name && hlen == 0) o->nameless = true;
  if (have > 0 && have_name && hlen > 0) emit();
  else if (have_name && hlen > 0 && !last_chunk) o->open_empty = true;  // the next header makes the reader give up
  else if (have > 0 && !by_ref) o->seqs.resize(seq_start);
  if (!by_ref) o->n_bases = o->seqs.size();
  return true;
}

// FASTQReader::read (src/kseq.cpp:140-185), serial
static void parse_fastq(const char* base, size_t e, ChunkOut* o) {
  int state = 0;
  uint64_t hoff = 0, soff = 0;
  uint32_t hlen = 0, slen = 0;
  size_t p = 0;
  while (p < e) {
    const char* nl = (const char*)memchr(base + p, '\n', e - p);
    size_t le = nl ? (size_t)(nl - base) : e;
    size_t ls = p;
    p = nl ? le + 1 : e;
    while (ls < le && is_space(base[ls])) ++ls;
    while (le > ls && is_space(base[le - 1])) --le;
    if (ls == le) continue;
    if (state == 0) {
      if (base[ls] != '@') return;
      hoff = ls + 1;
      hlen = (uint32_t)(le - ls - 1);
      state = 1;
    } else if (state == 1) {
      soff = ls;
      slen = (uint32_t)(le - ls);
      state = 2;
    } else if (state == 2) {
      const size_t len = le - ls;
      const bool ends = len >= hlen && memcmp(base + le - hlen, base + hoff, hlen) == 0;
      if (base[ls] == '+' && (len == 1 || ends)) state = 3;
      else return;
    } else {
      if (le - ls != slen) return;
      o->head_off.push_back(hoff);
      o->head_len.push_back(hlen);
      o->seq_len.push_back(slen);
      o->qual_off.push_back(ls);
      o->seqs.insert(o->seqs.end(), base + soff, base + soff + slen);
      state = 0;
    }
  }
}

bool LoadReads(const std::string& path, ReadStore* rs, unsigned nt, const HostSettings& hs) {
  const bool timing = hs.timing_loader, huge = !hs.no_hugepages;
  auto t_last = std::chrono::steady_clock::now();
  auto lap = [&](const char* what) {
    const auto t = std::chrono::steady_clock::now();
    if (timing) fprintf(stderr, "[siga]     loader: %-20s %7.3f s\n", what, std::chrono::duration<double>(t - t_last).count());
    t_last = t;
  };
  if (!slurp(path, &rs->file)) return false;
  lap("file image");
  const char* base = rs->file.data();
  const size_t size = rs->file.size();
  if (size == 0 || (base[0] != '@' && base[0] != '>')) return false;  // DNASeqReaderFactory::create (src/kseq.cpp:127-138)
  rs->fastq = base[0] == '@';
  std::vector<ChunkOut> outs;
  if (rs->fastq) {
    outs.resize(1);
    parse_fastq(base, size, &outs[0]);
    outs[0].n_bases = outs[0].seqs.size();
  } else {
    // chunk starts: the first header line at or after i * size / K
    const size_t K = std::max<size_t>(1, std::min<size_t>((size_t)nt * 4, size >> 16));
    std::vector<size_t> starts(1, 0);
    for (size_t i = 1; i < K; ++i) {
      size_t p = i * (size / K);
      const char* nl = (const char*)memchr(base + p, '\n', size - p);
      if (!nl) break;
      p = (size_t)(nl - base) + 1;
      while (p < size) {  // find a line whose first non-blank character is '>'
        size_t q = p;
        while (q < size && base[q] != '\n' && is_space(base[q])) ++q;
        if (q < size && base[q] == '>') break;
        const char* n2 = (const char*)memchr(base + p, '\n', size - p);
        if (!n2) {
          p = size;
          break;
        }
        p = (size_t)(n2 - base) + 1;
      }
      if (p < size && p > starts.back()) starts.push_back(p);
    }
    outs.resize(starts.size());
    parallel_for(starts.size(), nt, [&](size_t i) {
      const size_t e = i + 1 < starts.size() ? starts[i + 1] : size;
      if (hs.loader_copy || !parse_fasta_chunk(base, starts[i], e, i + 1 == starts.size(), &outs[i], true)) {
        outs[i] = ChunkOut();
        parse_fasta_chunk(base, starts[i], e, i + 1 == starts.size(), &outs[i], false);
      }
    });
    bool nameless = false;
    for (auto& o : outs) nameless = nameless || o.nameless;
    if (nameless) {  // state leaks across records: only the serial walk reproduces it
      outs.assign(1, ChunkOut());
      parse_fasta_chunk(base, 0, size, true, &outs[0], false);
    }
  }
  lap("chunks parsed");
  // concatenate up to the point where the serial reader would have given up
  size_t nchunks = 0, n = 0, nb = 0;
  for (; nchunks < outs.size(); ++nchunks) {
    n += outs[nchunks].head_off.size();
    nb += outs[nchunks].n_bases;
    if (outs[nchunks].stopped || outs[nchunks].open_empty) {
      ++nchunks;
      break;
    }
  }
  rs->head_off.resize(n, huge);
  rs->head_len.resize(n, huge);
  rs->name_len.resize(n, huge);
  rs->offs.resize(n + 1, huge);
  rs->seqs.resize(nb, huge);
  if (rs->fastq) rs->qual_off.resize(n, huge);
  std::vector<size_t> rbase(nchunks + 1, 0), bbase(nchunks + 1, 0);
  for (size_t c = 0; c < nchunks; ++c) {
    rbase[c + 1] = rbase[c] + outs[c].head_off.size();
    bbase[c + 1] = bbase[c] + outs[c].n_bases;
  }
  parallel_for(nchunks, nt, [&](size_t c) {
    ChunkOut& o = outs[c];
    uint64_t off = bbase[c];
    for (size_t k = 0; k < o.head_off.size(); ++k) {
      const size_t r = rbase[c] + k;
      rs->head_off[r] = o.head_off[k];
      rs->head_len[r] = o.head_len[k];
      const char* h = base + o.head_off[k];
      uint32_t nl = 0;
      while (nl < o.head_len[k] && h[nl] != ' ' && h[nl] != '\t') ++nl;  // make_seq_name (src/kseq.cpp:71-79)
      rs->name_len[r] = nl;
      rs->offs[r] = off;
      if (o.by_ref) memcpy(rs->seqs.data() + off, base + o.seq_off[k], o.seq_len[k]);  // straight from the file image
      off += o.seq_len[k];
      if (rs->fastq) rs->qual_off[r] = o.qual_off[k];
    }
    if (!o.by_ref && !o.seqs.empty()) memcpy(rs->seqs.data() + bbase[c], o.seqs.data(), o.seqs.size());
    // the chunk's own buffers go back here, on this thread: left to the vector of chunks' destructor they were unmapped
    // one after the other (0.4 s of the 0.97 s BASELINE configs[2]'s reads took to load)
    std::vector<char>().swap(o.seqs);
    std::vector<uint64_t>().swap(o.head_off);
    std::vector<uint64_t>().swap(o.seq_len);
    std::vector<uint64_t>().swap(o.seq_off);
    std::vector<uint64_t>().swap(o.qual_off);
    std::vector<uint32_t>().swap(o.head_len);
  });
  rs->offs[n] = nb;
  lap("joined");
  return true;
}

static void trim(std::string& s) {  // boost::algorithm::trim
  auto sp = [](char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\v' || c == '\f' || c == '\r'; };
  size_t b = 0, e = s.size();
  while (b < e && sp(s[b])) ++b;
  while (e > b && sp(s[e - 1])) --e;
  if (b > 0 || e < s.size()) s = s.substr(b, e - b);
}

static void make_seq_name(std::string& name, std::string& comment) {  // src/kseq.cpp:71-79
  size_t i = name.find_first_of(" \t");
  if (i != std::string::npos) {
    comment = name.substr(i + 1);
    name.resize(i);
  } else {
    comment.clear();
  }
}

DNASeqReader::DNASeqReader() : _fastq(false) {}
DNASeqReader::~DNASeqReader() {}

DNASeqReader* DNASeqReader::create(const std::string& path) {
  std::unique_ptr<LineSource> src(new LineSource(path));
  if (!src->ok()) return nullptr;
  int c = src->peek();  // src/kseq.cpp:127-138
  if (c != '@' && c != '>') return nullptr;
  DNASeqReader* r = new DNASeqReader();
  r->_fastq = c == '@';
  r->_src = std::move(src);
  return r;
}

bool DNASeqReader::failed() const { return _src->failed(); }

void DNASeqReader::reset() {
  _name.clear();
  _src->rewind();
}

bool DNASeqReader::read(DNASeq& sequence) {
  std::string line;
  if (_fastq) {  // src/kseq.cpp:140-185
    int state = 0;
    while (_src->getline(line)) {
      trim(line);
      if (line.empty()) continue;
      if (state == 0) {
        if (line[0] != '@') return false;
        sequence.name = line.substr(1);
        state = 1;
      } else if (state == 1) {
        sequence.seq = line;
        state = 2;
      } else if (state == 2) {
        const std::string& nm = sequence.name;
        bool ends = line.size() >= nm.size() && line.compare(line.size() - nm.size(), nm.size(), nm) == 0;
        if (line[0] == '+' && (line.length() == 1 || ends)) state = 3;
        else return false;
      } else {
        if (line.length() != sequence.seq.length()) return false;
        sequence.quality = line;
        make_seq_name(sequence.name, sequence.comment);
        return true;
      }
    }
    return false;
  }
  // src/kseq.cpp:187-228
  std::string seq;
  while (_src->getline(line)) {
    trim(line);
    if (line.empty()) continue;
    if (line[0] == '>') {
      if (!seq.empty() && !_name.empty()) {
        sequence.name = _name;
        make_seq_name(sequence.name, sequence.comment);
        sequence.seq.swap(seq);
        sequence.quality.clear();
        _name = line.substr(1);
        return true;
      } else if (!_name.empty()) {
        return false;
      }
      _name = line.substr(1);
    } else {
      seq += line;
    }
  }
  if (!seq.empty() && !_name.empty()) {
    sequence.name = _name;
    make_seq_name(sequence.name, sequence.comment);
    sequence.seq.swap(seq);
    sequence.quality.clear();
    _name.clear();  // the reference's stream is at EOF here and never reads again
    return true;
  }
  return false;
}

bool ReadDNASequences(const std::string& file, DNASeqList& sequences, uint32_t flags) {  // src/kseq.cpp:230-256
  std::unique_ptr<DNASeqReader> reader(DNASeqReader::create(file));
  if (!reader) return false;
  DNASeq seq;
  while (reader->read(seq)) {
    if (!(flags & kSeqWithQuality)) seq.quality.clear();
    if (!(flags & kSeqWithComment)) seq.comment.clear();
    sequences.push_back(seq);
  }
  return !reader->failed();  // a corrupt .gz is an error, not a shorter read set
}

std::string Utils::stem(const std::string& filename) {  // src/utils.cpp:128-135
  auto ends = [](const std::string& s, const char* suf) {
    size_t n = strlen(suf);
    return s.size() >= n && s.compare(s.size() - n, n, suf) == 0;
  };
  if (ends(filename, ".gz")) return stem(filename.substr(0, filename.size() - 3));
  if (ends(filename, ".bz2")) return stem(filename.substr(0, filename.size() - 4));
  size_t slash = filename.find_last_of('/');
  std::string base = slash == std::string::npos ? filename : filename.substr(slash + 1);
  if (base == "." || base == "..") return base;
  size_t dot = base.find_last_of('.');
  return dot == std::string::npos ? base : base.substr(0, dot);
}


}  // namespace sigah
