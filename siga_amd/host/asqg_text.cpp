// siga_amd/host/asqg_text.cpp -- see asqg_text.hpp: the VT and ED line formatters, the name ranks, VtAhead, AsqgWriter.
#include "asqg_text.hpp"

#include <cstring>

namespace sigah {

// TagValue<T>::fromstring (src/asqg.h:43-56): exactly three ':'-separated tokens, one-letter type code
static bool tag_tokens(const std::string& text, char code, std::string* value) {
  size_t a = text.find(':');
  if (a == std::string::npos) return false;
  size_t b = text.find(':', a + 1);
  if (b == std::string::npos) return false;
  if (text.find(':', b + 1) != std::string::npos) return false;
  if (b - a - 1 != 1 || text[a + 1] != code) return false;
  *value = text.substr(b + 1);
  return true;
}
static std::string first_word(const std::string& s) {  // std::istream >> std::string
  size_t b = 0;
  auto sp = [](char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\v' || c == '\f' || c == '\r'; };
  while (b < s.size() && sp(s[b])) ++b;
  size_t e = b;
  while (e < s.size() && !sp(s[e])) ++e;
  return s.substr(b, e - b);
}
static int parse_int(const std::string& s) {  // std::istream >> int (0 on failure, clamped on overflow)
  size_t i = 0;
  auto sp = [](char c) { return c == ' ' || c == '\t' || c == '\n' || c == '\v' || c == '\f' || c == '\r'; };
  while (i < s.size() && sp(s[i])) ++i;
  bool neg = false;
  if (i < s.size() && (s[i] == '+' || s[i] == '-')) neg = s[i++] == '-';
  if (i >= s.size() || s[i] < '0' || s[i] > '9') return 0;
  long long v = 0;
  while (i < s.size() && s[i] >= '0' && s[i] <= '9') {
    v = v * 10 + (s[i++] - '0');
    if (v > 4000000000LL) v = 4000000000LL;
  }
  if (neg) v = -v;
  if (v > 2147483647LL) v = 2147483647LL;
  if (v < -2147483648LL) v = -2147483648LL;
  return (int)v;
}

// OverlapPostProcess::operator() + VertexRecord << (src/overlap_builder.cpp:301-322, src/asqg.cpp:171-186)
static void write_vertex(std::string& o, std::string_view name, std::string_view comment_sv, std::string_view seq, bool substring) {
  bool hasCov = false, hasBar = false, hasExt = false;
  int cov = 0;
  std::string bar, ext, val;
  if (!comment_sv.empty()) {
    const std::string comment(comment_sv);
    size_t b = 0;
    while (true) {
      size_t e = comment.find(' ', b);
      std::string tok = comment.substr(b, e == std::string::npos ? std::string::npos : e - b);
      if (tok.compare(0, 2, "BX") == 0) {
        if (tag_tokens(tok, 'Z', &val)) { bar = first_word(val); hasBar = true; }
      } else if (tok.compare(0, 2, "CR") == 0) {
        if (tag_tokens(tok, 'i', &val)) { cov = parse_int(val); hasCov = true; }
      } else if (tok.compare(0, 2, "EX") == 0) {
        if (tag_tokens(tok, 'Z', &val)) { ext = first_word(val); hasExt = true; }
      }
      if (e == std::string::npos) break;
      b = e + 1;
    }
  }
  o += "VT\t";
  o.append(name.data(), name.size());
  o += '\t';
  o.append(seq.data(), seq.size());
  o += substring ? "\tSS:i:1" : "\tSS:i:0";
  if (hasCov) { o += "\tCR:i:"; o += std::to_string(cov); }
  if (hasBar) { o += "\tBX:Z:"; o += bar; }
  if (hasExt) { o += "\tEX:Z:"; o += ext; }
  o += '\n';
}

// EdgeRecord << (src/asqg.cpp:228-237, src/coord.cpp:4-80) with OverlapBlock::overlap's coordinates
// (src/overlap_builder.cpp:158-175)
// ... written through a raw pointer: the caller has room for the two names and 3 + 2 + 7 x 21 + 3 bytes more (22 M lines at
// BASELINE configs[2]: the capacity check of every append was a third of the formatting)
static inline char* put_u64(char* p, uint64_t v) {
  char tmp[24];
  int n = 0;
  do {
    tmp[n++] = (char)('0' + v % 10);
    v /= 10;
  } while (v);
  while (n) *p++ = tmp[--n];
  return p;
}
static const size_t kEdgeLineExtra = 3 + 2 + 7 * 21 + 3;
static inline char* write_edge_line(char* p, const sigax_edge& e, const std::string_view qn, const std::string_view tn, uint64_t ql, uint64_t tl,
                                    uint64_t num_diff = 0) {  // Match::numDiff (src/coord.cpp:67): 0 for the exact overlaps
  const uint64_t len = e.length;
  uint64_t s0 = ql - len, e0 = ql - 1, s1 = 0, e1 = len - 1;
  if (e.af & 1u) { uint64_t t = s0; s0 = ql - e0 - 1; e0 = ql - t - 1; }
  if (e.af & 2u) { uint64_t t = s1; s1 = tl - e1 - 1; e1 = tl - t - 1; }
  *p++ = 'E'; *p++ = 'D'; *p++ = '\t';
  memcpy(p, qn.data(), qn.size());
  p += qn.size();
  *p++ = ' ';
  memcpy(p, tn.data(), tn.size());
  p += tn.size();
  *p++ = ' ';
  p = put_u64(p, s0); *p++ = ' ';
  p = put_u64(p, e0); *p++ = ' ';
  p = put_u64(p, ql); *p++ = ' ';
  p = put_u64(p, s1); *p++ = ' ';
  p = put_u64(p, e1); *p++ = ' ';
  p = put_u64(p, tl); *p++ = ' ';
  *p++ = (e.af & 4u) ? '1' : '0';
  *p++ = ' ';
  p = put_u64(p, num_diff);
  *p++ = '\n';
  return p;
}
static char* write_edge(char* p, const sigax_edge& e, const ReadStore& reads, const uint32_t* lengths, uint64_t num_diff) {
  return write_edge_line(p, e, reads.name(e.query), reads.name(e.target), lengths[e.query], lengths[e.target], num_diff);
}
void append_edge_line(std::string& o, const sigax_edge& e, std::string_view qn, std::string_view tn, uint64_t ql, uint64_t tl) {
  const size_t at = o.size();
  o.resize(at + qn.size() + tn.size() + kEdgeLineExtra);
  o.resize((size_t)(write_edge_line(&o[at], e, qn, tn, ql, tl) - o.data()));
}


// ED text of `cnt` edge records in chunks of ed_chunk lines, one string per chunk, on nt threads: every chunk gets room for
// the longest lines there can be (two names of max_name bytes + kEdgeLineExtra) and is written through a raw pointer.
// num_diff: the records' mismatch counts, or nullptr for 0 everywhere.
static void format_edge_text(const ReadStore& reads, const uint32_t* read_len, const sigax_edge* e, const uint32_t* num_diff, uint64_t cnt, unsigned nt,
                             uint32_t max_name, size_t ed_chunk, std::vector<std::string>* parts) {
  parts->assign((cnt + ed_chunk - 1) / ed_chunk, std::string());
  parallel_for(parts->size(), nt, [&](size_t c) {
    const uint64_t cb = c * ed_chunk, ce = std::min<uint64_t>(cnt, cb + ed_chunk);
    std::string& o = (*parts)[c];
    o.resize((ce - cb) * (2 * (size_t)max_name + kEdgeLineExtra));  // room for the longest line there can be, times the lines
    char* w = &o[0];
    // a target's name is three dependent misses away (header offset, name length, the bytes in the file image):
    // asked for sixteen and eight edges ahead
    for (uint64_t i = cb; i < ce; ++i) {
      if (i + 16 < ce) {
        const uint32_t t = e[i + 16].target;
        __builtin_prefetch(&reads.head_off[t]);
        __builtin_prefetch(&reads.name_len[t]);
        __builtin_prefetch(&read_len[t]);
      }
      if (i + 8 < ce) __builtin_prefetch(reads.file.data() + reads.head_off[e[i + 8].target]);
      w = write_edge(w, e[i], reads, read_len, num_diff ? num_diff[i] : 0);
    }
    o.resize((size_t)(w - &o[0]));
    o.shrink_to_fit();  // the text may be held until the last batch is through: not with three times its size in reserve
  });
}

// ReadInfo{name,length} of the edge converter (src/overlap_builder.cpp:333-343) as lengths + rank of each name under
// std::string operator< (equal names, equal rank).  A sample sort on the host threads: names enter as (first eight bytes,
// big endian; index) pairs -- the file image is only gone back to on a tie --, splitters from a sample cut them into
// buckets of equal names' ranges, the buckets are sorted side by side, and the ranks follow from the distinct names
// counted per bucket.  (Round 2 merged sorted runs pairwise: the last merges ran on one thread, 1.3 s for 20 M names.)
void name_ranks(const ReadStore& rs, unsigned nt, std::vector<uint32_t>* lengths, std::vector<uint32_t>* ranks) {
  const size_t n = rs.size();
  lengths->resize(n);
  ranks->resize(n);
  if (n == 0) return;
  struct Key {
    uint64_t k;
    uint32_t i;
  };
  auto less = [&](const Key& a, const Key& b) { return a.k != b.k ? a.k < b.k : rs.name(a.i) < rs.name(b.i); };
  auto same = [&](const Key& a, const Key& b) { return a.k == b.k && rs.name(a.i) == rs.name(b.i); };
  std::vector<Key> keys(n), sorted(n);
  const size_t chunks = std::max<size_t>(1, std::min<size_t>((size_t)nt * 4, n / 4096));
  const size_t step = (n + chunks - 1) / chunks;
  parallel_for(chunks, nt, [&](size_t c) {
    const size_t b = std::min(n, c * step), e = std::min(n, b + step);
    for (size_t i = b; i < e; ++i) {
      (*lengths)[i] = (uint32_t)(rs.offs[i + 1] - rs.offs[i]);
      const std::string_view nm = rs.name(i);
      uint64_t k = 0;
      for (size_t j = 0; j < 8; ++j) k = (k << 8) | (j < nm.size() ? (unsigned char)nm[j] : 0u);
      keys[i] = {k, (uint32_t)i};
    }
  });
  // splitters: every bucket takes the names in [splitter b-1, splitter b)
  const size_t nbuckets = chunks > 1 ? std::min<size_t>((size_t)nt * 8, 1024) : 1;
  std::vector<Key> splitters;
  if (nbuckets > 1) {
    const size_t nsample = std::min(n, nbuckets * 64);
    std::vector<Key> sample(nsample);
    for (size_t j = 0; j < nsample; ++j) sample[j] = keys[(size_t)((unsigned __int128)j * n / nsample)];
    std::sort(sample.begin(), sample.end(), less);
    for (size_t b = 1; b < nbuckets; ++b) splitters.push_back(sample[b * nsample / nbuckets]);
  }
  auto bucket_of = [&](const Key& x) {  // splitters <= x
    return (size_t)(std::upper_bound(splitters.begin(), splitters.end(), x, less) - splitters.begin());
  };
  std::vector<uint32_t> which(n);
  std::vector<size_t> count(chunks * nbuckets, 0);
  parallel_for(chunks, nt, [&](size_t c) {
    const size_t b = std::min(n, c * step), e = std::min(n, b + step);
    size_t* cnt = &count[c * nbuckets];
    for (size_t i = b; i < e; ++i) cnt[which[i] = (uint32_t)bucket_of(keys[i])]++;
  });
  std::vector<size_t> bstart(nbuckets + 1, 0);
  {
    size_t at = 0;  // bucket-major, chunk-minor: a chunk's share of a bucket starts at count[c][b] afterwards
    for (size_t b = 0; b < nbuckets; ++b) {
      bstart[b] = at;
      for (size_t c = 0; c < chunks; ++c) {
        const size_t k = count[c * nbuckets + b];
        count[c * nbuckets + b] = at;
        at += k;
      }
    }
    bstart[nbuckets] = at;
  }
  parallel_for(chunks, nt, [&](size_t c) {
    const size_t b = std::min(n, c * step), e = std::min(n, b + step);
    size_t* at = &count[c * nbuckets];
    for (size_t i = b; i < e; ++i) sorted[at[which[i]]++] = keys[i];
  });
  std::vector<uint32_t> distinct(nbuckets, 0);  // names of a bucket that differ from their predecessor IN the bucket
  parallel_for(nbuckets, nt, [&](size_t b) {
    Key* lo = sorted.data() + bstart[b];
    Key* hi = sorted.data() + bstart[b + 1];
    std::sort(lo, hi, less);
    uint32_t d = 0;
    for (Key* q = lo + 1; q < hi; ++q) d += same(q[-1], q[0]) ? 0u : 1u;
    distinct[b] = d;
  });
  // rank of a bucket's first name: the distinct names before it (buckets hold disjoint ranges of names)
  std::vector<uint32_t> first(nbuckets, 0);
  {
    uint32_t rk = 0;
    bool any = false;
    for (size_t b = 0; b < nbuckets; ++b) {
      if (bstart[b] == bstart[b + 1]) continue;
      if (any) ++rk;  // its first name is a new one
      first[b] = rk;
      rk += distinct[b];
      any = true;
    }
  }
  parallel_for(nbuckets, nt, [&](size_t b) {
    uint32_t rk = first[b];
    for (size_t k = bstart[b]; k < bstart[b + 1]; ++k) {
      if (k > bstart[b] && !same(sorted[k - 1], sorted[k])) ++rk;
      (*ranks)[sorted[k].i] = rk;
    }
  });
}

std::string asqg_header(size_t minOverlap) {
  // src/overlap_builder.cpp:428-437 (the IN tag is never written: :494-495)
  return "HT\tVN:i:1\tOL:i:" + std::to_string((int)minOverlap) + "\tCN:i:1\n";
}

VtAhead::VtAhead(const ReadStore* reads, unsigned nt, const std::string& header, bool gz, const HostSettings& hs)
    : _reads(*reads), _nt(std::max(1u, nt)), _header(header), _gz(gz), _level(hs.gzip_level), _n(reads->size()), _cap(hs.vt_ahead_bytes) {
  _nchunks = (_n + kChunk - 1) / kChunk;
  _text.resize(_nchunks);
  _off.assign(_nchunks + 1, 0);
  _off[0] = header.size();
  // room for the longest text there can be: "VT\t" name "\t" seq "\tSS:i:0" + the three tags (each shorter than the
  // comment it is cut from, plus its six characters) + "\n"
  uint64_t bound = header.size();
  for (size_t i = 0; i < _n; ++i) bound += 3 + 1 + 7 + 1 + 18 + 2 * (uint64_t)_reads.head_len[i] + (_reads.offs[i + 1] - _reads.offs[i]);
  if (gz) _spec.resize((size_t)(bound / OutFile::block_bytes()) + 1);
  _thread = std::thread([this] { run(); });
}

VtAhead::~VtAhead() {
  {
    std::lock_guard<std::mutex> g(_mu);
    _stop = true;
  }
  _cv.notify_all();
  if (_thread.joinable()) _thread.join();
}
// The chunks [from, to) -- formatted, their blocks deflated -- with the substring flags of their reads applied; `parts`
// takes their text.  Call with from = the previous call's to.
void VtAhead::take(size_t from, size_t to, const uint8_t* substring, std::vector<std::string>* parts) {
  {
    std::unique_lock<std::mutex> g(_mu);
    _want = to;  // (whatever the cap says: these chunks are waited for)
    _cv.notify_all();
    _cv.wait(g, [&] { return _done >= to; });
  }
  parts->clear();
  parts->resize(to - from);
  std::vector<uint8_t> again(to - from, 0);
  parallel_for(to - from, _nt, [&](size_t k) {
    const size_t c = from + k, cb = c * kChunk, ce = std::min(_n, cb + kChunk);
    bool any = false;
    for (size_t i = cb; substring && i < ce && !any; ++i) any = substring[i] != 0;
    if (any) {
      std::string o;
      o.reserve(_text[c].size());
      for (size_t i = cb; i < ce; ++i) write_vertex(o, _reads.name(i), _reads.comment(i), _reads.seq(i), substring[i] != 0);
      _text[c].swap(o);
      again[k] = 1;
    }
    (*parts)[k].swap(_text[c]);
    std::string().swap(_text[c]);
  });
  // the blocks a re-written chunk touches are the writer's to deflate
  const size_t kb = OutFile::block_bytes();
  for (size_t k = 0; _gz && k < to - from; ++k) {
    const size_t c = from + k;
    if (!again[k] || _off[c + 1] == _off[c]) continue;
    for (size_t J = (size_t)(_off[c] / kb); J <= (size_t)((_off[c + 1] - 1) / kb) && J < _spec.n; ++J) _spec.state[J].store(2);
  }
}
// the text of chunks below `to` has left: the threads may run further ahead
void VtAhead::taken(size_t to) {
  {
    std::lock_guard<std::mutex> g(_mu);
    _taken_off = _off[to];
  }
  _cv.notify_all();
}
void VtAhead::run() {
  const size_t kb = OutFile::block_bytes();
  const size_t wave = (size_t)_nt * 8;
  std::string carry = _header;   // text of the stream from `carry_off` on that is in no finished block yet
  uint64_t carry_off = 0;        // a multiple of the block size
  for (size_t c0 = 0; c0 < _nchunks; c0 += wave) {
    {
      std::unique_lock<std::mutex> g(_mu);
      _cv.wait(g, [&] { return _stop || c0 < _want || _off[c0] - _taken_off <= _cap; });
      if (_stop) return;
    }
    const size_t c1 = std::min(_nchunks, c0 + wave);
    parallel_for(c1 - c0, _nt, [&](size_t k) {
      const size_t c = c0 + k, cb = c * kChunk, ce = std::min(_n, cb + kChunk);
      std::string& o = _text[c];
      o.reserve((size_t)(_reads.offs[ce] - _reads.offs[cb]) + (ce - cb) * 32);
      for (size_t i = cb; i < ce; ++i) write_vertex(o, _reads.name(i), _reads.comment(i), _reads.seq(i), false);
    });
    for (size_t c = c0; c < c1; ++c) _off[c + 1] = _off[c] + _text[c].size();
    if (_gz) {
      // pending text = carry + the wave's chunks, from carry_off on
      std::vector<const std::string*> segs;
      std::vector<uint64_t> start;
      uint64_t total = 0;
      auto add = [&](const std::string* x) {
        if (x->empty()) return;
        segs.push_back(x);
        start.push_back(total);
        total += x->size();
      };
      add(&carry);
      for (size_t c = c0; c < c1; ++c) add(&_text[c]);
      auto gather = [&](uint64_t off, size_t len, char* dst) {
        size_t k = (size_t)(std::upper_bound(start.begin(), start.end(), off) - start.begin()) - 1;
        while (len) {
          const size_t in = (size_t)(off - start[k]), take = std::min(len, segs[k]->size() - in);
          memcpy(dst, segs[k]->data() + in, take);
          dst += take;
          off += take;
          len -= take;
          ++k;
        }
      };
      const size_t nfull = (size_t)(total / kb), J0 = (size_t)(carry_off / kb);
      parallel_for(nfull, _nt, [&](size_t i) {
        if (J0 + i >= _spec.n) return;
        const uint64_t off = (uint64_t)i * kb;
        const size_t k = (size_t)(std::upper_bound(start.begin(), start.end(), off) - start.begin()) - 1;
        if (off - start[k] + kb <= segs[k]->size()) {
          OutFile::deflate_ahead(segs[k]->data() + (off - start[k]), _level, &_spec.out[J0 + i], &_spec.crc[J0 + i]);
        } else {
          std::string tmp(kb, '\0');
          gather(off, kb, &tmp[0]);
          OutFile::deflate_ahead(tmp.data(), _level, &_spec.out[J0 + i], &_spec.crc[J0 + i]);
        }
        _spec.made(J0 + i);
      });
      std::string rest((size_t)(total - (uint64_t)nfull * kb), '\0');
      if (!rest.empty()) gather((uint64_t)nfull * kb, rest.size(), &rest[0]);
      carry.swap(rest);
      carry_off += (uint64_t)nfull * kb;
    }
    {
      std::lock_guard<std::mutex> g(_mu);
      _done = c1;
    }
    _cv.notify_all();
  }
}

AsqgWriter::AsqgWriter(OutFile& out, const ReadStore& reads, const std::vector<uint32_t>& lengths, unsigned nt, const HostSettings& hs,
                       std::unique_ptr<VtAhead> ahead, size_t ed_chunk, void (*release)(void*), size_t nbatch)
    : _out(out), _reads(reads), _read_len(lengths.data()), _nt(nt), _timing(hs.timing), _ahead(std::move(ahead)),
      _ed_hold_max(hs.ed_hold_bytes), _ed_chunk(ed_chunk), _ed_inline(hs.ed_inline), _release(release) {
  for (uint32_t l : lengths) _maxLen = std::max(_maxLen, l);
  for (uint32_t l : reads.name_len) _max_name = std::max(_max_name, l);
  if (_ahead) _sub_all.assign(reads.size(), 0);
  _num_diff.reserve(nbatch);
  _edges.reserve(nbatch);    // (the edge-text job of a batch keeps its slots while the next batch is taken)
  _ed_text.reserve(nbatch);
}

AsqgWriter::~AsqgWriter() {
  join_ed();
  for (auto& e : _edges)
    if (_release && e.first) _release((void*)e.first);
}

void AsqgWriter::format_edges(size_t k) {
  format_edge_text(_reads, _read_len, _edges[k].first, _num_diff[k], _edges[k].second, _nt, _max_name, _ed_chunk, &_ed_text[k]);
}

void AsqgWriter::add_batch(size_t lo, size_t cnt, const uint8_t* substring, const sigax_edge* edges, uint64_t n_edges, double wait_s,
                           const uint32_t* num_diff) {
  const size_t b = _edges.size(), n = _reads.size();
  PhaseTimer clock(false);
  double vt_s = 0;
  if (_ahead) {
    // every chunk of text whose reads are all back (the chunks do not know about batches)
    if (substring) memcpy(_sub_all.data() + lo, substring, cnt);
    const size_t to = lo + cnt == n ? _ahead->chunks() : (lo + cnt) / VtAhead::kChunk;
    if (to > _ahead_from) {
      std::vector<std::string> parts;
      _ahead->take(_ahead_from, to, _sub_all.data(), &parts);
      vt_s = clock.split();
      _out.write_parts(parts, _ahead->blocks());
      _ahead->taken(to);
      _ahead_from = to;
    }
  } else {
    // (the strings keep their room from batch to batch: 165 MB of fresh 4 KB pages per batch otherwise)
    std::vector<std::string>& parts = _vt_parts;
    const size_t vt_chunk = VtAhead::kChunk;
    parts.resize((cnt + vt_chunk - 1) / vt_chunk);
    parallel_for(parts.size(), _nt, [&](size_t c) {
      const size_t cb = c * vt_chunk, ce = std::min(cnt, cb + vt_chunk);
      std::string& o = parts[c];
      o.clear();
      o.reserve((ce - cb) * (_maxLen + 32));
      for (size_t i = cb; i < ce; ++i)
        write_vertex(o, _reads.name(lo + i), _reads.comment(lo + i), _reads.seq(lo + i), substring && substring[i] != 0);
    });
    vt_s = clock.split();
    _out.write_parts(parts);
  }
  if (_timing) fprintf(stderr, "[siga]   batch %zu: VT text %.3f s, deflate + write %.3f s\n", b, vt_s, clock.split());
  _edges.emplace_back(edges, n_edges);
  _num_diff.push_back(num_diff);
  _ed_text.emplace_back();
  join_ed();  // (one batch's edge text at a time; ed_held is the job's to update, ours to read after the join)
  if (_timing) fprintf(stderr, "[siga]   batch %zu: waited %.3f s for the batch, %.3f s for the ED text before it\n", b, wait_s, clock.split());
  if (_ed_held < _ed_hold_max) {
    auto job = [this, b] {
      PhaseTimer ed_clock(false);
      format_edges(b);
      if (_timing) fprintf(stderr, "[siga]   batch %zu: ED text %.3f s\n", b, ed_clock.split());
      for (const std::string& p : _ed_text[b]) _ed_held += p.size();
      if (_ed_text[b].empty()) _ed_text[b].emplace_back();  // "formatted, and nothing to say"
      if (_release) _release((void*)_edges[b].first);
      _edges[b].first = nullptr;
    };
    // beside the next batch's VT lines (SIGA_ED_INLINE=1: before them, on this thread)
    if (_ed_inline) job();
    else _ed_job = std::thread(job);
  }
}

bool AsqgWriter::finish() {
  join_ed();
  for (size_t b = 0; b < _edges.size(); ++b) {
    if (_ed_text[b].empty()) format_edges(b);
    _out.write_parts(_ed_text[b]);
    std::vector<std::string>().swap(_ed_text[b]);
  }
  for (auto& e : _edges) {
    if (_release && e.first) _release((void*)e.first);
    e.first = nullptr;
  }
  return _out.close();
}

}  // namespace sigah
