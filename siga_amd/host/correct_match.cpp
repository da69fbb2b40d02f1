// siga_amd/host/correct_match.cpp -- CorrectProcessor (`siga correct`) and Matcher (`siga match`).
#include <cstdio>

#include "host_util.hpp"
#include "out_file.hpp"
#include "reads.hpp"
#include "siga_host.hpp"

namespace sigah {

bool CorrectProcessor::process(const FMIndex& index, const std::string& input, const std::string& output, size_t threads,
                               size_t* processed) const {
  (void)threads;
  (void)processed;
  _error.clear();
  if (!index.handle()) {
    _error = "FMIndex not loaded";
    return false;
  }
  // -a overlap: the reference text once, before any file is touched, then the k-mer path's batches through the pile-up
  sigax_pile_ref* ref = nullptr;
  struct RefGuard {
    sigax_pile_ref** r;
    ~RefGuard() { sigax_pile_ref_destroy(*r); }
  } ref_guard{&ref};
  for (int k = 0; k < 8; ++k) _pileStatus[k] = 0;
  _readsIn = 0;
  _readsOut = 0;
  if (_options.overlap && sigax_pile_ref_create(index.handle(), &ref) != SIGAX_OK) {
    _error = std::string("correct failed: ") + sigax_last_error();
    return false;
  }
  DNASeqList reads;
  if (!ReadDNASequences(input, reads)) {
    _error = "Failed to create DNASeqReader " + input;
    return false;
  }
  OutFile out(output);
  if (!out.ok()) {
    _error = "Failed to create DNASeqWriter " + output;
    return false;
  }
  const size_t n = reads.size(), per = 262144;
  _readsIn = n;
  std::string seqs, quals, corrected, text;
  std::vector<uint64_t> offs;
  std::vector<uint8_t> valid, changed;
  for (size_t base = 0; base < n; base += per) {
    size_t cnt = std::min(per, n - base);
    seqs.clear();
    quals.clear();
    offs.assign(1, 0);
    bool anyQual = false;
    for (size_t i = 0; i < cnt; ++i) anyQual = anyQual || !reads[base + i].quality.empty();
    for (size_t i = 0; i < cnt; ++i) {
      const DNASeq& rd = reads[base + i];
      seqs += rd.seq;
      if (anyQual) {  // a read without qualities scores 15 per base (src/kseq.h:34-40): '0' is phred 15
        if (rd.quality.empty()) quals.append(rd.seq.size(), (char)(15 + 33));
        else quals += rd.quality;
      }
      offs.push_back(seqs.size());
    }
    corrected.assign(seqs.size(), '\0');
    valid.assign(cnt, 0);
    if (_options.overlap) {
      changed.assign(cnt, 0);
      uint64_t st[8];
      if (sigax_pileup_batch(index.handle(), ref, seqs.data(), offs.data(), cnt, &_options.pile, (uint32_t)_options.rounds, &corrected[0],
                             valid.data(), changed.data(), st, nullptr) != SIGAX_OK) {
        _error = std::string("correct failed: ") + sigax_last_error();
        return false;
      }
      for (int k = 0; k < 8; ++k) _pileStatus[k] += st[k];
    } else if (sigax_correct_batch(index.handle(), seqs.data(), anyQual ? quals.data() : nullptr, offs.data(), (uint32_t)cnt,
                            (uint32_t)_options.kmerSize, (int32_t)_options.kmerThreshold, (uint32_t)_options.kmerRounds,
                            (uint32_t)_options.kmerCountOffset, &corrected[0], valid.data()) != SIGAX_OK) {
      _error = std::string("correct failed: ") + sigax_last_error();
      return false;
    }
    text.clear();
    for (size_t i = 0; i < cnt; ++i) {  // PostCorrector (src/correct_processor.cpp:247-253) + DNASeq << (src/kseq.cpp:106-126)
      if (valid[i] != 1) continue;
      ++_readsOut;
      const DNASeq& rd = reads[base + i];
      text += rd.quality.empty() ? '>' : '@';
      text += rd.name;
      if (!rd.comment.empty()) {
        text += ' ';
        text += rd.comment;
      }
      text += '\n';
      text.append(corrected, offs[i], offs[i + 1] - offs[i]);
      text += '\n';
      if (!rd.quality.empty()) {
        text += "+\n";
        text += rd.quality;
        text += '\n';
      }
    }
    out.write(text);
  }
  if (!out.close()) {
    _error = "Failed to write " + output;
    return false;
  }
  return true;
}

// ------------------------------------------------------------------------------------------------------
// Matcher (src/match.cpp:38-63).  Two device slots (sigax_matcher): batch i's upload and kernel are queued, then batch
// i - 1's counts are waited for and its lines formatted by the host threads, piece by piece, and written in read order.
// ------------------------------------------------------------------------------------------------------
bool Matcher::run(const FMIndex& index, const std::vector<std::string>& inputs, const std::string& output, size_t threads,
                  size_t batchReads, size_t* processed) const {
  _error.clear();
  if (processed) *processed = 0;
  if (!index.handle()) {
    _error = "FMIndex not loaded";
    return false;
  }
  FILE* out = output.empty() ? stdout : fopen(output.c_str(), "wb");
  if (!out) {
    _error = "Failed to create " + output;
    return false;
  }
  const HostSettings hs;
  const unsigned nt = host_threads(threads, hs);
  sigax_matcher* m = nullptr;
  bool ok = true;
  auto fail = [&](const std::string& what) {
    if (ok) _error = what;
    ok = false;
  };
  uint64_t cap_reads = 0, cap_bases = 0;
  std::vector<std::string> pieces;
  for (size_t f = 0; f < inputs.size() && ok; ++f) {
    ReadStore rs;
    if (!LoadReads(inputs[f], &rs, nt, hs)) {
      fail("Failed to create DNASeqReader " + inputs[f]);
      break;
    }
    const size_t n = rs.size();
    if (n == 0) continue;
    for (size_t i = 0; i < n; ++i)
      if (rs.offs[i + 1] - rs.offs[i] > 0xFFFFFFFFull) fail("read too long in " + inputs[f]);
    if (!ok) break;
    if (!m) {
      // sized by the first file that has reads: batchReads reads of its mean length (the longest read must fit too)
      uint64_t maxlen = 0;
      for (size_t i = 0; i < n; ++i) maxlen = std::max<uint64_t>(maxlen, rs.offs[i + 1] - rs.offs[i]);
      const uint64_t mean = std::max<uint64_t>(1, rs.offs[n] / n);
      uint64_t want_reads = batchReads, want_bases = batchReads ? std::max<uint64_t>(batchReads * mean * 2, maxlen) : 0;
      if (sigax_matcher_create(index.handle(), 2, want_reads, want_bases, &m) != SIGAX_OK) {
        fail(std::string("match failed: ") + sigax_last_error());
        break;
      }
      sigax_matcher_capacity(m, &cap_reads, &cap_bases);
    }
    // batches: as many reads as fit a slot, by number and by bases
    std::vector<size_t> cut(1, 0);
    for (size_t b = 0; b < n;) {
      size_t e = b;
      while (e < n && e - b < cap_reads && rs.offs[e + 1] - rs.offs[b] <= cap_bases) ++e;
      if (e == b) {
        fail("a read of " + inputs[f] + " does not fit the device batch");
        break;
      }
      cut.push_back(e);
      b = e;
    }
    if (!ok) break;
    const size_t nb = cut.size() - 1;
    auto drain = [&](size_t i) {  // batch i is on its way: wait for it, format, write
      const uint64_t* counts = nullptr;
      if (sigax_matcher_wait(m, (uint32_t)(i & 1), &counts, nullptr) != SIGAX_OK) {
        fail(std::string("match failed: ") + sigax_last_error());
        return;
      }
      const size_t b = cut[i], cnt = cut[i + 1] - b, np = std::min<size_t>(std::max<size_t>(1, cnt / 4096), 4 * (size_t)nt);
      pieces.resize(np);
      parallel_for(np, nt, [&](size_t p) {
        std::string& t = pieces[p];
        t.clear();
        for (size_t k = cnt * p / np; k < cnt * (p + 1) / np; ++k) {
          const std::string_view name = rs.name(b + k), seq = rs.seq(b + k);
          for (int side = 0; side < 2; ++side) {
            const uint64_t c = counts[2 * k + side];
            if (side == 1 && c == SIGAX_MATCH_NONE) break;
            t += side ? "VT\t1\t" : "VT\t0\t";
            t.append(name.data(), name.size());
            t += '\t';
            t.append(seq.data(), seq.size());
            t += '\t';
            append_u64(t, c);
            t += '\n';
          }
        }
      });
      for (const std::string& t : pieces)
        if (!t.empty() && fwrite(t.data(), 1, t.size(), out) != t.size()) fail("Failed to write " + (output.empty() ? std::string("stdout") : output));
      if (processed) *processed += cnt;
    };
    for (size_t i = 0; i < nb && ok; ++i) {
      if (sigax_matcher_submit(m, (uint32_t)(i & 1), rs.seqs.data(), rs.offs.data() + cut[i], cut[i + 1] - cut[i], _maxLength,
                               _rc ? SIGAX_RC : 0u) != SIGAX_OK) {
        fail(std::string("match failed: ") + sigax_last_error());
        break;
      }
      if (i > 0) drain(i - 1);
    }
    if (ok) drain(nb - 1);
  }
  if (m) sigax_matcher_destroy(m);
  if (fflush(out) != 0) fail("Failed to write output");
  if (out != stdout) fclose(out);
  return ok;
}

}  // namespace sigah
