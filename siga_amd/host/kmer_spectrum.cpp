// siga_amd/host/kmer_spectrum.cpp -- KmerSpectrum (`siga preqc`): the k-mer count distribution of strings drawn from the index.
#include <algorithm>
#include <random>

#include "host_util.hpp"
#include "siga_host.hpp"

namespace sigah {

// ------------------------------------------------------------------------------------------------------
// KmerSpectrum (KmerDistribution::sample, src/kmerdistr.cpp:7-36, as GenomeEstimator would call it had it an index:
// src/preqc.cpp).  The rows -- every read's once, or `samples` draws of std::mt19937_64(seed)() % n_symbols, uniform over
// all rows as Utils::rand(N) -- go to the device in batches sized from its free memory; sigax_kmer_spectrum_rows turns a
// batch into strings and strings into counts without either leaving the device, and adds to the one histogram kept here.
// ------------------------------------------------------------------------------------------------------
bool KmerSpectrum::run(const FMIndex& index, size_t batchRows) {
  _error.clear();
  sigax_index_info inf;
  if (!index.handle() || sigax_index_info_get(index.handle(), &inf) != SIGAX_OK) {
    _error = "FMIndex not loaded";
    return false;
  }
  if (_options.kmerSize == 0 || _options.kmerSize > 0xFFFFFFFFull) {
    _error = "the k-mer size must be between 1 and 2^32 - 1";
    return false;
  }
  const uint64_t n_bins = _options.maxCount + 1;  // counts 0 .. maxCount - 1, and "maxCount or more"
  _hist.assign(n_bins, 0);
  _strings = _bases = _windows = _rows = 0;
  const uint64_t total = _options.all ? inf.n_strings : _options.samples;
  if (total == 0 || inf.n_symbols == 0) return true;
  // a walk ends at its stretch's first symbol; the bound only keeps a damaged index from walking on
  const uint32_t max_len = (uint32_t)std::min<uint64_t>(inf.n_symbols, 0xFFFFFFFFull);
  uint64_t per = batchRows;
  if (per == 0) {
    const uint64_t mean = inf.n_strings ? (inf.n_symbols - inf.n_strings) / inf.n_strings : inf.n_symbols;
    if (sigax_kmer_spectrum_rows_hint(index.handle(), (uint32_t)std::min<uint64_t>(2 * mean + 16, 0xFFFFFFFFull), n_bins, &per) != SIGAX_OK) {
      _error = std::string("preqc failed: ") + sigax_last_error();
      return false;
    }
  }
  std::mt19937_64 rng(_options.seed);
  std::vector<uint64_t> rows;
  for (uint64_t base = 0; base < total; base += per) {
    const uint64_t cnt = std::min<uint64_t>(per, total - base);
    rows.resize(cnt);
    for (uint64_t i = 0; i < cnt; ++i) rows[i] = _options.all ? base + i : rng() % inf.n_symbols;
    uint64_t stat[4];
    if (sigax_kmer_spectrum_rows(index.handle(), rows.data(), cnt, (uint32_t)_options.kmerSize, max_len, n_bins, _hist.data(), stat) != SIGAX_OK) {
      _error = std::string("preqc failed: ") + sigax_last_error();
      return false;
    }
    _strings += stat[0];
    _bases += stat[1];
    _windows += stat[2];
    _rows += cnt;
  }
  return true;
}

std::string KmerSpectrum::json() const {
  std::string t = "{\"KmerDistribution\": {\"k\": ";
  append_u64(t, _options.kmerSize);
  t += _options.all ? ", \"mode\": \"all\"" : ", \"mode\": \"sample\"";
  t += ", \"samples\": ";
  append_u64(t, _rows);
  t += ", \"seed\": ";
  append_u64(t, _options.seed);
  t += ", \"strings\": ";
  append_u64(t, _strings);
  t += ", \"bases\": ";
  append_u64(t, _bases);
  t += ", \"windows\": ";
  append_u64(t, _windows);
  t += ", \"max_count\": ";
  append_u64(t, _options.maxCount);
  t += ", \"distribution\": [";
  bool first = true;
  for (size_t c = 0; c < _hist.size(); ++c) {
    if (!_hist[c]) continue;
    t += first ? "[" : ", [";
    first = false;
    append_u64(t, c);
    t += ", ";
    append_u64(t, _hist[c]);
    t += "]";
  }
  t += "]}}\n";
  return t;
}

}  // namespace sigah
