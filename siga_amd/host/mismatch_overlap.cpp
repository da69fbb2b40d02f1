// siga_amd/host/mismatch_overlap.cpp -- MismatchOverlapper (`siga overlap -e`): the reads for names and lengths, the read
// metadata into the index, the reference text once, sigax_mmoverlap_batch, and the ASQG text through the writer of
// OverlapBuilder::build.
#include <algorithm>

#include "asqg_text.hpp"
#include "host_util.hpp"
#include "out_file.hpp"
#include "reads.hpp"
#include "siga_host.hpp"

namespace sigah {

MismatchRecords::~MismatchRecords() { sigax_pile_ref_destroy(_ref); }

bool MismatchRecords::open(const FMIndex& index, std::string* error) {
  if (sigax_pile_ref_create(index.handle(), &_ref) != SIGAX_OK) {
    *error = sigax_last_error();
    return false;
  }
  return true;
}

bool MismatchRecords::find(const FMIndex& index, const sigax_mmo_params& params, size_t n, unsigned nt, std::vector<sigax_edge>* edges,
                           std::vector<uint32_t>* num_diff, std::vector<uint8_t>* contained, uint64_t status8[8], std::string* error,
                           std::vector<sigax_mm_edge>* containments) {
  sigax_mm_edge* found = nullptr;
  struct Found {
    sigax_mm_edge** p;
    ~Found() { sigax_free(*p); }
  } found_guard{&found};
  uint64_t n_found = 0;
  contained->assign(std::max<size_t>(n, 1), 0);
  sigax_mmo_params p = params;
  if (containments) p.flags |= SIGAX_MMO_CONTAINMENTS;
  if (sigax_mmoverlap_batch(index.handle(), _ref, &p, &found, &n_found, contained->data(), status8) != SIGAX_OK) {
    *error = sigax_last_error();
    return false;
  }
  if (containments) {  // the dovetails to the front, in their order; the containment records aside, in theirs
    containments->clear();
    uint64_t kept = 0;
    for (uint64_t i = 0; i < n_found; ++i) {
      if (found[i].af & SIGAX_MM_CONTAINMENT) containments->push_back(found[i]);
      else found[kept++] = found[i];
    }
    n_found = kept;
  }
  // the writer and the unitig calls take sigax_edge records; the mismatch counts go beside them
  edges->resize((size_t)n_found);
  num_diff->resize((size_t)n_found);
  parallel_for(((size_t)n_found + 65535) / 65536, nt, [&](size_t c) {
    const size_t b = c * 65536, e = std::min<size_t>((size_t)n_found, b + 65536);
    for (size_t i = b; i < e; ++i) {
      (*edges)[i].query = found[i].query;
      (*edges)[i].target = found[i].target;
      (*edges)[i].length = found[i].length;
      (*edges)[i].af = found[i].af;
      (*num_diff)[i] = found[i].num_diff;
    }
  });
  return true;
}

bool MismatchOverlapper::run(const FMIndex& index, const std::string& input, const std::string& output, size_t threads) const {
  for (int k = 0; k < 8; ++k) _status[k] = 0;
  _records = _containments = 0;
  // the reference text once, before any file is touched: an index that cannot serve is refused here
  MismatchRecords ref;
  if (!ref.open(index, &_error)) return false;
  const HostSettings hs;
  const unsigned nt = (unsigned)std::max<size_t>(threads, 1);
  ReadStore rs;
  if (!LoadReads(input, &rs, nt, hs)) {
    _error = "cannot read " + input;
    return false;
  }
  const size_t n = rs.size();
  sigax_index_info info;
  if (sigax_index_info_get(index.handle(), &info) != SIGAX_OK) {
    _error = sigax_last_error();
    return false;
  }
  if (info.n_strings != n) {
    _error = input + " holds " + std::to_string(n) + " reads, the index " + std::to_string(info.n_strings);
    return false;
  }
  std::vector<uint32_t> lengths, ranks;
  name_ranks(rs, nt, &lengths, &ranks);
  if (sigax_index_set_reads(index.handle(), lengths.data(), ranks.data(), n) != SIGAX_OK) {
    _error = sigax_last_error();
    return false;
  }
  std::vector<sigax_edge> edges;
  std::vector<uint32_t> num_diff;
  std::vector<uint8_t> contained;
  std::vector<sigax_mm_edge> conts;
  const bool want_conts = !_containments_path.empty();
  if (!ref.find(index, _params, n, nt, &edges, &num_diff, &contained, _status, &_error, want_conts ? &conts : nullptr)) return false;
  if (want_conts) {
    OutFile cf(_containments_path, nt);
    if (!cf.ok()) {
      _error = "cannot write " + _containments_path;
      return false;
    }
    std::string text;
    for (const sigax_mm_edge& c : conts) {
      text.append(rs.name(c.query)).push_back('\t');
      text.append(rs.name(c.target)).push_back('\t');
      text += std::to_string(c.reserved) + ((c.af & 4) ? "\t-\t" : "\t+\t") + std::to_string(c.num_diff) + "\n";
      if (text.size() >= (1u << 20)) {
        cf.write(text);
        text.clear();
      }
    }
    cf.write(text);
    if (!cf.close()) {
      _error = "cannot write " + _containments_path;
      return false;
    }
    _containments = conts.size();
  }
  const uint64_t n_found = edges.size();
  _records = n_found;
  OutFile out(output, nt);
  if (!out.ok()) {
    _error = "cannot write " + output;
    return false;
  }
  out.write(asqg_header((size_t)_params.min_overlap));
  AsqgWriter writer(out, rs, lengths, nt, hs, nullptr, 1000, nullptr, 1);  // (the records are this function's)
  writer.add_batch(0, n, contained.data(), edges.data(), n_found, 0, num_diff.data());
  if (!writer.finish()) {
    _error = "cannot write " + output;
    return false;
  }
  return true;
}

}  // namespace sigah
