// siga_amd/host/reads.hpp -- internal: a whole reads file parsed at once (ReadStore) by the chunk-parallel loader.
#ifndef SIGA_AMD_HOST_READS_HPP_
#define SIGA_AMD_HOST_READS_HPP_

#include <sys/mman.h>

#include <cstdint>
#include <string>
#include <string_view>
#include <type_traits>
#include <vector>

#include "host_util.hpp"

namespace sigah {

// ------------------------------------------------------------------------------------------------------
// ReadStore: a whole reads file parsed at once with the reference's reader semantics (src/kseq.cpp:140-228), in
// parallel for FASTA; names and comments are spans of the file image, sequences are packed the way the device batches
// take them
// ------------------------------------------------------------------------------------------------------
// The bytes of a reads file: a plain file is mapped (its pages come in under the parsing threads: reading 3.4 GB --
// BASELINE configs[2]'s reads as FASTA -- into a vector took one thread 1.3 s before the first chunk could be parsed),
// a compressed one is expanded into memory.
struct FileImage {
  std::vector<char> owned;
  const char* map = nullptr;
  size_t map_size = 0;
  FileImage() = default;
  FileImage(const FileImage&) = delete;
  FileImage& operator=(const FileImage&) = delete;
  ~FileImage() {
    if (map) munmap((void*)map, map_size);
  }
  const char* data() const { return map ? map : owned.data(); }
  size_t size() const { return map ? map_size : owned.size(); }
};

// Memory that is written before it is read: no zero fill by us (std::vector::resize ran 3 GB of it on one thread), and for
// large blocks 2 MB pages (anonymous mapping + MADV_HUGEPAGE; the GPU boxes run transparent huge pages in `madvise` mode):
// the first touch of BASELINE configs[2]'s 3 GB of bases was 790 k page faults on the join's threads, each with its 4 KB
// cleared by the kernel -- most of the 0.31 s the join took.
struct RawBlock {
  void* p = nullptr;
  size_t bytes = 0;
  bool mapped = false;
  RawBlock() = default;
  RawBlock(const RawBlock&) = delete;
  RawBlock& operator=(const RawBlock&) = delete;
  RawBlock(RawBlock&& o) noexcept : p(o.p), bytes(o.bytes), mapped(o.mapped) { o.p = nullptr; o.bytes = 0; o.mapped = false; }
  RawBlock& operator=(RawBlock&& o) noexcept {
    if (this != &o) {
      release();
      p = o.p; bytes = o.bytes; mapped = o.mapped;
      o.p = nullptr; o.bytes = 0; o.mapped = false;
    }
    return *this;
  }
  ~RawBlock() { release(); }
  void release() {
    if (p) {
      if (mapped) munmap(p, bytes);
      else ::operator delete(p);
    }
    p = nullptr;
    bytes = 0;
    mapped = false;
  }
  void alloc(size_t want, bool huge) {  // contents undefined; huge: 2 MB pages for a large block
    release();
    if (want == 0) want = 1;
    if (want >= ((size_t)8 << 20) && huge) {
      const size_t two = (size_t)2 << 20;
      const size_t len = (want + two - 1) & ~(two - 1);
      void* q = mmap(nullptr, len, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
      if (q != MAP_FAILED) {
#ifdef MADV_HUGEPAGE
        (void)madvise(q, len, MADV_HUGEPAGE);
#endif
        p = q;
        bytes = len;
        mapped = true;
        return;
      }
    }
    p = ::operator new(want);
    bytes = want;
    mapped = false;
  }
};

struct RawChars {
  RawBlock b;
  size_t n = 0;
  void resize(size_t k, bool huge) {  // contents undefined
    b.alloc(k, huge);
    n = k;
  }
  char* data() { return (char*)b.p; }
  const char* data() const { return (const char*)b.p; }
  size_t size() const { return n; }
};

// ... and the per-read tables likewise (every entry is written by the loader's join, on its threads)
template <class T>
struct RawVec {
  static_assert(std::is_trivial<T>::value, "RawVec holds plain values");
  RawBlock b;
  size_t n = 0;
  void resize(size_t k, bool huge) {  // contents undefined
    b.alloc(k * sizeof(T), huge);
    n = k;
  }
  T* data() { return (T*)b.p; }
  const T* data() const { return (const T*)b.p; }
  size_t size() const { return n; }
  T& operator[](size_t i) { return ((T*)b.p)[i]; }
  const T& operator[](size_t i) const { return ((const T*)b.p)[i]; }
  const T* begin() const { return (const T*)b.p; }
  const T* end() const { return (const T*)b.p + n; }
};

struct ReadStore {
  FileImage file;
  RawChars seqs;
  RawVec<uint64_t> offs;                 // n + 1
  RawVec<uint64_t> head_off;             // raw header (after '>' / '@'), a span of `file`
  RawVec<uint32_t> head_len, name_len;   // name = head[0, name_len); comment = head[name_len + 1, head_len)
  RawVec<uint64_t> qual_off;             // FASTQ: span of `file`, seq length long
  bool fastq = false;
  size_t size() const { return head_off.size(); }
  std::string_view name(size_t i) const { return std::string_view(file.data() + head_off[i], name_len[i]); }
  std::string_view comment(size_t i) const {
    return name_len[i] < head_len[i] ? std::string_view(file.data() + head_off[i] + name_len[i] + 1, head_len[i] - name_len[i] - 1)
                                     : std::string_view();
  }
  std::string_view seq(size_t i) const { return std::string_view(seqs.data() + offs[i], offs[i + 1] - offs[i]); }
  std::string_view quality(size_t i) const {
    return fastq ? std::string_view(file.data() + qual_off[i], offs[i + 1] - offs[i]) : std::string_view();
  }
};

// false: the file cannot be read or is neither FASTA nor FASTQ
bool LoadReads(const std::string& path, ReadStore* rs, unsigned nt, const HostSettings& hs);

}  // namespace sigah

#endif
