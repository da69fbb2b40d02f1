// siga_amd/host/siga_main.cpp -- `siga index` / `siga overlap` / `siga match` / `siga locate` / `siga preqc` / `siga unitig` ... command line, option for option as the reference
// (src/main.cpp:17-83, src/indexer.cpp:119-156, src/overlap.cpp:66-105).  Exit codes follow the reference:
// a runner returning -1 exits 255; printing help returns 256, i.e. exit status 0.
#include <cerrno>
#include <getopt.h>
#include <unistd.h>

#include <chrono>
#include <thread>
#include <algorithm>
#include <cctype>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "siga_host.hpp"

extern "C" int sigah_index_file_dev(const char*, const char*, int, int, int, int, char*, uint64_t);
extern "C" int sigah_index_file_sais(const char*, const char*, int, int, int, char*, uint64_t);

// -s, --ini=FILE (src/main.cpp:62-77): boost::property_tree::read_ini fills the option tree, then the command line's options
// are put over it.  Here: the file's top-level `key=value` lines (`;` comments; keys under a [section] have dotted names no
// option carries) become "--key=value" / "--key" arguments in front of the command line's own, for the keys this
// sub-command's option table knows, so that what the command line says wins.  Returns 1 (the reference's exit status) when
// the file cannot be read or a line has no '='.
static int apply_ini(int argc, char** argv, const option* longopts, std::vector<std::string>* store, std::vector<char*>* out) {
  std::string path;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    if (a == "--") break;
    if ((a == "-s" || a == "--ini") && i + 1 < argc) path = argv[i + 1];
    else if (a.compare(0, 6, "--ini=") == 0) path = a.substr(6);
    else if (a.size() > 2 && a[0] == '-' && a[1] == 's') path = a.substr(2);
  }
  out->assign(argv, argv + argc);
  if (path.empty()) return 0;
  FILE* f = fopen(path.c_str(), "r");
  if (!f) {
    fprintf(stderr, "load %s failed(cannot open file).\n", path.c_str());
    return 1;
  }
  auto trim = [](std::string x) {
    const char* ws = " \t\r\n";
    const size_t b = x.find_first_not_of(ws);
    if (b == std::string::npos) return std::string();
    return x.substr(b, x.find_last_not_of(ws) - b + 1);
  };
  char line[4096];
  bool in_section = false;
  int rc = 0;
  while (fgets(line, sizeof(line), f)) {
    const std::string l = trim(line);
    if (l.empty() || l[0] == ';') continue;
    if (l[0] == '[') {
      in_section = true;
      continue;
    }
    const size_t eq = l.find('=');
    if (eq == std::string::npos) {
      fprintf(stderr, "load %s failed('=' character not found in line).\n", path.c_str());
      rc = 1;
      break;
    }
    if (in_section) continue;
    const std::string key = trim(l.substr(0, eq)), val = trim(l.substr(eq + 1));
    for (const option* o = longopts; o->name; ++o)
      if (key == o->name && key != "ini") store->push_back(o->has_arg == no_argument ? "--" + key : "--" + key + "=" + val);
  }
  fclose(f);
  if (rc) return rc;
  out->clear();
  out->push_back(argv[0]);
  for (std::string& x : *store) out->push_back(&x[0]);
  for (int i = 1; i < argc; ++i) out->push_back(argv[i]);
  return 0;
}

static int usage() {
  printf("siga [index|correct|overlap|rmdup|preqc|locate|unitig|match] [OPTION] ... READSFILE\n"
         "  index     build the FM-index (.sai/.bwt/.rsai/.rbwt) of READSFILE\n"
         "  overlap   compute pairwise overlaps between all the sequences in READSFILE (GPU)\n"
         "  rmdup     remove duplicated reads (GPU)\n"
         "  correct   k-mer or overlap based error correction (GPU)\n"
         "  match     count the occurrences of every read of READSFILE in the indexed reads (GPU)\n"
         "  locate    list where every sequence of QUERYFILE occurs in the indexed reads: read, offset, strand (GPU)\n"
         "  unitig    overlap READSFILE and compact every unbranched chain of overlaps into one sequence (GPU)\n"
         "  preqc     pre-assembly quality checks: the k-mer count distribution of the indexed reads (GPU)\n"
         "common options: -s, --ini=FILE (options from FILE, the command line goes over them);\n"
         "                -c, --log4cxx=FILE is accepted and ignored (this build logs to stderr; SIGA_TIMING=1 prints phase\n"
         "                times and the reference's \"processed N sequences\" progress lines)\n");
  return 256;
}

static int index_help() {
  printf("siga index [OPTION] ... READSFILE\n"
         "Index the reads in READSFILE using a suffixarray/bwt\n"
         "\n"
         "      -h, --help                       display this help and exit\n"
         "\n"
         "      -a, --algorithm=STR              BWT construction algorithm. STR can be:\n"
         "                                       sais - induced sort algorithm's suffix order (host sorter, ACGT-only reads)\n"
         "                                       sais2 - very fast and works for very long sequences (default; GPU sorter)\n"
         "      -t, --threads=NUM                use NUM threads to construct the index (default: 1)\n"
         "      -p, --prefix=PREFIX              write index to file using PREFIX instead of prefix of READSFILE\n"
         "          --no-reverse                 suppress construction of the reverse BWT\n"
         "          --no-forward                 suppress construction of the forward BWT\n"
         "          --device=NUM                 GPU that sorts the suffixes (default: 0)\n"
         "          --cpu                        sort on the host (-t threads) instead; also taken when no GPU is visible\n"
         "\n");
  return 256;
}

static int overlap_help() {
  // help text of src/overlap.cpp:66-82 (the defaults it prints differ from the code defaults 10 / 10000, :44)
  printf("siga overlap [OPTION] ... READSFILE\n"
         "Compute pairwise overlap between all the sequences in READS\n"
         "\n"
         "      -h, --help                       display this help and exit\n"
         "\n"
         "      -t, --threads=NUM                use NUM threads to construct the index (default: 1)\n"
         "          --batch-size=NUM             use NUM batches for each thread (default: 1000)\n"
         "      -m, --min-overlap=LEN            minimum overlap required between two reads (default: 45)\n"
         "      -p, --prefix=PREFIX              write index to file using PREFIX instead of prefix of READSFILE\n"
         "      -x, --exhaustive                 output all overlaps, including transitive edges\n"
         "          --no-opposite-strand         treat all reads as forward strand\n"
         "          --device=NUM                 first GPU to use (default: 0)\n"
         "          --gpus=NUM                   shard the reads over NUM GPUs of this node, index replicated on each (default: 1)\n"
         "\n"
         "Overlaps with mismatches (needs PREFIX.sai and reads of ACGT only; one GPU, both strands):\n"
         "      -e, --error-permille=N           output every overlap of at least -m columns (default with -e: 45) with at most N\n"
         "                                       mismatches per mille of its columns, 0..250, without gaps, as -x does for exact ones;\n"
         "                                       found by seeds and verified, the mismatches in the last column of the ED lines\n"
         "          --seed-length=N              length of the seeds that find the candidates, 12..64 (default: 24)\n"
         "          --seed-stride=N              distance between two seeds of a read, 1..seed length (default: 12)\n"
         "          --max-seed-hits=N            skip a seed that occurs more than N times, 1..4096 (default: 256)\n"
         "          --max-candidates=N           a read with more than N candidates reports nothing itself, 1..4096 (default: 512)\n"
         "          --containments=FILE          write one line per containment to FILE (gz when it ends with .gz): contained read,\n"
         "                                       container, first column of the container it covers, + or - (reverse-complemented\n"
         "                                       in the container), mismatches\n"
         "\n");
  return 256;
}

static int run_index(int argc, char** argv) {
  enum { OPT_NO_REVERSE = 1, OPT_NO_FORWARD, OPT_DEVICE, OPT_CPU };
  static const option longopts[] = {{"log4cxx", required_argument, nullptr, 'c'},  {"ini", required_argument, nullptr, 's'},
                                    {"prefix", required_argument, nullptr, 'p'},   {"algorithm", required_argument, nullptr, 'a'},
                                    {"threads", required_argument, nullptr, 't'},  {"no-reverse", no_argument, nullptr, OPT_NO_REVERSE},
                                    {"no-forward", no_argument, nullptr, OPT_NO_FORWARD}, {"device", required_argument, nullptr, OPT_DEVICE},
                                    {"cpu", no_argument, nullptr, OPT_CPU},        {"help", no_argument, nullptr, 'h'},
                                    {nullptr, 0, nullptr, 0}};
  std::string prefix, algorithm = "sais2";
  int threads = 1, c, device = 0;
  bool help = false, nofwd = false, norev = false, cpu = false;
  std::vector<std::string> ini_store;
  std::vector<char*> ini_argv;
  if (apply_ini(argc, argv, longopts, &ini_store, &ini_argv) != 0) return 1;
  argc = (int)ini_argv.size();
  argv = ini_argv.data();
  while ((c = getopt_long(argc, argv, "c:s:a:t:p:h", longopts, nullptr)) != -1) {
    switch (c) {
      case 'p': prefix = optarg; break;
      case 'a': algorithm = optarg; break;
      case 't': threads = atoi(optarg); break;
      case OPT_NO_REVERSE: norev = true; break;
      case OPT_NO_FORWARD: nofwd = true; break;
      case OPT_DEVICE: device = atoi(optarg); break;
      case OPT_CPU: cpu = true; break;
      case 'h': help = true; break;
      default: break;
    }
  }
  if (help || argc - optind != 1) return index_help();
  std::string input = argv[optind];
  if (prefix.empty()) prefix = sigah::Utils::stem(input);
  // src/suffix_array_builder.cpp:684-692: "sais" and "sais2" (case-insensitive); anything else fails to create a builder
  for (char& ch : algorithm) ch = (char)tolower((unsigned char)ch);
  if (algorithm == "sais") {  // SAISBuilder's order (every read's own sentinel, by read index): the host sorter only
    char err[512] = "";
    if (sigah_index_file_sais(input.c_str(), prefix.c_str(), threads, nofwd ? 0 : 1, norev ? 0 : 1, err, sizeof(err)) != 0) {
      fprintf(stderr, "%s\n", err);
      return -1;
    }
    return 0;
  }
  if (algorithm != "sais2") {
    fprintf(stderr, "Failed to create suffix array builder algorithm %s\n", algorithm.c_str());
    return -1;
  }
  if (!cpu) {
    int ndev = 0;
    if (sigax_device_count(&ndev) != SIGAX_OK || ndev <= 0) cpu = true;  // `siga index` also runs on a host without a GPU
  }
  char err[512] = "";
  if (sigah_index_file_dev(input.c_str(), prefix.c_str(), cpu ? -1 : device, threads, nofwd ? 0 : 1, norev ? 0 : 1, err, sizeof(err)) != 0) {
    fprintf(stderr, "%s\n", err);
    return -1;
  }
  return 0;
}

static int run_overlap(int argc, char** argv) {
  enum { OPT_BATCH_SIZE = 1, OPT_NO_RC, OPT_DEVICE, OPT_GPUS, OPT_SEED_LENGTH, OPT_SEED_STRIDE, OPT_MAX_SEED_HITS, OPT_MAX_CANDIDATES,
         OPT_CONTAINMENTS };
  static const option longopts[] = {{"log4cxx", required_argument, nullptr, 'c'},     {"ini", required_argument, nullptr, 's'},
                                    {"error-permille", required_argument, nullptr, 'e'}, {"seed-length", required_argument, nullptr, OPT_SEED_LENGTH},
                                    {"containments", required_argument, nullptr, OPT_CONTAINMENTS},
                                    {"seed-stride", required_argument, nullptr, OPT_SEED_STRIDE},
                                    {"max-seed-hits", required_argument, nullptr, OPT_MAX_SEED_HITS},
                                    {"max-candidates", required_argument, nullptr, OPT_MAX_CANDIDATES},
                                    {"prefix", required_argument, nullptr, 'p'},      {"threads", required_argument, nullptr, 't'},
                                    {"batch-size", required_argument, nullptr, OPT_BATCH_SIZE},
                                    {"min-overlap", required_argument, nullptr, 'm'}, {"exhaustive", no_argument, nullptr, 'x'},
                                    {"no-opposite-strand", no_argument, nullptr, OPT_NO_RC},
                                    {"device", required_argument, nullptr, OPT_DEVICE}, {"gpus", required_argument, nullptr, OPT_GPUS},
                                    {"help", no_argument, nullptr, 'h'}, {nullptr, 0, nullptr, 0}};
  std::string prefix, containments;
  size_t threads = 1, batch = 10000, minOverlap = 10;  // code defaults of src/overlap.cpp:44
  bool exhaustive = false, norc = false, help = false;
  int device = 0, gpus = 1, c;
  // -e: overlaps with mismatches (MismatchOverlapper); the seed options are its own
  sigax_mmo_params mmo = sigah::MismatchOverlapper::defaults(0);
  bool mismatches = false;
  const char* seed_option = nullptr;  // the first option on the line that only -e takes
  // a number in 0 .. 2^32 - 1, or 2^32 - 1 for anything else: the library names the field that is out of range
  auto num32 = [](const char* a) {
    char* end = nullptr;
    const unsigned long long v = strtoull(a, &end, 10);
    return (uint32_t)((*a == '-' || end == a || *end || v > 0xFFFFFFFFull) ? 0xFFFFFFFFull : v);
  };
  std::vector<std::string> ini_store;
  std::vector<char*> ini_argv;
  if (apply_ini(argc, argv, longopts, &ini_store, &ini_argv) != 0) return 1;
  argc = (int)ini_argv.size();
  argv = ini_argv.data();
  while ((c = getopt_long(argc, argv, "c:s:t:p:m:e:xh", longopts, nullptr)) != -1) {
    switch (c) {
      case 'p': prefix = optarg; break;
      case 't': threads = strtoull(optarg, nullptr, 10); break;
      case 'm': minOverlap = strtoull(optarg, nullptr, 10); mmo.min_overlap = num32(optarg); break;
      case 'e': mmo.error_permille = num32(optarg); mismatches = true; break;
      case OPT_SEED_LENGTH: mmo.seed_length = num32(optarg); if (!seed_option) seed_option = "--seed-length"; break;
      case OPT_SEED_STRIDE: mmo.seed_stride = num32(optarg); if (!seed_option) seed_option = "--seed-stride"; break;
      case OPT_MAX_SEED_HITS: mmo.max_seed_hits = num32(optarg); if (!seed_option) seed_option = "--max-seed-hits"; break;
      case OPT_MAX_CANDIDATES: mmo.max_candidates = num32(optarg); if (!seed_option) seed_option = "--max-candidates"; break;
      case OPT_CONTAINMENTS: containments = optarg; if (!seed_option) seed_option = "--containments"; break;
      case 'x': exhaustive = true; break;
      case OPT_BATCH_SIZE: batch = strtoull(optarg, nullptr, 10); break;
      case OPT_NO_RC: norc = true; break;
      case OPT_DEVICE: device = atoi(optarg); break;
      case OPT_GPUS: gpus = atoi(optarg); break;
      case 'h': help = true; break;
      default: break;
    }
  }
  if (help || argc - optind != 1) return overlap_help();
  std::string input = argv[optind];
  if (prefix.empty()) prefix = sigah::Utils::stem(input);
  if (!mismatches && seed_option) {
    fprintf(stderr, "siga overlap: option %s applies to -e/--error-permille only\n", seed_option);
    return 1;
  }
  if (mismatches) {
    if (norc || gpus > 1) {
      fprintf(stderr, "siga overlap: option %s cannot be combined with -e/--error-permille\n", norc ? "--no-opposite-strand" : "--gpus");
      return 1;
    }
    uint64_t probe = 0;
    if (sigax_mmoverlap_workspace(0, 0, &mmo, 0, &probe) != SIGAX_OK) {  // the ranges are the library's
      fprintf(stderr, "siga overlap: %s\n", sigax_last_error());
      return 1;
    }
    sigah::FMIndex fmi;
    if (!sigah::FMIndex::loadForwardSai(prefix, fmi, device)) {  // (a missing .sai file is named in the text)
      fprintf(stderr, "Failed to load FMIndex from %s: %s\n", prefix.c_str(), sigax_last_error());
      return 1;
    }
    sigah::MismatchOverlapper finder(mmo);
    finder.setContainments(containments);
    if (!finder.run(fmi, input, prefix + ".asqg.gz", threads)) {
      fprintf(stderr, "Failed to build overlaps from reads %s: %s\n", input.c_str(), finder.error().c_str());
      return 1;
    }
    const uint64_t* st = finder.status();
    fprintf(stderr, "siga overlap -e: %llu overlaps; %llu reads too short or too long, %llu over --max-candidates, %llu seeds located, "
            "%llu skipped as repeats, %llu candidates tested, %llu accepted\n",
            (unsigned long long)finder.records(), (unsigned long long)st[1], (unsigned long long)st[2], (unsigned long long)st[3],
            (unsigned long long)st[4], (unsigned long long)st[5], (unsigned long long)st[6]);
    if (!containments.empty())
      fprintf(stderr, "siga overlap -e: %llu containments to %s\n", (unsigned long long)finder.containments(), containments.c_str());
    return 0;
  }
  // (not destroyed: the process ends when this command returns, and handing tens of GB of tables back to the driver one
  // hipFree at a time was 0.2 s of a 2 s run at BASELINE configs[2])
  sigah::FMIndex& fmi = *new sigah::FMIndex;
  sigah::OverlapBuilder& builder = *new sigah::OverlapBuilder(&fmi, prefix, !exhaustive, !norc);
  builder.setGPUs(gpus);
  builder.keepReads(true);
  const auto t_load = std::chrono::steady_clock::now();
  // the index goes to the GPU while the host threads parse the reads
  bool loaded = false;
  std::string load_error;
  std::thread loader([&] {
    loaded = sigah::FMIndex::load(prefix, fmi, device);
    if (!loaded) load_error = sigax_last_error();
  });
  builder.preload(input, threads, (long)minOverlap, prefix + ".asqg.gz");
  loader.join();
  if (!loaded) {
    fprintf(stderr, "Failed to load FMIndex from %s: %s\n", input.c_str(), load_error.c_str());
    return -1;
  }
  if (getenv("SIGA_TIMING"))
    fprintf(stderr, "[siga] %-28s %8.3f s\n", "FMIndex::load || parse", std::chrono::duration<double>(std::chrono::steady_clock::now() - t_load).count());
  if (!builder.build(input, minOverlap, prefix + ".asqg.gz", threads, batch)) {
    fprintf(stderr, "Failed to build overlaps from reads %s: %s\n", input.c_str(), builder.error().c_str());
    return -1;
  }
  return 0;
}

static int rmdup_help() {
  printf("siga rmdup [OPTION] ... READSFILE\n"
         "Remove duplicated reads from the data set\n"
         "\n"
         "      -h, --help                       display this help and exit\n"
         "      -p, --prefix=PREFIX              use PREFIX instead of the prefix of the reads filename for the input/output files\n"
         "      -t, --threads=N                  use N threads (default: 1)\n"
         "          --device=NUM                 GPU to use (default: 0)\n"
         "\n");
  return 256;
}

// src/rmdup.cpp:22-49: outputs <prefix>.rmdup.fa and <prefix>.rmdup.dups.fa
static int run_rmdup(int argc, char** argv) {
  enum { OPT_DEVICE = 1 };
  static const option longopts[] = {{"log4cxx", required_argument, nullptr, 'c'}, {"ini", required_argument, nullptr, 's'},
                                    {"prefix", required_argument, nullptr, 'p'},  {"threads", required_argument, nullptr, 't'},
                                    {"sample-rate", required_argument, nullptr, 'd'}, {"device", required_argument, nullptr, OPT_DEVICE},
                                    {"help", no_argument, nullptr, 'h'}, {nullptr, 0, nullptr, 0}};
  std::string prefix;
  size_t threads = 1;
  bool help = false;
  int device = 0, c;
  std::vector<std::string> ini_store;
  std::vector<char*> ini_argv;
  if (apply_ini(argc, argv, longopts, &ini_store, &ini_argv) != 0) return 1;
  argc = (int)ini_argv.size();
  argv = ini_argv.data();
  while ((c = getopt_long(argc, argv, "c:s:t:p:d:h", longopts, nullptr)) != -1) {
    switch (c) {
      case 'p': prefix = optarg; break;
      case 't': threads = strtoull(optarg, nullptr, 10); break;
      case OPT_DEVICE: device = atoi(optarg); break;
      case 'h': help = true; break;
      default: break;
    }
  }
  if (help || argc - optind != 1) return rmdup_help();
  std::string input = argv[optind];
  if (prefix.empty()) prefix = sigah::Utils::stem(input);
  sigah::FMIndex fmi;
  if (!sigah::FMIndex::load(prefix, fmi, device)) {
    fprintf(stderr, "Failed to load FMIndex from %s: %s\n", input.c_str(), sigax_last_error());
    return -1;
  }
  sigah::OverlapBuilder builder(&fmi, prefix);
  if (!builder.rmdup(input, prefix + ".rmdup.fa", prefix + ".rmdup.dups.fa", threads)) {
    fprintf(stderr, "Failed to remove duplicates from reads %s: %s\n", input.c_str(), builder.error().c_str());
    return -1;
  }
  return 0;
}

static int correct_help() {
  printf("siga correct [OPTION] ... READSFILE\n"
         "Correct sequencing errors in all the reads in READSFILE\n"
         "\n"
         "      -h, --help                       display this help and exit\n"
         "\n"
         "      -p, --prefix=PREFIX              use PREFIX instead of prefix of READSFILE for the names of the index files\n"
         "      -o, --outfile=FILE               write the corrected reads to FILE (default READFILE.ec.fa)\n"
         "      -t, --threads=NUM                use NUM threads for the computation (default: 1)\n"
         "      -a, --algorithm=STR              specify the correction algorithm to use. STR is one of kmer, overlap. (default: kmer)\n"
         "\n"
         "      -k, --kmer-size=N                the length of the kmer to user (default: 31)\n"
         "      -x, --kmer-threshold=N           attempt to correct kmers that are seen less than N times (default: 3)\n"
         "      -i, --kmer-rounds=N              perform up to N rounds of kmer correction (default: 10)\n"
         "      -O, --kmer-count-offset=N        when correcting a kmer, require the count of the new kmer is at least +N higher than the count of the old kmer. (default: 1)\n"
         "          --device=NUM                 GPU to use (default: 0)\n"
         "\n"
         "Overlap correction parameters (-a overlap; needs PREFIX.sai and reads of ACGT only in the index; -k, -x and -O do not apply):\n"
         "      -i, --rounds=N                   perform up to N rounds of pile-up correction (default: 1)\n"
         "      -m, --min-overlap=LEN            columns a read of the pile must share with the read (default: 45)\n"
         "      -e, --error-permille=N           mismatches allowed per 1000 columns of an overlap, 0..250 (default: 40)\n"
         "          --seed-length=N              length of the seeds that find the pile, 12..64 (default: 24)\n"
         "          --seed-stride=N              distance between two seeds, 1..seed length (default: 12)\n"
         "          --max-seed-hits=N            skip a seed that occurs more than N times, 1..4096 (default: 256)\n"
         "          --conflict=N                 change a base when another has N votes and it has fewer (default: 5)\n"
         "          --min-depth=N                write a read only if every base has N votes (default: 2)\n"
         "          --max-candidates=N           leave a read with more than N reads in its pile alone, 1..4096 (default: 512)\n"
         "\n");
  return 256;
}

// src/correct.cpp:22-60
static int run_correct(int argc, char** argv) {
  enum { OPT_DEVICE = 1, OPT_SEED_LENGTH, OPT_SEED_STRIDE, OPT_MAX_SEED_HITS, OPT_CONFLICT, OPT_MIN_DEPTH, OPT_MAX_CANDIDATES };
  static const option longopts[] = {{"log4cxx", required_argument, nullptr, 'c'},   {"ini", required_argument, nullptr, 's'},
                                    {"prefix", required_argument, nullptr, 'p'},    {"outfile", required_argument, nullptr, 'o'},
                                    {"threads", required_argument, nullptr, 't'},   {"algorithm", required_argument, nullptr, 'a'},
                                    {"kmer-size", required_argument, nullptr, 'k'}, {"kmer-threshold", required_argument, nullptr, 'x'},
                                    {"kmer-rounds", required_argument, nullptr, 'i'}, {"kmer-count-offset", required_argument, nullptr, 'O'},
                                    {"rounds", required_argument, nullptr, 'i'},    {"min-overlap", required_argument, nullptr, 'm'},
                                    {"error-permille", required_argument, nullptr, 'e'}, {"seed-length", required_argument, nullptr, OPT_SEED_LENGTH},
                                    {"seed-stride", required_argument, nullptr, OPT_SEED_STRIDE},
                                    {"max-seed-hits", required_argument, nullptr, OPT_MAX_SEED_HITS},
                                    {"conflict", required_argument, nullptr, OPT_CONFLICT}, {"min-depth", required_argument, nullptr, OPT_MIN_DEPTH},
                                    {"max-candidates", required_argument, nullptr, OPT_MAX_CANDIDATES},
                                    {"device", required_argument, nullptr, OPT_DEVICE}, {"help", no_argument, nullptr, 'h'},
                                    {nullptr, 0, nullptr, 0}};
  std::string prefix, outfile, algorithm = "kmer";
  sigah::CorrectProcessor::Options o;
  size_t threads = 1;
  bool help = false, rounds_given = false;
  const char* kmer_only = nullptr;     // the first of -k, -x, -O on the line
  const char* overlap_only = nullptr;  // the first option on the line that only -a overlap takes
  int device = 0, c;
  // a number in 0 .. 2^32 - 1, or 2^32 - 1 for anything else: the library names the field that is out of range
  auto num32 = [](const char* a) {
    char* end = nullptr;
    const unsigned long long v = strtoull(a, &end, 10);
    return (uint32_t)((*a == '-' || end == a || *end || v > 0xFFFFFFFFull) ? 0xFFFFFFFFull : v);
  };
  std::vector<std::string> ini_store;
  std::vector<char*> ini_argv;
  if (apply_ini(argc, argv, longopts, &ini_store, &ini_argv) != 0) return 1;
  argc = (int)ini_argv.size();
  argv = ini_argv.data();
  while ((c = getopt_long(argc, argv, "c:s:p:o:t:a:k:x:i:O:m:e:h", longopts, nullptr)) != -1) {
    switch (c) {
      case 'p': prefix = optarg; break;
      case 'o': outfile = optarg; break;
      case 't': threads = strtoull(optarg, nullptr, 10); break;
      case 'a': algorithm = optarg; break;
      case 'k': o.kmerSize = strtoull(optarg, nullptr, 10); if (!kmer_only) kmer_only = "-k/--kmer-size"; break;
      case 'x': o.kmerThreshold = strtoull(optarg, nullptr, 10); if (!kmer_only) kmer_only = "-x/--kmer-threshold"; break;
      case 'i': o.kmerRounds = strtoull(optarg, nullptr, 10); o.rounds = num32(optarg); rounds_given = true; break;
      case 'O': o.kmerCountOffset = strtoull(optarg, nullptr, 10); if (!kmer_only) kmer_only = "-O/--kmer-count-offset"; break;
      case 'm': o.pile.min_overlap = num32(optarg); if (!overlap_only) overlap_only = "-m/--min-overlap"; break;
      case 'e': o.pile.error_permille = num32(optarg); if (!overlap_only) overlap_only = "-e/--error-permille"; break;
      case OPT_SEED_LENGTH: o.pile.seed_length = num32(optarg); if (!overlap_only) overlap_only = "--seed-length"; break;
      case OPT_SEED_STRIDE: o.pile.seed_stride = num32(optarg); if (!overlap_only) overlap_only = "--seed-stride"; break;
      case OPT_MAX_SEED_HITS: o.pile.max_seed_hits = num32(optarg); if (!overlap_only) overlap_only = "--max-seed-hits"; break;
      case OPT_CONFLICT: o.pile.conflict = num32(optarg); if (!overlap_only) overlap_only = "--conflict"; break;
      case OPT_MIN_DEPTH: o.pile.min_depth = num32(optarg); if (!overlap_only) overlap_only = "--min-depth"; break;
      case OPT_MAX_CANDIDATES: o.pile.max_candidates = num32(optarg); if (!overlap_only) overlap_only = "--max-candidates"; break;
      case OPT_DEVICE: device = atoi(optarg); break;
      case 'h': help = true; break;
      default: break;
    }
  }
  if (help || argc - optind != 1) return correct_help();
  std::string input = argv[optind];
  std::string stem = sigah::Utils::stem(input);
  if (outfile.empty()) outfile = stem + ".ec.fa";
  if (prefix.empty()) prefix = stem;
  if (algorithm != "kmer" && algorithm != "overlap") {  // AbstractCorrector::create returns NULL
    fprintf(stderr, "Failed to do error correction for reads %s: algorithm %s is not built\n", input.c_str(), algorithm.c_str());
    return -1;
  }
  if (algorithm == "kmer" && overlap_only) fprintf(stderr, "siga correct: option %s applies to -a overlap only and is ignored\n", overlap_only);
  if (algorithm == "overlap") {
    if (kmer_only) {
      fprintf(stderr, "siga correct: option %s applies to -a kmer only, not to -a overlap\n", kmer_only);
      return 1;
    }
    o.overlap = true;
    if (!rounds_given) o.rounds = 1;
    if (o.rounds < 1 || o.rounds == 0xFFFFFFFFull) {
      fprintf(stderr, "siga correct: -i/--rounds must be a number from 1\n");
      return 1;
    }
    uint64_t probe = 0;
    if (sigax_pileup_workspace(0, 0, &o.pile, 0, &probe) != SIGAX_OK) {  // the ranges are the library's
      fprintf(stderr, "siga correct: %s\n", sigax_last_error());
      return 1;
    }
    sigah::FMIndex fmi;
    if (!sigah::FMIndex::loadForwardSai(prefix, fmi, device)) {  // (a missing .sai file is named in the text)
      fprintf(stderr, "Failed to load FMIndex from %s: %s\n", prefix.c_str(), sigax_last_error());
      return 1;
    }
    sigah::CorrectProcessor proc(o);
    if (!proc.process(fmi, input, outfile, threads)) {
      fprintf(stderr, "Failed to do error correction for reads %s: %s\n", input.c_str(), proc.error().c_str());
      return 1;
    }
    const uint64_t* st = proc.pileStatus();
    fprintf(stderr, "siga correct -a overlap: %llu reads in, %llu written, %llu bases changed; %llu reads too long, %llu over --max-candidates, "
            "%llu seeds located, %llu skipped as repeats, %llu candidates tested, %llu accepted\n",
            (unsigned long long)proc.readsIn(), (unsigned long long)proc.readsOut(), (unsigned long long)st[7], (unsigned long long)st[1],
            (unsigned long long)st[2], (unsigned long long)st[3], (unsigned long long)st[4], (unsigned long long)st[5], (unsigned long long)st[6]);
    return 0;
  }
  sigah::FMIndex fmi;
  if (!sigah::FMIndex::loadForward(prefix, fmi, device)) {
    fprintf(stderr, "Failed to load FMIndex from %s: %s\n", prefix.c_str(), sigax_last_error());
    return -1;
  }
  sigah::CorrectProcessor proc(o);
  if (!proc.process(fmi, input, outfile, threads)) {
    fprintf(stderr, "Failed to do error correction for reads %s: %s\n", input.c_str(), proc.error().c_str());
    return -1;
  }
  return 0;
}

static int match_help() {
  // help text of src/match.cpp:83-94, plus the -l and -t lines it leaves out and --device
  printf("siga match [OPTION] ... READSFILE\n"
         "Match reads in READSFILE with ref\n"
         "\n"
         "      -h, --help                       display this help and exit\n"
         "\n"
         "      -p, --prefix=PREFIX              use PREFIX instead of prefix of READSFILE for the names of the index files\n"
         "      -l, --max-length=N               match the first and the last N bases of reads longer than N (default: whole reads)\n"
         "          --no-opposite-strand         treat all reads as forward strand\n"
         "      -t, --threads=NUM                accepted; the GPU does the counting\n"
         "          --device=NUM                 GPU to use (default: 0)\n"
         "\n");
  return 256;
}

// src/match.cpp:23-71
static int run_match(int argc, char** argv) {
  enum { OPT_NO_RC = 1, OPT_DEVICE };
  static const option longopts[] = {{"log4cxx", required_argument, nullptr, 'c'},  {"ini", required_argument, nullptr, 's'},
                                    {"prefix", required_argument, nullptr, 'p'},   {"threads", required_argument, nullptr, 't'},
                                    {"max-length", required_argument, nullptr, 'l'}, {"no-opposite-strand", no_argument, nullptr, OPT_NO_RC},
                                    {"device", required_argument, nullptr, OPT_DEVICE}, {"help", no_argument, nullptr, 'h'},
                                    {nullptr, 0, nullptr, 0}};
  std::string prefix;
  uint64_t maxLength = sigah::Matcher::kNoLimit;  // options.get<size_t>("max-length", -1)
  size_t threads = 1;
  bool help = false, rc = true;
  int device = 0, c;
  std::vector<std::string> ini_store;
  std::vector<char*> ini_argv;
  if (apply_ini(argc, argv, longopts, &ini_store, &ini_argv) != 0) return 1;
  argc = (int)ini_argv.size();
  argv = ini_argv.data();
  while ((c = getopt_long(argc, argv, "c:s:p:t:l:h", longopts, nullptr)) != -1) {
    switch (c) {
      case 'p': prefix = optarg; break;
      case 't': threads = strtoull(optarg, nullptr, 10); break;
      case 'l': maxLength = strtoull(optarg, nullptr, 10); break;
      case OPT_NO_RC: rc = false; break;
      case OPT_DEVICE: device = atoi(optarg); break;
      case 'h': help = true; break;
      default: break;
    }
  }
  if (help || argc - optind < 1) return match_help();
  std::vector<std::string> inputs(argv + optind, argv + argc);
  if (prefix.empty()) prefix = sigah::Utils::stem(inputs[0]);
  sigah::FMIndex fmi;
  if (!sigah::FMIndex::loadForward(prefix, fmi, device)) {
    fprintf(stderr, "Failed to load FMIndex from %s: %s\n", prefix.c_str(), sigax_last_error());
    return -1;
  }
  sigah::Matcher matcher(maxLength, rc);
  if (!matcher.run(fmi, inputs, std::string(), threads)) {
    fprintf(stderr, "Failed to match reads: %s\n", matcher.error().c_str());
    return -1;
  }
  return 0;
}

static int locate_help() {
  printf("siga locate [OPTION] ... QUERYFILE...\n"
         "List where the sequences of QUERYFILE occur in the indexed reads\n"
         "\n"
         "      -h, --help                       display this help and exit\n"
         "\n"
         "      -p, --prefix=PREFIX              use PREFIX instead of prefix of QUERYFILE for the names of the index files (.bwt, .sai)\n"
         "          --no-opposite-strand         do not look for the reverse complement of the queries\n"
         "          --max-hits=N                 list the hits of queries that occur at most N times (default: 1000)\n"
         "          --max-length=N               give up on a hit more than N bases into its read (default: no limit)\n"
         "      -t, --threads=NUM                accepted; the GPU does the searching\n"
         "          --device=NUM                 GPU to use (default: 0)\n"
         "\n"
         "Prints per query, in input order, QT <name> <query length> <occurrences> <hits listed> and then one line\n"
         "HT <name> <read> <offset> <+|-> per hit, tab-separated: <read> is the 0-based position of the read in the indexed\n"
         "set (the reads file is not opened), read[offset, offset + length) is the query (+) or its reverse complement (-).\n"
         "A query with a base outside ACGT, or with more than --max-hits occurrences, lists no hits; a hit given up on at\n"
         "--max-length prints * for <read> and <offset>.\n"
         "Needs <prefix>.sai and an index of reads that hold ACGT only: with other bases a row of the index is a piece of a\n"
         "read, and the index carries no table from pieces to reads.\n"
         "\n");
  return 256;
}

static int run_locate(int argc, char** argv) {
  enum { OPT_NO_RC = 1, OPT_DEVICE, OPT_MAX_HITS, OPT_MAX_LENGTH };
  static const option longopts[] = {{"log4cxx", required_argument, nullptr, 'c'},  {"ini", required_argument, nullptr, 's'},
                                    {"prefix", required_argument, nullptr, 'p'},   {"threads", required_argument, nullptr, 't'},
                                    {"max-hits", required_argument, nullptr, OPT_MAX_HITS}, {"max-length", required_argument, nullptr, OPT_MAX_LENGTH},
                                    {"no-opposite-strand", no_argument, nullptr, OPT_NO_RC}, {"device", required_argument, nullptr, OPT_DEVICE},
                                    {"help", no_argument, nullptr, 'h'}, {nullptr, 0, nullptr, 0}};
  std::string prefix;
  uint64_t maxHits = 1000, maxLength = sigah::Locator::kNoLimit;
  size_t threads = 1;
  bool help = false, rc = true;
  int device = 0, c;
  std::vector<std::string> ini_store;
  std::vector<char*> ini_argv;
  if (apply_ini(argc, argv, longopts, &ini_store, &ini_argv) != 0) return 1;
  argc = (int)ini_argv.size();
  argv = ini_argv.data();
  while ((c = getopt_long(argc, argv, "c:s:p:t:h", longopts, nullptr)) != -1) {
    switch (c) {
      case 'p': prefix = optarg; break;
      case 't': threads = strtoull(optarg, nullptr, 10); break;
      case OPT_MAX_HITS: maxHits = strtoull(optarg, nullptr, 10); break;
      case OPT_MAX_LENGTH: maxLength = strtoull(optarg, nullptr, 10); break;
      case OPT_NO_RC: rc = false; break;
      case OPT_DEVICE: device = atoi(optarg); break;
      case 'h': help = true; break;
      default: break;
    }
  }
  if (help || argc - optind < 1) return locate_help();
  std::vector<std::string> inputs(argv + optind, argv + argc);
  if (prefix.empty()) prefix = sigah::Utils::stem(inputs[0]);
  sigah::FMIndex fmi;
  if (!sigah::FMIndex::loadForwardSai(prefix, fmi, device)) {
    fprintf(stderr, "Failed to load FMIndex from %s: %s\n", prefix.c_str(), sigax_last_error());
    return -1;
  }
  const uint64_t top = 0xFFFFFFFFull;  // the library counts a query's listed hits, and a walk's steps, in 32 bits
  sigah::Locator locator((uint32_t)std::min(maxHits, top), (uint32_t)std::min(maxLength, top), rc);
  if (!locator.run(fmi, inputs, std::string(), threads)) {
    fprintf(stderr, "Failed to locate queries: %s\n", locator.error().c_str());
    return -1;
  }
  return 0;
}

static int unitig_help() {
  printf("siga unitig [OPTION] ... READSFILE\n"
         "Overlap the reads of READSFILE and write the unitigs: every unbranched chain of overlaps merged into one sequence\n"
         "\n"
         "      -h, --help                       display this help and exit\n"
         "\n"
         "      -m, --min-overlap=LEN            minimum overlap required between two reads (default: 45)\n"
         "      -p, --prefix=PREFIX              use PREFIX instead of prefix of READSFILE for the names of the index files\n"
         "      -o, --out=FILE                   write the unitigs to FILE (default: <prefix>.unitigs.fa)\n"
         "          --layout=FILE                also write one line per read to FILE: unitig, read name, + or -, offset\n"
         "      -e, --error-permille=P           take the overlaps with at most P mismatches per mille, found by seeds and verified as\n"
         "                                       `siga overlap -e` does, instead of the exact ones; a read contained in another is set\n"
         "                                       aside (no output shows it; with -x it goes as an island and --removed lists it; the\n"
         "                                       unitig count printed includes it), and every unitig column is then rewritten by vote\n"
         "                                       over the reads laid over it (headers gain changed=<columns>).  These records are\n"
         "                                       exhaustive: without --reduce nearly every read end is branched, as with --exhaustive.\n"
         "                                       Needs the .sai of the index and reads of ACGT only; not with --exhaustive or\n"
         "                                       --no-opposite-strand\n"
         "          --seed-length=N, --seed-stride=N, --max-seed-hits=N, --max-candidates=N\n"
         "                                       (need -e) the seeds, as in `siga overlap -e` (defaults: 24, 12, 256, 512)\n"
         "          --contained=FILE             (needs -e) write the names of the contained reads to FILE, in input order\n"
         "          --place-contained            (needs -e) place every contained read where its container lies, so that it votes,\n"
         "                                       counts in KC:i: and pairs; --layout lists it with a fifth column `contained`,\n"
         "                                       --removed no longer does, and its own unitig stays hidden\n"
         "          --consensus, --no-consensus  the vote on or off (default: on exactly with -e); without -e it changes no base and\n"
         "                                       adds changed=0 to every header\n"
         "          --consensus-min-votes=N      replace a base only by one with at least N votes (default: 1)\n"
         "          --exhaustive                 overlap exhaustively, transitive edges included (they branch: fewer merges;\n"
         "                                       see --reduce)\n"
         "          --reduce                     flag the overlaps a third read explains exactly (transitive reduction) before the\n"
         "                                       unitigs are built and, with -x, anew before every round over the reads that are left:\n"
         "                                       a flagged overlap is not there for any step, for the unitigs or for --graph\n"
         "          --reduced-edges=FILE         (needs --reduce) write one line per overlap flagged in the final graph to FILE: query\n"
         "                                       name, target name, length\n"
         "          --no-opposite-strand         treat all reads as forward strand\n"
         "      -t, --threads=NUM                host threads that parse READSFILE (default: 1)\n"
         "          --device=NUM                 GPU to use (default: 0)\n"
         "\n"
         "Trimming parameters (as `siga assemble`):\n"
         "      -x, --cut-terminal=N             cut off terminal branches (dead ends and islands) in N rounds (default: 0, none)\n"
         "      -n, --min-branch-length=LEN      remove terminal branches only if they are at most LEN bases in length (default: 150)\n"
         "      -C, --min-branch-coverage=N      ... and only if their coverage, (reads - 1) / bases, is at most (N - 1) / LEN\n"
         "          --graph=FILE                 write the graph between the unitigs to FILE as ASQG (gzip if it ends in .gz):\n"
         "                                       one VT line per unitig, one ED line per overlap that was not merged\n"
         "          --removed=FILE               write one line per removed read to FILE: read name, the round it went in\n"
         "\n"
         "Maximal overlap parameters (as `siga assemble`; they need -x: the cutting runs in its rounds, before the trimming):\n"
         "      -d, --max-overlap-delta=LEN      at a unitig that counts as unique, cut every overlap shorter by LEN or more than the\n"
         "                                       longest at the same unitig end (default: 0, none)\n"
         "          --max-overlap-carefully      ... but keep it where the unitig is among the longest seen from the overlap's other end\n"
         "      -N, --num-reads=N                the number of reads in the data set (default: the reads in READSFILE)\n"
         "      -G, --genome-size=LEN            the genome's length (required with -d)\n"
         "      -T, --uniq-threshold=X           a unitig counts as unique from this score on (default: 13.0)\n"
         "          --cut-edges=FILE             write one line per cut overlap to FILE: query name, target name, length, round\n"
         "\n"
         "Chimeric parameters (as `siga assemble`; they need -x and -G: the removal is the last step of a round):\n"
         "      -l, --min-chimeric-length=LEN    remove a unitig of at most LEN bases that bridges two branched unitig ends, one of\n"
         "                                       them at a unique unitig whose other neighbours are all longer or deeper\n"
         "                                       (default: 0, none)\n"
         "      -A, --min-chimeric-coverage=N    ... and only if its coverage, (reads - 1) / bases, is at most (N - 1) / LEN\n"
         "      -a, --max-chimeric-delta=LEN     the other neighbours must be longer by more than LEN bases (default: 0)\n"
         "          --chimeric=FILE              write one line per read removed as chimeric to FILE: read name, the round it went in\n"
         "      -T sets both thresholds; without it cutting takes 13.0 and the chimeric step 0.0\n"
         "\n"
         "Bubble parameters (they need -x: the step runs in its rounds, after the trimming and before the chimeric step):\n"
         "      -b, --max-bubble-span=LEN        of the unitigs that join the same two unitig ends and hold the same number of bases, at\n"
         "                                       most LEN, between them, keep the one with the most reads (default: 0, none)\n"
         "          --bubble-divergence=PERMILLE ... and remove another only if its bases differ from the kept one's in at most\n"
         "                                       PERMILLE per mille of those bases (default: 50)\n"
         "          --no-bubble-bases            ... whatever its bases\n"
         "          --bubbles=FILE               write one line per read removed as a bubble arm to FILE: read name, the round it went in\n"
         "                                       (with --bubble-edits: then the reads an indel step removed, with a third column `indel`)\n"
         "          --bubble-edits=E             (needs -b, at most 4096) also compare the unitigs between the same two unitig ends whose\n"
         "                                       bases between them differ in number by 1 to E, 0 to 31: remove another than the kept one\n"
         "                                       if at most E edits (substituted, inserted or deleted bases) turn its bases between the\n"
         "                                       ends into the kept one's (default: 0, none)\n"
         "          --bubble-edit-permille=M     ... and at most M per mille of the bases of the shorter of the two unitigs (default: 50)\n"
         "\n"
         "Paired-end parameters (mates by name: the last character swaps 1 and 2, A and B, f and r):\n"
         "          --pairs=FILE                 look every pair up in the unitigs and write the statistics to FILE as JSON: the counts\n"
         "                                       by class, the insert size estimate of `siga assemble --pe-mode=1`, the span histogram\n"
         "          --links=FILE                 also write one line per pair of unitig ends that pairs join to FILE:\n"
         "                                       LK, unitig, B or E, unitig, B or E, pairs, smallest span, sum of spans (needs --pairs)\n"
         "          --max-span=LEN               leave out of the links a pair whose span with the two ends abutting exceeds LEN\n"
         "                                       (default: 0, no limit)\n"
         "          --outward                    the library's pairs point away from each other (default: towards each other)\n"
         "          --pairs-bins=N               bins of the span histogram, 1 to 8192 (default: 1024); the last takes the rest\n"
         "          --pairs-shift=S              a bin is 2^S bases wide, 0 to 31 (default: 0)\n"
         "\n"
         "Scaffold parameters (they need --pairs: the scaffolds are built from its links):\n"
         "          --scaffold=FILE              join the unitigs whose ends one link joins and no other, and write the scaffolds to FILE,\n"
         "                                       N in the gaps: >scaffold-<n> unitigs=<k> gaps=<k - 1>, circular=<closing gap> for a ring\n"
         "          --scaffold-layout=FILE       also write one line per unitig to FILE: scaffold, unitig, + or -, offset, gap before it\n"
         "          --min-pairs=N                a link needs at least N pairs (default: 2)\n"
         "          --link-ratio=R               set aside a link of C pairs where C * R is at most the largest count at one of its ends\n"
         "                                       (default: 0, off)\n"
         "          --min-scaffold-unitig=LEN    leave links at unitigs of fewer than LEN bases alone (default: 0)\n"
         "          --insert-size=N              the span of a pair, from which a gap is estimated (default: the mean span of the pairs\n"
         "                                       inside a unitig, sum / n rounded down)\n"
         "          --min-gap=N                  a gap is at least N bases, also where the estimate is smaller or negative (default: 1)\n"
         "          --max-gap=N                  ... and at most N bases (default: 1000000)\n"
         "\n"
         "Gap filling parameters (they need --scaffold):\n"
         "          --gapfill                    walk from each unitig's last k-mer over the k-mers of the reads towards the next unitig's\n"
         "                                       first, and back where that walk forks or ends; a gap a walk closes gets its bases for\n"
         "                                       its N, every header gains filled=<gaps filled>, and the layout gives the new offsets\n"
         "          --gap-kmer=K                 the walks' k, 8 to 128 (default: 31)\n"
         "          --gap-min-count=N            a k-mer counts when it occurs N times in the reads, either strand (default: 3)\n"
         "          --gap-slack=N                a walk may arrive N bases before or after the gap's estimate (default: 100)\n"
         "          --gap-max-fill=N             leave gaps estimated above N bases alone (default: 10000)\n"
         "          --gaps=FILE                  also write one line per gap to FILE: GP, scaffold, the two unitigs, the bases laid, the\n"
         "                                       gap's class, the two walks' outcomes, + or - for the walk that filled it, the fill, the\n"
         "                                       offset at which the gap starts; with --join-overlaps the offsets are still those of\n"
         "                                       the gap filling, before any join\n"
         "\n"
         "Overlap joining parameters (they need --scaffold):\n"
         "          --join-overlaps              after the scaffolds are laid, and after --gapfill if given: where the last v bases of a\n"
         "                                       unitig are the first v of the next for exactly one v, and the reads support the sequence\n"
         "                                       across the junction, drop the N between them and one copy of the overlap; every header\n"
         "                                       gains joined=<gaps joined>, and the layout's gap before becomes signed, -v for a joined pair\n"
         "          --join-min-overlap=N         the shortest overlap looked for, 8 to 4096 (default: 16)\n"
         "          --join-max-overlap=N         the longest, up to 4096 (default: 1000)\n"
         "          --join-slack=N               leave gaps of more than N bases alone (default: 100)\n"
         "          --join-kmer=K                the k of the support test, 8 to 128 (default: 31)\n"
         "          --join-min-count=N           every k-mer across a junction must occur N times in the reads, either strand (default: 3)\n"
         "          --joins=FILE                 also write one line per gap to FILE: JN, scaffold, the two unitigs, the bases laid, the\n"
         "                                       gap's class, the overlap, the overlaps that matched, the junction k-mers looked up, the\n"
         "                                       offset at which the right unitig or the gap now starts; with --join-mismatches also the\n"
         "                                       differing bases and how many of them were taken from the right unitig\n"
         "          --join-mismatches=N          (needs --join-overlaps) where no overlap matches exactly, take the one v whose two copies\n"
         "                                       differ in at most N bases, 0 to 16, and in at most --join-mismatch-permille of v; at each\n"
         "                                       such base the copy whose k-mer the reads hold more often is written, and every k-mer that\n"
         "                                       touches the overlap must then occur --join-min-count times; every header gains\n"
         "                                       corrected=<bases taken from the right unitig> (default: 0, exact overlaps only)\n"
         "          --join-mismatch-permille=M   (needs --join-overlaps) at most v * M / 1000 differing bases, 1 to 250 (default: 50)\n"
         "\n"
         "The first step of `siga assemble` (the graph's simplify()) without the ASQG file in between: the overlap stages leave\n"
         "their edge records, and reads joined by an overlap that is the only one at both read ends it touches are merged.\n"
         "Headers: >unitig-<n> KC:i:<reads> (the tag only for more than one read), circular=<closing overlap> for a ring.\n"
         "\n");
  return 256;
}

// the numeric argument of a trimming option: digits only, at most `most` (`-x` was once --exhaustive's short form and took no
// argument: `siga unitig -x reads.fa` must not read the file name as a number)
static bool unitig_number(const char* arg, const char* option, unsigned long long most, size_t* out) {
  char* end = nullptr;
  errno = 0;
  const unsigned long long v = strtoull(arg, &end, 10);
  if (arg[0] < '0' || arg[0] > '9' || *end != '\0' || errno != 0 || v > most) {
    fprintf(stderr, "siga unitig: %s needs a number from 0 to %llu, got '%s'\n", option, most, arg);
    return false;
  }
  *out = (size_t)v;
  return true;
}

static int run_unitig(int argc, char** argv) {
  enum { OPT_NO_RC = 1, OPT_DEVICE, OPT_LAYOUT, OPT_EXHAUSTIVE, OPT_GRAPH, OPT_REMOVED, OPT_CAREFULLY, OPT_CUT_EDGES, OPT_CHIMERIC, OPT_PAIRS, OPT_LINKS,
         OPT_MAX_SPAN, OPT_OUTWARD, OPT_PAIRS_BINS, OPT_PAIRS_SHIFT, OPT_SCAFFOLD, OPT_SCAFFOLD_LAYOUT, OPT_MIN_PAIRS, OPT_LINK_RATIO,
         OPT_MIN_SCAFFOLD_UNITIG, OPT_INSERT_SIZE, OPT_MIN_GAP, OPT_MAX_GAP, OPT_BUBBLE_DIVERGENCE, OPT_NO_BUBBLE_BASES, OPT_BUBBLES,
         OPT_GAPFILL, OPT_GAP_KMER, OPT_GAP_MIN_COUNT, OPT_GAP_SLACK, OPT_GAP_MAX_FILL, OPT_GAPS,
         OPT_JOIN, OPT_JOIN_MIN_OVERLAP, OPT_JOIN_MAX_OVERLAP, OPT_JOIN_SLACK, OPT_JOIN_KMER, OPT_JOIN_MIN_COUNT, OPT_JOINS,
         OPT_JOIN_MISMATCHES, OPT_JOIN_MISMATCH_PERMILLE, OPT_BUBBLE_EDITS, OPT_BUBBLE_EDIT_PERMILLE, OPT_REDUCE, OPT_REDUCED_EDGES,
         OPT_SEED_LENGTH, OPT_SEED_STRIDE, OPT_MAX_SEED_HITS, OPT_MAX_CANDIDATES, OPT_CONSENSUS, OPT_NO_CONSENSUS, OPT_CONSENSUS_MIN_VOTES, OPT_CONTAINED,
         OPT_PLACE_CONTAINED };
  static const option longopts[] = {{"log4cxx", required_argument, nullptr, 'c'},     {"ini", required_argument, nullptr, 's'},
                                    {"prefix", required_argument, nullptr, 'p'},      {"threads", required_argument, nullptr, 't'},
                                    {"min-overlap", required_argument, nullptr, 'm'}, {"exhaustive", no_argument, nullptr, OPT_EXHAUSTIVE},
                                    {"out", required_argument, nullptr, 'o'},         {"layout", required_argument, nullptr, OPT_LAYOUT},
                                    {"cut-terminal", required_argument, nullptr, 'x'}, {"min-branch-length", required_argument, nullptr, 'n'},
                                    {"min-branch-coverage", required_argument, nullptr, 'C'}, {"graph", required_argument, nullptr, OPT_GRAPH},
                                    {"removed", required_argument, nullptr, OPT_REMOVED},
                                    {"max-overlap-delta", required_argument, nullptr, 'd'}, {"max-overlap-carefully", no_argument, nullptr, OPT_CAREFULLY},
                                    {"num-reads", required_argument, nullptr, 'N'},   {"genome-size", required_argument, nullptr, 'G'},
                                    {"uniq-threshold", required_argument, nullptr, 'T'}, {"cut-edges", required_argument, nullptr, OPT_CUT_EDGES},
                                    {"min-chimeric-length", required_argument, nullptr, 'l'},
                                    {"min-chimeric-coverage", required_argument, nullptr, 'A'},
                                    {"max-chimeric-delta", required_argument, nullptr, 'a'}, {"chimeric", required_argument, nullptr, OPT_CHIMERIC},
                                    {"max-bubble-span", required_argument, nullptr, 'b'},
                                    {"bubble-divergence", required_argument, nullptr, OPT_BUBBLE_DIVERGENCE},
                                    {"no-bubble-bases", no_argument, nullptr, OPT_NO_BUBBLE_BASES}, {"bubbles", required_argument, nullptr, OPT_BUBBLES},
                                    {"bubble-edits", required_argument, nullptr, OPT_BUBBLE_EDITS},
                                    {"bubble-edit-permille", required_argument, nullptr, OPT_BUBBLE_EDIT_PERMILLE},
                                    {"reduce", no_argument, nullptr, OPT_REDUCE}, {"reduced-edges", required_argument, nullptr, OPT_REDUCED_EDGES},
                                    {"pairs", required_argument, nullptr, OPT_PAIRS}, {"links", required_argument, nullptr, OPT_LINKS},
                                    {"max-span", required_argument, nullptr, OPT_MAX_SPAN}, {"outward", no_argument, nullptr, OPT_OUTWARD},
                                    {"pairs-bins", required_argument, nullptr, OPT_PAIRS_BINS},
                                    {"pairs-shift", required_argument, nullptr, OPT_PAIRS_SHIFT},
                                    {"scaffold", required_argument, nullptr, OPT_SCAFFOLD},
                                    {"scaffold-layout", required_argument, nullptr, OPT_SCAFFOLD_LAYOUT},
                                    {"min-pairs", required_argument, nullptr, OPT_MIN_PAIRS}, {"link-ratio", required_argument, nullptr, OPT_LINK_RATIO},
                                    {"min-scaffold-unitig", required_argument, nullptr, OPT_MIN_SCAFFOLD_UNITIG},
                                    {"insert-size", required_argument, nullptr, OPT_INSERT_SIZE},
                                    {"min-gap", required_argument, nullptr, OPT_MIN_GAP}, {"max-gap", required_argument, nullptr, OPT_MAX_GAP},
                                    {"gapfill", no_argument, nullptr, OPT_GAPFILL}, {"gap-kmer", required_argument, nullptr, OPT_GAP_KMER},
                                    {"gap-min-count", required_argument, nullptr, OPT_GAP_MIN_COUNT},
                                    {"gap-slack", required_argument, nullptr, OPT_GAP_SLACK},
                                    {"gap-max-fill", required_argument, nullptr, OPT_GAP_MAX_FILL}, {"gaps", required_argument, nullptr, OPT_GAPS},
                                    {"join-overlaps", no_argument, nullptr, OPT_JOIN}, {"join-min-overlap", required_argument, nullptr, OPT_JOIN_MIN_OVERLAP},
                                    {"join-max-overlap", required_argument, nullptr, OPT_JOIN_MAX_OVERLAP},
                                    {"join-slack", required_argument, nullptr, OPT_JOIN_SLACK}, {"join-kmer", required_argument, nullptr, OPT_JOIN_KMER},
                                    {"join-min-count", required_argument, nullptr, OPT_JOIN_MIN_COUNT}, {"joins", required_argument, nullptr, OPT_JOINS},
                                    {"join-mismatches", required_argument, nullptr, OPT_JOIN_MISMATCHES},
                                    {"join-mismatch-permille", required_argument, nullptr, OPT_JOIN_MISMATCH_PERMILLE},
                                    {"error-permille", required_argument, nullptr, 'e'}, {"seed-length", required_argument, nullptr, OPT_SEED_LENGTH},
                                    {"seed-stride", required_argument, nullptr, OPT_SEED_STRIDE},
                                    {"max-seed-hits", required_argument, nullptr, OPT_MAX_SEED_HITS},
                                    {"max-candidates", required_argument, nullptr, OPT_MAX_CANDIDATES},
                                    {"consensus", no_argument, nullptr, OPT_CONSENSUS}, {"no-consensus", no_argument, nullptr, OPT_NO_CONSENSUS},
                                    {"consensus-min-votes", required_argument, nullptr, OPT_CONSENSUS_MIN_VOTES},
                                    {"contained", required_argument, nullptr, OPT_CONTAINED},
                                    {"place-contained", no_argument, nullptr, OPT_PLACE_CONTAINED},
                                    {"no-opposite-strand", no_argument, nullptr, OPT_NO_RC}, {"device", required_argument, nullptr, OPT_DEVICE},
                                    {"help", no_argument, nullptr, 'h'}, {nullptr, 0, nullptr, 0}};
  std::string prefix, out, layout, graph, removed, cutEdges, chimericOut, pairsOut, linksOut, reducedEdges;
  // -e: mismatch overlaps in (the seed options are its own, as in `siga overlap -e`), consensus bases out
  sigax_mmo_params mmo = sigah::MismatchOverlapper::defaults(0);
  bool mismatches = false, votesTuned = false;
  int consensus = -1;  // -1: on exactly when -e is given
  size_t minVotes = 1;
  std::string containedOut;
  bool placeContained = false;
  const char* seed_option = nullptr;  // the first option on the line that only -e takes
  auto num32 = [](const char* a) {  // a number in 0 .. 2^32 - 1, or 2^32 - 1 for anything else: the library names the field out of range
    char* end = nullptr;
    const unsigned long long v = strtoull(a, &end, 10);
    return (uint32_t)((*a == '-' || end == a || *end || v > 0xFFFFFFFFull) ? 0xFFFFFFFFull : v);
  };
  bool reduce = false;
  size_t maxSpan = 0, pairsBins = 1024, pairsShift = 0;
  bool outward = false, pairsTuned = false;
  std::string scaffoldOut, scaffoldLayout;
  size_t minPairs = 2, linkRatio = 0, minScaffoldUnitig = 0, insertSize = 0, minGap = 1, maxGap = 1000000;
  bool haveInsertSize = false, scaffoldTuned = false;
  bool gapfill = false, gapTuned = false;
  size_t gapKmer = 31, gapMinCount = 3, gapSlack = 100, gapMaxFill = 10000;
  std::string gapsOut;
  bool joinOverlaps = false, joinTuned = false;
  size_t joinMinOverlap = 16, joinMaxOverlap = 1000, joinSlack = 100, joinKmer = 31, joinMinCount = 3, joinMismatches = 0, joinMismatchPermille = 50;
  std::string joinsOut;
  size_t threads = 1, minOverlap = 45, cutTerminal = 0, minBranchLength = 150, delta = 0, numReads = 0, genomeSize = 0;
  size_t chimLength = 0, chimDelta = 0;
  size_t bubbleSpan = 0, bubbleDivergence = 50;
  bool noBubbleBases = false, bubbleTuned = false;
  size_t bubbleEdits = 0, bubbleEditPermille = 50;
  bool editsTuned = false;
  std::string bubblesOut;
  long minBranchCoverage = -1, chimCoverage = -1;
  double uniqThreshold = 13.0, chimThreshold = 0.0;  // (-T sets both: src/assembler.cpp:55-67)
  bool exhaustive = false, norc = false, help = false, carefully = false;
  int device = 0, c;
  std::vector<std::string> ini_store;
  std::vector<char*> ini_argv;
  if (apply_ini(argc, argv, longopts, &ini_store, &ini_argv) != 0) return 1;
  argc = (int)ini_argv.size();
  argv = ini_argv.data();
  while ((c = getopt_long(argc, argv, "c:s:t:p:m:o:x:n:C:d:N:G:T:l:A:a:b:e:h", longopts, nullptr)) != -1) {
    switch (c) {
      case 'e': mmo.error_permille = num32(optarg); mismatches = true; break;
      case OPT_SEED_LENGTH: mmo.seed_length = num32(optarg); if (!seed_option) seed_option = "--seed-length"; break;
      case OPT_SEED_STRIDE: mmo.seed_stride = num32(optarg); if (!seed_option) seed_option = "--seed-stride"; break;
      case OPT_MAX_SEED_HITS: mmo.max_seed_hits = num32(optarg); if (!seed_option) seed_option = "--max-seed-hits"; break;
      case OPT_MAX_CANDIDATES: mmo.max_candidates = num32(optarg); if (!seed_option) seed_option = "--max-candidates"; break;
      case OPT_CONTAINED: containedOut = optarg; if (!seed_option) seed_option = "--contained"; break;
      case OPT_PLACE_CONTAINED: placeContained = true; if (!seed_option) seed_option = "--place-contained"; break;
      case OPT_CONSENSUS: consensus = 1; break;
      case OPT_NO_CONSENSUS: consensus = 0; break;
      case OPT_CONSENSUS_MIN_VOTES:
        if (!unitig_number(optarg, "--consensus-min-votes", 0xFFFFFFFFull, &minVotes)) return 1;
        if (minVotes == 0) {
          fprintf(stderr, "siga unitig: --consensus-min-votes needs a number from 1 to 4294967295, got '0'\n");
          return 1;
        }
        votesTuned = true;
        break;
      case 'p': prefix = optarg; break;
      case 't': threads = strtoull(optarg, nullptr, 10); break;
      case 'm': minOverlap = strtoull(optarg, nullptr, 10); break;
      case 'o': out = optarg; break;
      case 'x': if (!unitig_number(optarg, "-x, --cut-terminal", 64, &cutTerminal)) return 1; break;
      case 'n': if (!unitig_number(optarg, "-n, --min-branch-length", 0xFFFFFFFFull, &minBranchLength)) return 1; break;
      case 'C': {
        size_t v = 0;
        if (!unitig_number(optarg, "-C, --min-branch-coverage", 0xFFFFFFFEull, &v)) return 1;
        minBranchCoverage = (long)v;
        break;
      }
      case 'd': if (!unitig_number(optarg, "-d, --max-overlap-delta", 0xFFFFFFFFull, &delta)) return 1; break;
      case 'N': if (!unitig_number(optarg, "-N, --num-reads", ~0ull, &numReads)) return 1; break;
      case 'G': if (!unitig_number(optarg, "-G, --genome-size", ~0ull, &genomeSize)) return 1; break;
      case 'T': {
        char* end = nullptr;
        uniqThreshold = strtod(optarg, &end);
        if (end == optarg || *end != '\0') {
          fprintf(stderr, "siga unitig: -T, --uniq-threshold needs a number, got '%s'\n", optarg);
          return 1;
        }
        chimThreshold = uniqThreshold;
        break;
      }
      case 'l': if (!unitig_number(optarg, "-l, --min-chimeric-length", 0xFFFFFFFFull, &chimLength)) return 1; break;
      case 'a': if (!unitig_number(optarg, "-a, --max-chimeric-delta", 0xFFFFFFFFull, &chimDelta)) return 1; break;
      case 'A': {
        size_t v = 0;
        if (!unitig_number(optarg, "-A, --min-chimeric-coverage", 0xFFFFFFFEull, &v)) return 1;
        chimCoverage = (long)v;
        break;
      }
      case OPT_CHIMERIC: chimericOut = optarg; break;
      case 'b': if (!unitig_number(optarg, "-b, --max-bubble-span", 0xFFFFFFFFull, &bubbleSpan)) return 1; break;
      case OPT_BUBBLE_DIVERGENCE: if (!unitig_number(optarg, "--bubble-divergence", 0xFFFFFFFEull, &bubbleDivergence)) return 1; bubbleTuned = true; break;
      case OPT_NO_BUBBLE_BASES: noBubbleBases = bubbleTuned = true; break;
      case OPT_BUBBLES: bubblesOut = optarg; break;
      case OPT_BUBBLE_EDITS: if (!unitig_number(optarg, "--bubble-edits", 31, &bubbleEdits)) return 1; break;
      case OPT_BUBBLE_EDIT_PERMILLE: if (!unitig_number(optarg, "--bubble-edit-permille", 0xFFFFFFFFull, &bubbleEditPermille)) return 1; editsTuned = true; break;
      case OPT_PAIRS: pairsOut = optarg; break;
      case OPT_LINKS: linksOut = optarg; break;
      case OPT_MAX_SPAN: if (!unitig_number(optarg, "--max-span", ~0ull, &maxSpan)) return 1; pairsTuned = true; break;
      case OPT_OUTWARD: outward = pairsTuned = true; break;
      case OPT_PAIRS_BINS: if (!unitig_number(optarg, "--pairs-bins", 8192, &pairsBins) || pairsBins == 0) return 1; pairsTuned = true; break;
      case OPT_PAIRS_SHIFT: if (!unitig_number(optarg, "--pairs-shift", 31, &pairsShift)) return 1; pairsTuned = true; break;
      case OPT_SCAFFOLD: scaffoldOut = optarg; break;
      case OPT_SCAFFOLD_LAYOUT: scaffoldLayout = optarg; scaffoldTuned = true; break;
      case OPT_MIN_PAIRS: if (!unitig_number(optarg, "--min-pairs", 0xFFFFFFFFull, &minPairs)) return 1; scaffoldTuned = true; break;
      case OPT_LINK_RATIO: if (!unitig_number(optarg, "--link-ratio", 0xFFFFFFFFull, &linkRatio)) return 1; scaffoldTuned = true; break;
      case OPT_MIN_SCAFFOLD_UNITIG: if (!unitig_number(optarg, "--min-scaffold-unitig", 0xFFFFFFFFull, &minScaffoldUnitig)) return 1; scaffoldTuned = true; break;
      case OPT_INSERT_SIZE: if (!unitig_number(optarg, "--insert-size", (1ull << 62) - 1, &insertSize)) return 1; haveInsertSize = scaffoldTuned = true; break;
      case OPT_MIN_GAP: if (!unitig_number(optarg, "--min-gap", 0x7FFFFFFFull, &minGap) || minGap == 0) return 1; scaffoldTuned = true; break;
      case OPT_MAX_GAP: if (!unitig_number(optarg, "--max-gap", 0x7FFFFFFFull, &maxGap)) return 1; scaffoldTuned = true; break;
      case OPT_GAPFILL: gapfill = true; break;
      case OPT_GAP_KMER: if (!unitig_number(optarg, "--gap-kmer", 128, &gapKmer) || gapKmer < 8) return 1; gapTuned = true; break;
      case OPT_GAP_MIN_COUNT: if (!unitig_number(optarg, "--gap-min-count", 0xFFFFFFFFull, &gapMinCount) || gapMinCount == 0) return 1; gapTuned = true; break;
      case OPT_GAP_SLACK: if (!unitig_number(optarg, "--gap-slack", 0x7FFFFFFFull, &gapSlack)) return 1; gapTuned = true; break;
      case OPT_GAP_MAX_FILL: if (!unitig_number(optarg, "--gap-max-fill", 0x7FFFFFFFull, &gapMaxFill)) return 1; gapTuned = true; break;
      case OPT_GAPS: gapsOut = optarg; gapTuned = true; break;
      case OPT_JOIN: joinOverlaps = true; break;
      case OPT_JOIN_MIN_OVERLAP: if (!unitig_number(optarg, "--join-min-overlap", 4096, &joinMinOverlap) || joinMinOverlap < 8) return 1; joinTuned = true; break;
      case OPT_JOIN_MAX_OVERLAP: if (!unitig_number(optarg, "--join-max-overlap", 4096, &joinMaxOverlap) || joinMaxOverlap < 8) return 1; joinTuned = true; break;
      case OPT_JOIN_SLACK: if (!unitig_number(optarg, "--join-slack", 0x7FFFFFFFull, &joinSlack)) return 1; joinTuned = true; break;
      case OPT_JOIN_KMER: if (!unitig_number(optarg, "--join-kmer", 128, &joinKmer) || joinKmer < 8) return 1; joinTuned = true; break;
      case OPT_JOIN_MIN_COUNT: if (!unitig_number(optarg, "--join-min-count", 0xFFFFFFFFull, &joinMinCount) || joinMinCount == 0) return 1; joinTuned = true; break;
      case OPT_JOINS: joinsOut = optarg; joinTuned = true; break;
      case OPT_JOIN_MISMATCHES: if (!unitig_number(optarg, "--join-mismatches", 16, &joinMismatches)) return 1; joinTuned = true; break;
      case OPT_JOIN_MISMATCH_PERMILLE:
        if (!unitig_number(optarg, "--join-mismatch-permille", 250, &joinMismatchPermille) || joinMismatchPermille < 1) return 1;
        joinTuned = true;
        break;
      case OPT_CAREFULLY: carefully = true; break;
      case OPT_CUT_EDGES: cutEdges = optarg; break;
      case OPT_REDUCE: reduce = true; break;
      case OPT_REDUCED_EDGES: reducedEdges = optarg; break;
      case OPT_EXHAUSTIVE: exhaustive = true; break;
      case OPT_GRAPH: graph = optarg; break;
      case OPT_REMOVED: removed = optarg; break;
      case OPT_LAYOUT: layout = optarg; break;
      case OPT_NO_RC: norc = true; break;
      case OPT_DEVICE: device = atoi(optarg); break;
      case 'h': help = true; break;
      default: break;
    }
  }
  if (help || argc - optind != 1) return unitig_help();
  if (!mismatches && seed_option) {
    fprintf(stderr, "siga unitig: option %s applies to -e/--error-permille only\n", seed_option);
    return 1;
  }
  if (mismatches && (exhaustive || norc)) {
    fprintf(stderr, "siga unitig: option %s cannot be combined with -e/--error-permille\n", exhaustive ? "--exhaustive" : "--no-opposite-strand");
    return 1;
  }
  const bool vote = consensus < 0 ? mismatches : consensus != 0;
  if (votesTuned && !vote) {
    fprintf(stderr, "siga unitig: --consensus-min-votes needs --consensus or -e/--error-permille\n");
    return 1;
  }
  if (mismatches) {
    mmo.min_overlap = (uint32_t)std::min<size_t>(minOverlap, 0xFFFFFFFFull);
    uint64_t probe = 0;
    if (sigax_mmoverlap_workspace(0, 0, &mmo, 0, &probe) != SIGAX_OK) {  // the ranges are the library's
      fprintf(stderr, "siga unitig: %s\n", sigax_last_error());
      return 1;
    }
  }
  if (delta > 0 && cutTerminal == 0) {
    fprintf(stderr, "siga unitig: -d, --max-overlap-delta needs -x, --cut-terminal: the cutting runs in its rounds\n");
    return 1;
  }
  if (delta > 0 && genomeSize == 0) {
    fprintf(stderr, "siga unitig: -d, --max-overlap-delta needs -G, --genome-size\n");
    return 1;
  }
  if (!reduce && !reducedEdges.empty()) {
    fprintf(stderr, "siga unitig: --reduced-edges needs --reduce\n");
    return 1;
  }
  if (delta == 0 && (carefully || !cutEdges.empty())) {
    fprintf(stderr, "siga unitig: --max-overlap-carefully and --cut-edges need -d, --max-overlap-delta\n");
    return 1;
  }
  if (chimLength > 0 && cutTerminal == 0) {
    fprintf(stderr, "siga unitig: -l, --min-chimeric-length needs -x, --cut-terminal: the removal runs in its rounds\n");
    return 1;
  }
  if (chimLength > 0 && genomeSize == 0) {
    fprintf(stderr, "siga unitig: -l, --min-chimeric-length needs -G, --genome-size\n");
    return 1;
  }
  if (chimLength == 0 && (chimCoverage >= 0 || chimDelta > 0 || !chimericOut.empty())) {
    fprintf(stderr, "siga unitig: -A, -a and --chimeric need -l, --min-chimeric-length\n");
    return 1;
  }
  if (bubbleSpan > 0 && cutTerminal == 0) {
    fprintf(stderr, "siga unitig: -b, --max-bubble-span needs -x, --cut-terminal: the step runs in its rounds\n");
    return 1;
  }
  if (bubbleSpan == 0 && (bubbleTuned || !bubblesOut.empty())) {
    fprintf(stderr, "siga unitig: --bubble-divergence, --no-bubble-bases and --bubbles need -b, --max-bubble-span\n");
    return 1;
  }
  if (bubbleEdits > 0 && (bubbleSpan == 0 || bubbleSpan > 4096)) {
    fprintf(stderr, "siga unitig: --bubble-edits needs -b, --max-bubble-span from 1 to 4096\n");
    return 1;
  }
  if (bubbleEdits == 0 && editsTuned) {
    fprintf(stderr, "siga unitig: --bubble-edit-permille needs --bubble-edits\n");
    return 1;
  }
  if (pairsOut.empty() && (!linksOut.empty() || pairsTuned)) {
    fprintf(stderr, "siga unitig: --links, --max-span, --outward, --pairs-bins and --pairs-shift need --pairs\n");
    return 1;
  }
  if (scaffoldOut.empty() && scaffoldTuned) {
    fprintf(stderr, "siga unitig: --scaffold-layout, --min-pairs, --link-ratio, --min-scaffold-unitig, --insert-size, --min-gap and --max-gap need --scaffold\n");
    return 1;
  }
  if (!scaffoldOut.empty() && pairsOut.empty()) {
    fprintf(stderr, "siga unitig: --scaffold needs --pairs: the scaffolds are built from its links\n");
    return 1;
  }
  if (!gapfill && gapTuned) {
    fprintf(stderr, "siga unitig: --gap-kmer, --gap-min-count, --gap-slack, --gap-max-fill and --gaps need --gapfill\n");
    return 1;
  }
  if (gapfill && scaffoldOut.empty()) {
    fprintf(stderr, "siga unitig: --gapfill needs --scaffold: it fills the gaps of the scaffolds\n");
    return 1;
  }
  if (!joinOverlaps && joinTuned) {
    fprintf(stderr, "siga unitig: --join-min-overlap, --join-max-overlap, --join-slack, --join-kmer, --join-min-count, --joins, --join-mismatches and "
                    "--join-mismatch-permille need --join-overlaps\n");
    return 1;
  }
  if (joinOverlaps && scaffoldOut.empty()) {
    fprintf(stderr, "siga unitig: --join-overlaps needs --scaffold: it joins the neighbours of the scaffolds\n");
    return 1;
  }
  if (joinOverlaps && joinMaxOverlap < joinMinOverlap) {
    fprintf(stderr, "siga unitig: --join-max-overlap %zu is below --join-min-overlap %zu\n", joinMaxOverlap, joinMinOverlap);
    return 1;
  }
  if (maxGap < minGap) {
    fprintf(stderr, "siga unitig: --max-gap %zu is below --min-gap %zu\n", maxGap, minGap);
    return 1;
  }
  std::string input = argv[optind];
  if (prefix.empty()) prefix = sigah::Utils::stem(input);
  if (out.empty()) out = prefix + ".unitigs.fa";
  sigah::FMIndex fmi;
  if (!sigah::FMIndex::load(prefix, fmi, device)) {
    fprintf(stderr, "Failed to load FMIndex from %s: %s\n", prefix.c_str(), sigax_last_error());
    return -1;
  }
  sigah::Unitigger unitigger(!exhaustive, !norc);
  unitigger.setChimeric(chimLength, chimCoverage, chimDelta, chimThreshold);
  unitigger.setChimericOut(chimericOut);
  unitigger.setBubble(bubbleSpan, noBubbleBases ? -1 : (long)bubbleDivergence);
  unitigger.setBubbleOut(bubblesOut);
  unitigger.setBubbleEdits(bubbleEdits, bubbleEditPermille);
  unitigger.setTrim(cutTerminal, minBranchLength, minBranchCoverage);
  unitigger.setGraph(graph);
  unitigger.setRemoved(removed);
  unitigger.setMaxOverlap(delta, carefully, numReads, genomeSize, uniqThreshold);
  unitigger.setCutEdges(cutEdges);
  unitigger.setReduce(reduce);
  unitigger.setReducedEdges(reducedEdges);
  unitigger.setPairs(pairsOut, linksOut, maxSpan, outward, pairsBins, pairsShift);
  unitigger.setScaffold(scaffoldOut, scaffoldLayout, minPairs, linkRatio, minScaffoldUnitig, haveInsertSize ? (long long)insertSize : -1, minGap, maxGap);
  unitigger.setGapfill(gapfill, gapKmer, gapMinCount, gapSlack, gapMaxFill, gapsOut);
  unitigger.setJoinOverlaps(joinOverlaps, joinMinOverlap, joinMaxOverlap, joinSlack, joinKmer, joinMinCount, joinsOut);
  unitigger.setJoinMismatches(joinMismatches, joinMismatchPermille);
  if (mismatches) unitigger.setMismatch(mmo, containedOut);
  unitigger.setPlaceContained(placeContained);
  unitigger.setConsensus(vote, minVotes);
  if (!unitigger.run(fmi, input, minOverlap, out, layout, threads)) {
    fprintf(stderr, "Failed to build unitigs from reads %s: %s\n", input.c_str(), unitigger.error().c_str());
    return -1;
  }
  fprintf(stderr, "%llu unitigs, %llu bases, %llu overlaps merged, %llu circular\n", (unsigned long long)unitigger.unitigs(),
          (unsigned long long)unitigger.bases(), (unsigned long long)unitigger.merged(), (unsigned long long)unitigger.cycles());
  if (mismatches)
    fprintf(stderr, "%llu contained reads set aside; %llu of the unitigs counted above are such a read on its own, which no output shows%s\n",
            (unsigned long long)unitigger.containedReads(), (unsigned long long)unitigger.unitigsHidden(),
            cutTerminal ? " (the others went as islands in the trim rounds: --removed lists them)" : "");
  if (placeContained) {
    const uint64_t* pc = unitigger.placeClasses();
    fprintf(stderr, "%llu contained reads placed, %llu not: %llu without a record, %llu without a root, %llu with a removed root, %llu invalid; "
            "longest chain %llu\n", (unsigned long long)pc[SIGAX_CP_PLACED],
            (unsigned long long)(pc[SIGAX_CP_NO_RECORD] + pc[SIGAX_CP_NO_ROOT] + pc[SIGAX_CP_ROOT_REMOVED] + pc[SIGAX_CP_INVALID]),
            (unsigned long long)pc[SIGAX_CP_NO_RECORD], (unsigned long long)pc[SIGAX_CP_NO_ROOT], (unsigned long long)pc[SIGAX_CP_ROOT_REMOVED],
            (unsigned long long)pc[SIGAX_CP_INVALID], (unsigned long long)unitigger.placeStatus()[6]);
  }
  if (vote)
    fprintf(stderr, "%llu columns changed by the vote, %llu of depth below 2, %llu ties kept, largest depth %llu\n",
            (unsigned long long)unitigger.consensusChanged(), (unsigned long long)unitigger.consensusStatus()[3],
            (unsigned long long)unitigger.consensusStatus()[4], (unsigned long long)unitigger.consensusStatus()[6]);
  if (cutTerminal)
    fprintf(stderr, "%llu trim rounds, %llu islands and %llu dead ends removed, %llu reads\n", (unsigned long long)unitigger.trimRounds(),
            (unsigned long long)unitigger.islands(), (unsigned long long)unitigger.deadEnds(), (unsigned long long)unitigger.readsRemoved());
  if (reduce)
    fprintf(stderr, "%llu records transitive in the final graph, %llu in the first of %llu reduction passes\n",
            (unsigned long long)unitigger.reducedFinal(), (unsigned long long)unitigger.reducedFirst(), (unsigned long long)unitigger.reducePasses());
  if (delta)
    fprintf(stderr, "%llu records cut in %llu rounds\n", (unsigned long long)unitigger.recordsCut(), (unsigned long long)unitigger.cutRounds());
  if (chimLength)
    fprintf(stderr, "%llu chimeric unitigs removed, %llu reads\n", (unsigned long long)unitigger.chimericUnitigs(),
            (unsigned long long)unitigger.chimericReads());
  if (bubbleSpan)
    fprintf(stderr, "%llu bubble arms popped, %llu reads, %llu kept on divergence\n", (unsigned long long)unitigger.bubblesPopped(),
            (unsigned long long)unitigger.bubbleReads(), (unsigned long long)unitigger.bubblesKept());
  if (bubbleEdits)
    fprintf(stderr, "%llu indel arms popped, %llu reads, %llu kept on edits, %llu not compared\n", (unsigned long long)unitigger.indelsPopped(),
            (unsigned long long)unitigger.indelReads(), (unsigned long long)unitigger.indelsKept(),
            (unsigned long long)unitigger.indelsNotCompared());
  if (!pairsOut.empty())
    fprintf(stderr, "%llu pairs, %llu in one unitig (insert size %llu, delta %llu), %llu across unitigs in %llu links\n",
            (unsigned long long)unitigger.pairs(), (unsigned long long)unitigger.pairsSame(), (unsigned long long)unitigger.insertSize(),
            (unsigned long long)unitigger.insertDelta(), (unsigned long long)unitigger.pairsAcross(), (unsigned long long)unitigger.pairLinks());
  if (!scaffoldOut.empty())
    fprintf(stderr, "%llu scaffolds, %llu joins, %llu ambiguous links, %llu gap bases\n", (unsigned long long)unitigger.scaffolds(),
            (unsigned long long)unitigger.scaffoldJoins(), (unsigned long long)unitigger.scaffoldAmbiguous(),
            (unsigned long long)unitigger.scaffoldGapBases());
  if (gapfill)
    fprintf(stderr, "%llu gaps, %llu filled with %llu bases, %llu N left\n", (unsigned long long)unitigger.gaps(), (unsigned long long)unitigger.gapsFilled(),
            (unsigned long long)unitigger.gapFillBases(), (unsigned long long)unitigger.gapBasesLeft());
  if (joinOverlaps)
    fprintf(stderr, "%llu gaps looked at, %llu joined over %llu overlap bases, %llu N removed\n", (unsigned long long)unitigger.joinGaps(),
            (unsigned long long)unitigger.joinsMade(), (unsigned long long)unitigger.joinOverlapBases(), (unsigned long long)unitigger.joinNRemoved());
  if (joinOverlaps && joinMismatches)
    fprintf(stderr, "%llu of the joins through ends that nearly agree, %llu bases taken from the right unitig\n",
            (unsigned long long)unitigger.joinsApproximate(), (unsigned long long)unitigger.joinCorrected());
  return 0;
}

static int preqc_help() {
  // help text of src/preqc.cpp:209-222, plus the options of the k-mer distribution the reference computes no further than
  // GenomeEstimator::estimate's null index
  printf("siga preqc [OPTION] READSFILE\n"
         "Preform pre-assembly quality checks\n"
         "\n"
         "      -h, --help                       display this help and exit\n"
         "\n"
         "      -o, --prefix=PREFIX              use PREFIX instead of prefix of READSFILE for the name of the index file (.bwt)\n"
         "      -k, --kmer=N                     the length of the k-mers to count (default: 31)\n"
         "      -n, --samples=N                  draw N rows of the index and count the k-mers of their strings (default: 50000)\n"
         "          --seed=N                     seed of the std::mt19937_64 that draws the rows (default: 1)\n"
         "          --all                        count every read once instead of sampled rows\n"
         "          --max-count=N                counts of N and more share the last bin (default: 1024)\n"
         "      -t, --threads=NUM                accepted; the GPU does the counting\n"
         "          --device=NUM                 GPU to use (default: 0)\n"
         "          --simple                     not built: the metrics that do not need the FM-index (and the QualityScores\n"
         "                                       block) are a host pass over FASTQ qualities with an unseeded sampler\n"
         "\n"
         "Prints {\"KmerDistribution\": {...}} on stdout: windows by the number of times their k-mer occurs in the reads, both\n"
         "strands together.  READSFILE only names the index; the strings are read back out of it.\n"
         "\n");
  return 256;
}

// src/preqc.cpp:20-60, 227-236: the k-mer distribution of GenomeEstimator, with an index
static int run_preqc(int argc, char** argv) {
  enum { OPT_SIMPLE = 1, OPT_SEED, OPT_ALL, OPT_MAX_COUNT, OPT_DEVICE };
  static const option longopts[] = {{"log4cxx", required_argument, nullptr, 'c'},  {"ini", required_argument, nullptr, 's'},
                                    {"prefix", required_argument, nullptr, 'o'},   {"threads", required_argument, nullptr, 't'},
                                    {"kmer", required_argument, nullptr, 'k'},     {"samples", required_argument, nullptr, 'n'},
                                    {"seed", required_argument, nullptr, OPT_SEED}, {"all", no_argument, nullptr, OPT_ALL},
                                    {"max-count", required_argument, nullptr, OPT_MAX_COUNT}, {"simple", no_argument, nullptr, OPT_SIMPLE},
                                    {"device", required_argument, nullptr, OPT_DEVICE}, {"help", no_argument, nullptr, 'h'},
                                    {nullptr, 0, nullptr, 0}};
  std::string prefix;
  sigah::KmerSpectrum::Options o;
  bool help = false, simple = false;
  int device = 0, c;
  std::vector<std::string> ini_store;
  std::vector<char*> ini_argv;
  if (apply_ini(argc, argv, longopts, &ini_store, &ini_argv) != 0) return 1;
  argc = (int)ini_argv.size();
  argv = ini_argv.data();
  while ((c = getopt_long(argc, argv, "c:s:o:t:k:n:h", longopts, nullptr)) != -1) {
    switch (c) {
      case 'o': prefix = optarg; break;
      case 't': break;
      case 'k': o.kmerSize = strtoull(optarg, nullptr, 10); break;
      case 'n': o.samples = strtoull(optarg, nullptr, 10); break;
      case OPT_SEED: o.seed = strtoull(optarg, nullptr, 10); break;
      case OPT_ALL: o.all = true; break;
      case OPT_MAX_COUNT: o.maxCount = strtoull(optarg, nullptr, 10); break;
      case OPT_SIMPLE: simple = true; break;
      case OPT_DEVICE: device = atoi(optarg); break;
      case 'h': help = true; break;
      default: break;
    }
  }
  if (help || argc - optind != 1) return preqc_help();
  std::string input = argv[optind];
  if (prefix.empty()) prefix = sigah::Utils::stem(input);
  if (simple) {
    fprintf(stderr, "Failed to do pre-assembly quality checks for reads %s: --simple is not built\n", input.c_str());
    return -1;
  }
  if (o.maxCount == 0 || o.maxCount > (1ull << 28)) {
    fprintf(stderr, "Failed to do pre-assembly quality checks for reads %s: --max-count must be between 1 and 2^28\n", input.c_str());
    return -1;
  }
  sigah::FMIndex fmi;
  if (!sigah::FMIndex::loadForward(prefix, fmi, device)) {
    fprintf(stderr, "Failed to load FMIndex from %s: %s\n", prefix.c_str(), sigax_last_error());
    return -1;
  }
  sigah::KmerSpectrum spectrum(o);
  if (!spectrum.run(fmi)) {
    fprintf(stderr, "Failed to do pre-assembly quality checks for reads %s: %s\n", input.c_str(), spectrum.error().c_str());
    return -1;
  }
  const std::string text = spectrum.json();
  if (fwrite(text.data(), 1, text.size(), stdout) != text.size()) return -1;
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) return usage();
  const auto t0 = std::chrono::steady_clock::now();
  std::string cmd = argv[1];
  int rc = 256;
  if (cmd == "index") rc = run_index(argc - 1, argv + 1);
  else if (cmd == "rmdup") rc = run_rmdup(argc - 1, argv + 1);
  else if (cmd == "correct") rc = run_correct(argc - 1, argv + 1);
  else if (cmd == "overlap") rc = run_overlap(argc - 1, argv + 1);
  else if (cmd == "match") rc = run_match(argc - 1, argv + 1);
  else if (cmd == "locate") rc = run_locate(argc - 1, argv + 1);
  else if (cmd == "preqc") rc = run_preqc(argc - 1, argv + 1);
  else if (cmd == "unitig") rc = run_unitig(argc - 1, argv + 1);
  else return usage();
  if (getenv("SIGA_TIMING"))
    fprintf(stderr, "[siga] %-28s %8.3f s\n", "main() total", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
  // every output file is closed by now: leave without tearing the HIP runtime down (tens of milliseconds of nothing)
  // (SIGA_CLEAN_EXIT=1: the ordinary way out, for profilers that write their report from an exit handler)
  fflush(nullptr);
  if (getenv("SIGA_CLEAN_EXIT")) return rc & 0xFF;
  _exit(rc & 0xFF);
}
