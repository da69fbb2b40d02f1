"""ctypes bindings of libsiga_host.so (host C++ mirror of the reference classes: `siga index`, OverlapBuilder::build)."""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# SIGA_HOST_LIB / SIGA_CLI: another build of the host side (tools/sanitize_host.sh runs the CPU tests on ASan/UBSan and TSan builds)
LIB_PATH = os.environ.get("SIGA_HOST_LIB", os.path.join(HERE, "lib", "libsiga_host.so"))
CLI_PATH = os.environ.get("SIGA_CLI", os.path.join(HERE, "lib", "siga"))
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("siga_amd host library missing: %s (python -m siga_amd.build)" % LIB_PATH)
        L = C.CDLL(LIB_PATH)
        L.sigah_index_build.argtypes = [C.c_char_p, C.c_void_p, C.c_uint64, C.c_char_p, C.c_int, C.c_char_p, C.c_uint64]
        L.sigah_index_build_dev.argtypes = [C.c_char_p, C.c_void_p, C.c_uint64, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int,
                                            C.c_char_p, C.c_uint64]
        L.sigah_index_file_dev.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_uint64]
        L.sigah_index_file.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.c_uint64]
        L.sigah_index_file_sais.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_uint64]
        L.sigah_overlap_file.argtypes = [C.c_char_p, C.c_char_p, C.c_uint64, C.c_char_p, C.c_int, C.c_int, C.c_uint64,
                                         C.c_uint64, C.c_int, C.c_char_p, C.c_uint64]
        L.sigah_overlap_file_gpus.argtypes = [C.c_char_p, C.c_char_p, C.c_uint64, C.c_char_p, C.c_int, C.c_int, C.c_uint64,
                                              C.c_uint64, C.c_int, C.c_int, C.c_char_p, C.c_uint64]
        L.sigah_parse_file.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_int]
        L.sigah_parse_file.restype = C.c_int64
        L.sigah_stem.argtypes = [C.c_char_p, C.c_char_p, C.c_uint64]
        L.sigah_write_file.argtypes = [C.c_char_p, C.c_char_p, C.c_uint64, C.c_uint64]
        L.sigah_correct_file.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64,
                                         C.c_int, C.c_char_p, C.c_uint64]
        L.sigah_correct_overlap_file.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p,
                                                 C.c_char_p, C.c_uint64]
        L.sigah_overlap_mismatch_file.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p,
                                                  C.c_char_p, C.c_uint64]
        L.sigah_overlap_mismatch_containments_file.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_void_p, C.c_uint64, C.c_int,
                                                               C.c_void_p, C.c_char_p, C.c_uint64]
        L.sigah_format_asqg.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_char_p, C.c_int]
        L.sigah_format_asqg.restype = C.c_int64
        L.sigah_rmdup_file.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.c_uint64]
        L.sigah_match_files.argtypes = [C.POINTER(C.c_char_p), C.c_uint64, C.c_char_p, C.c_uint64, C.c_int, C.c_int, C.c_char_p,
                                        C.c_uint64, C.c_char_p, C.c_uint64]
        L.sigah_locate_files.argtypes = [C.POINTER(C.c_char_p), C.c_uint64, C.c_char_p, C.c_uint32, C.c_uint32, C.c_int, C.c_int,
                                         C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64]
        L.sigah_unitig_file.argtypes = [C.c_char_p, C.c_char_p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_char_p,
                                        C.c_uint64, C.c_char_p, C.c_uint64]
        L.sigah_unitig_trim_file.argtypes = [C.c_char_p, C.c_char_p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_char_p,
                                             C.c_uint64, C.c_uint64, C.c_uint64, C.c_int64, C.c_char_p, C.c_char_p, C.c_void_p,
                                             C.c_char_p, C.c_uint64]
        L.sigah_unitig_prune_file.argtypes = [C.c_char_p, C.c_char_p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_char_p,
                                              C.c_uint64, C.c_uint64, C.c_uint64, C.c_int64, C.c_char_p, C.c_char_p, C.c_uint64, C.c_int,
                                              C.c_uint64, C.c_uint64, C.c_double, C.c_char_p, C.c_void_p, C.c_char_p, C.c_uint64]
        L.sigah_unitig_chimeric_file.argtypes = [C.c_char_p, C.c_char_p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_char_p,
                                                 C.c_uint64, C.c_uint64, C.c_uint64, C.c_int64, C.c_char_p, C.c_char_p, C.c_uint64, C.c_int,
                                                 C.c_uint64, C.c_uint64, C.c_double, C.c_char_p, C.c_uint64, C.c_int64, C.c_uint64, C.c_double,
                                                 C.c_char_p, C.c_void_p, C.c_char_p, C.c_uint64]
        L.sigah_unitig_bubble_file.argtypes = [C.c_char_p, C.c_char_p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_char_p,
                                               C.c_uint64, C.c_uint64, C.c_uint64, C.c_int64, C.c_char_p, C.c_char_p, C.c_uint64, C.c_int,
                                               C.c_uint64, C.c_uint64, C.c_double, C.c_char_p, C.c_uint64, C.c_int64, C.c_uint64, C.c_double,
                                               C.c_char_p, C.c_uint64, C.c_int64, C.c_char_p, C.c_void_p, C.c_char_p, C.c_uint64]
        L.sigah_unitig_indel_file.argtypes = [C.c_char_p, C.c_char_p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_char_p,
                                              C.c_uint64, C.c_uint64, C.c_uint64, C.c_int64, C.c_char_p, C.c_char_p, C.c_uint64, C.c_int,
                                              C.c_uint64, C.c_uint64, C.c_double, C.c_char_p, C.c_uint64, C.c_int64, C.c_uint64, C.c_double,
                                              C.c_char_p, C.c_uint64, C.c_int64, C.c_char_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_char_p,
                                              C.c_uint64]
        L.sigah_unitig_consensus_file.argtypes = [C.c_char_p, C.c_char_p, C.c_uint64, C.c_int, C.c_int, C.c_int, C.c_char_p, C.c_char_p,
                                                  C.c_uint64, C.c_uint64, C.c_uint64, C.c_int64, C.c_char_p, C.c_char_p, C.c_uint64, C.c_int,
                                                  C.c_uint64, C.c_uint64, C.c_double, C.c_char_p, C.c_uint64, C.c_int64, C.c_uint64, C.c_double,
                                                  C.c_char_p, C.c_uint64, C.c_int64, C.c_char_p, C.c_uint64, C.c_uint64, C.c_int, C.c_int64,
                                                  C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_uint64, C.c_char_p, C.c_void_p,
                                                  C.c_char_p, C.c_uint64]
        a = L.sigah_unitig_consensus_file.argtypes
        L.sigah_unitig_placed_file.argtypes = a[:-3] + [C.c_int] + a[-3:]
        L.sigah_preqc.argtypes = [C.c_char_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_uint64, C.c_int, C.c_char_p,
                                  C.c_uint64, C.c_char_p, C.c_uint64]
        _lib = L
    return _lib


def index_build(seq_bytes, offs, prefix, threads=2):
    """`siga index` for in-memory reads: writes <prefix>.{bwt,sai,rbwt,rsai}."""
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    err = C.create_string_buffer(512)
    buf = seq_bytes if isinstance(seq_bytes, (bytes, bytearray)) else np.ascontiguousarray(seq_bytes).tobytes()
    if lib().sigah_index_build(buf, offs.ctypes.data, len(offs) - 1, prefix.encode(), threads, err, 512) != 0:
        raise RuntimeError("siga index failed: " + err.value.decode())


def index_build_gpu(seq_bytes, offs, prefix, device=0, threads=2):
    """`siga index` for in-memory reads on the GPU (sigax_build_strand): writes <prefix>.{bwt,sai,rbwt,rsai}."""
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    err = C.create_string_buffer(512)
    if isinstance(seq_bytes, np.ndarray):
        arr = np.ascontiguousarray(seq_bytes)
        ptr = C.c_char_p(arr.ctypes.data)  # no copy: BASELINE-sized sets are gigabytes
    else:
        ptr = seq_bytes
    if lib().sigah_index_build_dev(ptr, offs.ctypes.data, len(offs) - 1, prefix.encode(), device, threads, 1, 1, err, 512) != 0:
        raise RuntimeError("siga index failed: " + err.value.decode())


def index_file_gpu(reads_path, prefix, device=0, threads=2):
    err = C.create_string_buffer(512)
    if lib().sigah_index_file_dev(reads_path.encode(), prefix.encode(), device, threads, 1, 1, err, 512) != 0:
        raise RuntimeError("siga index failed: " + err.value.decode())


def index_file(reads_path, prefix, threads=2):
    err = C.create_string_buffer(512)
    if lib().sigah_index_file(reads_path.encode(), prefix.encode(), threads, err, 512) != 0:
        raise RuntimeError("siga index failed: " + err.value.decode())


def index_file_sais(reads_path, prefix, threads=2):
    """`siga index -a sais`: SAISBuilder's suffix order (every read's own sentinel, ordered by read index), host sorter"""
    err = C.create_string_buffer(512)
    if lib().sigah_index_file_sais(reads_path.encode(), prefix.encode(), threads, 1, 1, err, 512) != 0:
        raise RuntimeError("siga index -a sais failed: " + err.value.decode())


def overlap_file(reads_path, prefix, min_overlap, output, irreducible=True, rc=True, threads=1, batch=10000, device=0, gpus=1,
                 error_permille=None, containments=None, **seed):
    """FMIndex::load + OverlapBuilder::build in the host C++ library (GPU compute), reads sharded over `gpus` GPUs.
    error_permille given (`siga overlap -e`): FMIndex::loadForwardSai + MismatchOverlapper::run instead -- every overlap of
    min_overlap columns with that many mismatches per mille at most, the rules of include/sigax.h, with seed_length, seed_stride,
    max_seed_hits and max_candidates as keywords; one GPU, both strands; -> the eight status words.  containments: a path
    (`--containments FILE`, with error_permille only) for one line per containment record -- contained name, container name,
    offset, + or -, mismatches; status[7] then counts those records too."""
    err = C.create_string_buffer(512)
    if error_permille is not None:
        if gpus != 1 or not rc:
            raise ValueError("error_permille with gpus=%r, rc=%r" % (gpus, rc))
        from . import _lib as core
        params = core.MmoParams(int(error_permille), min_overlap=int(min_overlap), **seed)
        status = np.zeros(8, dtype=np.uint64)
        if lib().sigah_overlap_mismatch_containments_file(reads_path.encode(), prefix.encode(), output.encode(),
                                                          containments.encode() if containments else None, C.addressof(params), threads,
                                                          device, status.ctypes.data, err, 512) != 0:
            raise RuntimeError("siga overlap failed: " + err.value.decode())
        return status
    if seed or containments:
        raise ValueError("%r without error_permille" % (sorted(seed) + (["containments"] if containments else [])))
    r = lib().sigah_overlap_file_gpus(reads_path.encode(), prefix.encode(), min_overlap, output.encode(), int(irreducible), int(rc),
                                      threads, batch, device, gpus, err, 512)
    if r != 0:
        raise RuntimeError("siga overlap failed: " + err.value.decode())


def rmdup_file(reads_path, prefix, output, duplicates, device=0):
    """FMIndex::load + OverlapBuilder::rmdup in the host C++ library (GPU compute)."""
    err = C.create_string_buffer(512)
    if lib().sigah_rmdup_file(reads_path.encode(), prefix.encode(), output.encode(), duplicates.encode(), device, err, 512) != 0:
        raise RuntimeError("siga rmdup failed: " + err.value.decode())


def correct_file(reads_path, prefix, output, k=31, threshold=3, rounds=None, offset=1, device=0, algorithm="kmer", **pile):
    """FMIndex::load + CorrectProcessor::process in the host C++ library (GPU compute).  algorithm "kmer": the k-mer
    corrector with k, threshold, rounds (default 10) and offset.  algorithm "overlap": the pile-up of include/sigax.h with
    rounds (default 1) and the fields of sigax_pile_params as keywords (seed_length=..., min_overlap=..., ...); needs
    <prefix>.sai; -> the eight status words added up over the batches."""
    err = C.create_string_buffer(512)
    if algorithm == "overlap":
        from . import _lib as core
        params = core.PileParams(**pile)
        status = np.zeros(8, dtype=np.uint64)
        if lib().sigah_correct_overlap_file(reads_path.encode(), prefix.encode(), output.encode(), C.addressof(params),
                                            1 if rounds is None else int(rounds), device, status.ctypes.data, err, 512) != 0:
            raise RuntimeError("siga correct failed: " + err.value.decode())
        return status
    if algorithm != "kmer" or pile:
        raise ValueError("algorithm %r with %r" % (algorithm, sorted(pile)))
    if lib().sigah_correct_file(reads_path.encode(), prefix.encode(), output.encode(), k, threshold, 10 if rounds is None else rounds,
                                offset, device, err, 512) != 0:
        raise RuntimeError("siga correct failed: " + err.value.decode())


def match_files(paths, prefix, max_length=None, rc=True, device=0, out=None, batch_reads=0):
    """`siga match`: FMIndex::load(<prefix>.bwt) + Matcher::run over the files of `paths`, in order; the VT lines go to the file
    `out`, or to stdout.  max_length None: whole reads.  batch_reads: reads per device batch (0: from the free memory)."""
    err = C.create_string_buffer(512)
    arr = (C.c_char_p * len(paths))(*[p.encode() for p in paths])
    lim = (1 << 64) - 1 if max_length is None else int(max_length)
    if lib().sigah_match_files(arr, len(paths), prefix.encode(), lim, int(rc), device, (out or "").encode(), batch_reads, err, 512) != 0:
        raise RuntimeError("siga match failed: " + err.value.decode())


def locate_files(paths, prefix, rc=True, max_hits=1000, max_len=None, device=0, out=None, batch_queries=0):
    """`siga locate`: FMIndex::loadForwardSai(<prefix>.bwt, <prefix>.sai) + Locator::run over the query files of `paths`, in
    order; the QT and HT lines go to the file `out`, or to stdout.  max_len None: walks of any length.  batch_queries: queries
    per device batch (0: the default)."""
    err = C.create_string_buffer(512)
    arr = (C.c_char_p * len(paths))(*[p.encode() for p in paths])
    lim = (1 << 32) - 1 if max_len is None else int(max_len)
    if lib().sigah_locate_files(arr, len(paths), prefix.encode(), int(max_hits), lim, int(rc), device, (out or "").encode(),
                                batch_queries, err, 512) != 0:
        raise RuntimeError("siga locate failed: " + err.value.decode())


def unitig_file(reads_path, prefix, min_overlap, out=None, layout=None, irreducible=True, rc=True, device=0, piece_reads=0, cut_terminal=0,
                min_branch_length=150, min_branch_coverage=None, graph=None, removed=None, max_overlap_delta=0, max_overlap_carefully=False,
                num_reads=None, genome_size=None, uniq_threshold=13.0, cut_edges=None, min_chimeric_length=0, min_chimeric_coverage=None,
                max_chimeric_delta=0, chimeric_threshold=0.0, chimeric=None, max_bubble_span=0, bubble_divergence=50, bubbles=None,
                bubble_edits=0, bubble_edit_permille=50, reduce=False, error_permille=None, consensus=None, min_votes=1, contained=None, place_contained=False,
                **seed):
    """`siga unitig`: FMIndex::load + Unitigger::run; the FASTA goes to the file `out`, or to stdout, the placements to the file
    `layout` when one is named.  piece_reads: reads per overlap call (0: 2^20); the result does not depend on it.
    cut_terminal (-x), min_branch_length (-n), min_branch_coverage (-C, None: no coverage test): tip trimming, 0 rounds = none;
    graph: the file of the unitig graph (ASQG, gzip if it ends in .gz); removed: the file of "name<TAB>round" lines.  With any
    of them -> dict(unitigs, bases, merged, circular, rounds, islands, dead_ends, reads_removed).
    max_overlap_delta (-d; 0: none), max_overlap_carefully, num_reads (-N; None: the reads of the file), genome_size (-G),
    uniq_threshold (-T): non-maximal overlap cutting in the rounds; cut_edges: the file of "query<TAB>target<TAB>length<TAB>round"
    lines.  With a delta the dict also holds records_cut and cut_rounds.
    min_chimeric_length (-l; 0: none), min_chimeric_coverage (-A, None: no coverage test), max_chimeric_delta (-a),
    chimeric_threshold (-T as the chimeric step takes it): chimeric unitig removal as the last step of a round; chimeric: the file
    of "name<TAB>round" lines of the reads it removed.  With a length the dict also holds chimeric_unitigs and chimeric_reads.
    max_bubble_span (-b; 0: none), bubble_divergence (--bubble-divergence, per mille; None: --no-bubble-bases): bubble popping between
    the trim and the chimeric step of a round; bubbles: the file of "name<TAB>round" lines of the reads it removed.  With a span the
    dict also holds bubbles_popped, bubble_reads and bubbles_kept.
    bubble_edits (--bubble-edits; 0: none; at most 31, with a span of at most 4096), bubble_edit_permille (--bubble-edit-permille):
    indel bubble popping between the bubble and the chimeric step of a round; `bubbles` then also lists the reads it removed, as
    "name<TAB>round<TAB>indel" lines behind the others.  With edits the dict also holds indels_popped, indel_reads, indels_kept and
    indels_not_compared.
    error_permille (-e; None: exact overlaps): mismatch overlaps in, found as `siga overlap -e` finds them with the seed options
    seed_length, seed_stride, max_seed_hits and max_candidates (**seed); contained reads are set aside, their names go to the file
    `contained`.  consensus (None: on exactly when error_permille is given), min_votes: the consensus pass behind the unitig call.
    reduce (--reduce): the transitive reduction in the rounds.  With any of them -> the dict of bubble_edits plus reduced,
    contained_reads, columns_changed and shallow_columns.
    place_contained (--place-contained, with error_permille only): every contained read placed where its container lies, so that
    it votes, counts and pairs; the dict then also holds contained_placed."""
    err = C.create_string_buffer(512)
    if min_votes != 1 and not (consensus or (consensus is None and error_permille is not None)):
        raise ValueError("min_votes needs the consensus pass")
    if place_contained and error_permille is None:
        raise ValueError("place_contained applies to error_permille only")
    if error_permille is not None or consensus or reduce or contained is not None or seed:
        unknown = set(seed) - {"seed_length", "seed_stride", "max_seed_hits", "max_candidates"}
        if unknown:
            raise TypeError("unitig_file: unknown option %s" % ", ".join(sorted(unknown)))
        if error_permille is None and (seed or contained is not None):
            raise ValueError("the seed options and `contained` apply to error_permille only")
        status = np.zeros(24, dtype=np.uint64)
        if lib().sigah_unitig_placed_file(reads_path.encode(), prefix.encode(), min_overlap, int(irreducible), int(rc), device,
                                             (out or "").encode(), (layout or "").encode(), piece_reads, int(cut_terminal), int(min_branch_length),
                                             -1 if min_branch_coverage is None else int(min_branch_coverage), (graph or "").encode(),
                                             (removed or "").encode(), int(max_overlap_delta), int(max_overlap_carefully), int(num_reads or 0),
                                             int(genome_size or 0), float(uniq_threshold), (cut_edges or "").encode(), int(min_chimeric_length),
                                             -1 if min_chimeric_coverage is None else int(min_chimeric_coverage), int(max_chimeric_delta),
                                             float(chimeric_threshold), (chimeric or "").encode(), int(max_bubble_span),
                                             -1 if bubble_divergence is None else int(bubble_divergence), (bubbles or "").encode(),
                                             int(bubble_edits), int(bubble_edit_permille), int(bool(reduce)),
                                             -1 if error_permille is None else int(error_permille), int(seed.get("seed_length", 24)),
                                             int(seed.get("seed_stride", 12)), int(seed.get("max_seed_hits", 256)),
                                             int(seed.get("max_candidates", 512)), -1 if consensus is None else int(bool(consensus)),
                                             int(min_votes), (contained or "").encode(), int(bool(place_contained)), status.ctypes.data, err,
                                             512) != 0:
            raise RuntimeError("siga unitig failed: " + err.value.decode())
        return dict(zip(("unitigs", "bases", "merged", "circular", "rounds", "islands", "dead_ends", "reads_removed", "records_cut", "cut_rounds",
                         "chimeric_unitigs", "chimeric_reads", "bubbles_popped", "bubble_reads", "bubbles_kept", "indels_popped", "indel_reads",
                         "indels_kept", "indels_not_compared", "reduced", "contained_reads", "columns_changed", "shallow_columns") +
                        (("contained_placed",) if place_contained else ()), (int(x) for x in status)))
    if bubble_edits:
        status = np.zeros(19, dtype=np.uint64)
        if lib().sigah_unitig_indel_file(reads_path.encode(), prefix.encode(), min_overlap, int(irreducible), int(rc), device,
                                         (out or "").encode(), (layout or "").encode(), piece_reads, int(cut_terminal), int(min_branch_length),
                                         -1 if min_branch_coverage is None else int(min_branch_coverage), (graph or "").encode(),
                                         (removed or "").encode(), int(max_overlap_delta), int(max_overlap_carefully), int(num_reads or 0),
                                         int(genome_size or 0), float(uniq_threshold), (cut_edges or "").encode(), int(min_chimeric_length),
                                         -1 if min_chimeric_coverage is None else int(min_chimeric_coverage), int(max_chimeric_delta),
                                         float(chimeric_threshold), (chimeric or "").encode(), int(max_bubble_span),
                                         -1 if bubble_divergence is None else int(bubble_divergence), (bubbles or "").encode(),
                                         int(bubble_edits), int(bubble_edit_permille), status.ctypes.data, err, 512) != 0:
            raise RuntimeError("siga unitig failed: " + err.value.decode())
        return dict(zip(("unitigs", "bases", "merged", "circular", "rounds", "islands", "dead_ends", "reads_removed", "records_cut", "cut_rounds",
                         "chimeric_unitigs", "chimeric_reads", "bubbles_popped", "bubble_reads", "bubbles_kept", "indels_popped", "indel_reads",
                         "indels_kept", "indels_not_compared"), (int(x) for x in status)))
    if max_bubble_span:
        status = np.zeros(15, dtype=np.uint64)
        if lib().sigah_unitig_bubble_file(reads_path.encode(), prefix.encode(), min_overlap, int(irreducible), int(rc), device,
                                          (out or "").encode(), (layout or "").encode(), piece_reads, int(cut_terminal), int(min_branch_length),
                                          -1 if min_branch_coverage is None else int(min_branch_coverage), (graph or "").encode(),
                                          (removed or "").encode(), int(max_overlap_delta), int(max_overlap_carefully), int(num_reads or 0),
                                          int(genome_size or 0), float(uniq_threshold), (cut_edges or "").encode(), int(min_chimeric_length),
                                          -1 if min_chimeric_coverage is None else int(min_chimeric_coverage), int(max_chimeric_delta),
                                          float(chimeric_threshold), (chimeric or "").encode(), int(max_bubble_span),
                                          -1 if bubble_divergence is None else int(bubble_divergence), (bubbles or "").encode(),
                                          status.ctypes.data, err, 512) != 0:
            raise RuntimeError("siga unitig failed: " + err.value.decode())
        return dict(zip(("unitigs", "bases", "merged", "circular", "rounds", "islands", "dead_ends", "reads_removed", "records_cut", "cut_rounds",
                         "chimeric_unitigs", "chimeric_reads", "bubbles_popped", "bubble_reads", "bubbles_kept"), (int(x) for x in status)))
    if min_chimeric_length:
        status = np.zeros(12, dtype=np.uint64)
        if lib().sigah_unitig_chimeric_file(reads_path.encode(), prefix.encode(), min_overlap, int(irreducible), int(rc), device,
                                            (out or "").encode(), (layout or "").encode(), piece_reads, int(cut_terminal), int(min_branch_length),
                                            -1 if min_branch_coverage is None else int(min_branch_coverage), (graph or "").encode(),
                                            (removed or "").encode(), int(max_overlap_delta), int(max_overlap_carefully), int(num_reads or 0),
                                            int(genome_size or 0), float(uniq_threshold), (cut_edges or "").encode(), int(min_chimeric_length),
                                            -1 if min_chimeric_coverage is None else int(min_chimeric_coverage), int(max_chimeric_delta),
                                            float(chimeric_threshold), (chimeric or "").encode(), status.ctypes.data, err, 512) != 0:
            raise RuntimeError("siga unitig failed: " + err.value.decode())
        return dict(zip(("unitigs", "bases", "merged", "circular", "rounds", "islands", "dead_ends", "reads_removed", "records_cut", "cut_rounds",
                         "chimeric_unitigs", "chimeric_reads"), (int(x) for x in status)))
    if max_overlap_delta:
        status = np.zeros(10, dtype=np.uint64)
        if lib().sigah_unitig_prune_file(reads_path.encode(), prefix.encode(), min_overlap, int(irreducible), int(rc), device, (out or "").encode(),
                                         (layout or "").encode(), piece_reads, int(cut_terminal), int(min_branch_length),
                                         -1 if min_branch_coverage is None else int(min_branch_coverage), (graph or "").encode(),
                                         (removed or "").encode(), int(max_overlap_delta), int(max_overlap_carefully), int(num_reads or 0),
                                         int(genome_size or 0), float(uniq_threshold), (cut_edges or "").encode(), status.ctypes.data, err,
                                         512) != 0:
            raise RuntimeError("siga unitig failed: " + err.value.decode())
        return dict(zip(("unitigs", "bases", "merged", "circular", "rounds", "islands", "dead_ends", "reads_removed", "records_cut", "cut_rounds"),
                        (int(x) for x in status)))
    if not cut_terminal and graph is None and removed is None:
        if lib().sigah_unitig_file(reads_path.encode(), prefix.encode(), min_overlap, int(irreducible), int(rc), device, (out or "").encode(),
                                   (layout or "").encode(), piece_reads, err, 512) != 0:
            raise RuntimeError("siga unitig failed: " + err.value.decode())
        return None
    status = np.zeros(8, dtype=np.uint64)
    if lib().sigah_unitig_trim_file(reads_path.encode(), prefix.encode(), min_overlap, int(irreducible), int(rc), device, (out or "").encode(),
                                    (layout or "").encode(), piece_reads, int(cut_terminal), int(min_branch_length),
                                    -1 if min_branch_coverage is None else int(min_branch_coverage), (graph or "").encode(),
                                    (removed or "").encode(), status.ctypes.data, err, 512) != 0:
        raise RuntimeError("siga unitig failed: " + err.value.decode())
    return dict(zip(("unitigs", "bases", "merged", "circular", "rounds", "islands", "dead_ends", "reads_removed"), (int(x) for x in status)))


def preqc(prefix, k=31, samples=50000, seed=1, all_reads=False, max_count=1024, device=0, out=None, batch_rows=0):
    """`siga preqc`: FMIndex::load(<prefix>.bwt) + KmerSpectrum over `samples` rows drawn from std::mt19937_64(seed), or over every
    read once (all_reads); the JSON object goes to the file `out`, or to stdout.  batch_rows: rows per device batch (0: from the
    free memory)."""
    err = C.create_string_buffer(512)
    if lib().sigah_preqc(prefix.encode(), k, samples, seed, int(all_reads), max_count, device, (out or "").encode(), batch_rows,
                         err, 512) != 0:
        raise RuntimeError("siga preqc failed: " + err.value.decode())


def parse_file(path, out_path, parallel=True, threads=4):
    """records of a FASTA/FASTQ file as the host library reads them (parallel loader or record-at-a-time reader)"""
    return lib().sigah_parse_file(path.encode(), 0 if parallel else 1, out_path.encode(), threads)


def read_table(path, out_path, threads=4):
    """the edge converter's read table as the host builds it: one "rank<TAB>length" line per read (name ranks under
    std::string's order, equal names equal rank)"""
    return lib().sigah_parse_file(path.encode(), 2, out_path.encode(), threads)


def write_file(path, data, pieces=1):
    """The host library's output stream (multi-threaded single-member gzip when the name ends with .gz)."""
    if lib().sigah_write_file(path.encode(), data, len(data), pieces) != 0:
        raise IOError("cannot write " + path)


def stem(path):
    out = C.create_string_buffer(1024)
    lib().sigah_stem(path.encode(), out, 1024)
    return out.value.decode()


def format_asqg(reads_path, substring, edges, min_overlap, out_path, threads=4):
    """Test hook: the text side of OverlapBuilder::build without a GPU (loader, VT lines, raw-pointer ED formatter, output
    stream) for given substring flags (uint8[n]) and edge records (EDGE_DTYPE[k]).  Returns the number of reads."""
    sub = np.ascontiguousarray(substring, dtype=np.uint8)
    ed = np.ascontiguousarray(edges)
    assert ed.dtype.itemsize == 16
    n = lib().sigah_format_asqg(reads_path.encode(), sub.ctypes.data, ed.ctypes.data, len(ed), min_overlap, out_path.encode(), threads)
    if n < 0:
        raise RuntimeError("sigah_format_asqg failed")
    return int(n)
