"""Python mirror of the reference's overlap interface on top of the C-ABI (include/sigax.h).

Names follow the reference: `FMIndexPair.load(prefix)` stands for the two FMIndex::load calls of
Overlapping::run (src/overlap.cpp:41-42); `OverlapBuilder(fmi_pair, prefix, irreducible, rc)` mirrors
src/overlap_builder.h:19-45 with `overlap(reads, min_overlap)` (batched OverlapBuilder::overlap) and
`build(input, min_overlap, output)` (HT/VT/ED text as src/overlap_builder.cpp:423-509 writes it at -t 1).
All compute is in libsigax.so; nothing here computes overlaps on the CPU.
"""
import ctypes as C
import gzip
import os

import numpy as np

from . import _lib
from ._lib import BLOCK_DTYPE, EDGE_DTYPE, HIT_DTYPE, PLACEMENT_DTYPE, SIGAX_DUPLICATE, SIGAX_EDGES, SIGAX_IRREDUCIBLE, SIGAX_RC


class SigaxError(RuntimeError):
    def __init__(self, code, where):
        super().__init__("%s failed (%d): %s" % (where, code, _lib.last_error()))
        self.code = code


def _check(code, where):
    if code != 0:
        raise SigaxError(code, where)


MATCH_NONE = (1 << 64) - 1  # SIGAX_MATCH_NONE; as max_length: never split
NO_STRETCH = (1 << 64) - 1  # SIGAX_NO_STRETCH
MAX_STRING_LEN = (1 << 32) - 1  # get_strings / kmer_spectrum: walks as long as the index's longest stretch


def pack_reads(seqs):
    if isinstance(seqs, tuple):  # (uint8 array of concatenated bases, offsets u64[n+1]): BASELINE-sized sets, no copies
        buf, offs = seqs
        return np.ascontiguousarray(buf, dtype=np.uint8), np.ascontiguousarray(offs, dtype=np.uint64)
    bs = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
    offs = np.zeros(len(bs) + 1, dtype=np.uint64)
    if bs:
        offs[1:] = np.cumsum([len(b) for b in bs], dtype=np.uint64)
    return b"".join(bs), offs


def name_ranks(names):
    """rank of each name under std::string operator< (bytewise), equal names share a rank."""
    bs = [n.encode() if isinstance(n, str) else bytes(n) for n in names]
    order = {b: i for i, b in enumerate(sorted(set(bs)))}
    return np.array([order[b] for b in bs], dtype=np.uint32)


def read_sequences(path):
    """FASTA/FASTQ reader with the reference's semantics (src/kseq.cpp:127-228): returns (name, comment, seq)."""
    opener = gzip.open if path.endswith(".gz") else open
    with opener(path, "rb") as f:
        data = f.read().decode("latin-1")
    out = []
    ws = " \t\n\v\f\r"
    lines = [l.strip(ws) for l in data.split("\n")]
    lines = [l for l in lines if l]
    if not lines:
        return out

    def split_name(n):
        for i, ch in enumerate(n):
            if ch in " \t":
                return n[:i], n[i + 1:]
        return n, ""

    if data[:1] == ">":
        name, seq = None, ""
        for l in lines:
            if l.startswith(">"):
                if seq and name:
                    out.append(split_name(name) + (seq,))
                    seq = ""
                elif name:
                    return out
                name = l[1:]
            else:
                seq += l
        if seq and name:
            out.append(split_name(name) + (seq,))
    elif data[:1] == "@":
        i = 0
        while i + 4 <= len(lines):
            n, s, p, q = lines[i:i + 4]
            if not n.startswith("@") or not p.startswith("+") or len(q) != len(s):
                break
            if not (len(p) == 1 or p.endswith(n[1:])):
                break
            out.append(split_name(n[1:]) + (s,))
            i += 4
    return out


def _copy_records(ptr, n, dtype):
    """n records of `dtype` at the C pointer `ptr` -> an owned numpy array (ctypes.string_at stops at 2 GiB: one rank's shard
    of BASELINE configs[4] returns 27 M blocks of 80 bytes)"""
    out = np.empty(n, dtype=dtype)
    if n:
        C.memmove(out.ctypes.data, ptr, n * dtype.itemsize)
    return out


def _unitig_arrays(edges, lengths, seqs, offs):
    """The read set and records of a `unitigs*` call as the library takes them -> (edges, lengths, bases buffer, offs, n)."""
    edges = np.ascontiguousarray(edges, dtype=EDGE_DTYPE)
    lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    n = len(lengths)
    if len(offs) != n + 1:
        raise ValueError("offs must have len(lengths) + 1 entries")
    if isinstance(seqs, np.ndarray):
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
        buf = (C.c_char_p(seqs.ctypes.data) if seqs.size else b""), seqs  # (the array is kept alive with its pointer)
    else:
        buf = bytes(seqs), None
    return edges, lengths, buf, offs, n


def unitigs(edges, lengths, seqs, offs, min_overlap, device=0, bases=True):
    """Unbranched chains of overlaps compacted (sigax_unitigs_host, the rules in include/sigax.h): `edges` EDGE_DTYPE records
    of an overlap run, reads as lengths u32[n], bases `seqs` (bytes or uint8 array) and offs u64[n+1] by read id -> dict(
    seq_offs u64[U+1], lay_offs u64[U+1], uflags u32[U], layout PLACEMENT_DTYPE[n], useqs uint8 array (None with
    bases=False), status u64[6]).  Unitig u is useqs[seq_offs[u]:seq_offs[u+1]], its reads layout[lay_offs[u]:lay_offs[u+1]];
    uflags & SIGAX_UNITIG_CIRCULAR marks a cycle, uflags >> 1 is its closing overlap.  status = {unitigs, unitig bases,
    records ignored as malformed, records below min_overlap, simple records merged, cycles}.  Needs no index."""
    edges, lengths, buf, offs, n = _unitig_arrays(edges, lengths, seqs, offs)
    L = _lib.lib()
    nu = C.c_uint64()
    so, lo, uf, lay, us = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
    _check(L.sigax_unitigs_host(device, edges.ctypes.data if len(edges) else None, len(edges), lengths.ctypes.data if n else None, buf[0],
                                offs.ctypes.data, n, int(min_overlap), C.byref(nu), C.byref(so), C.byref(lo), C.byref(uf), C.byref(lay),
                                C.byref(us) if bases else None), "sigax_unitigs_host")
    try:
        u = int(nu.value)
        status = np.zeros(6, dtype=np.uint64)
        _check(L.sigax_unitigs_last_status(status.ctypes.data), "sigax_unitigs_last_status")
        out = {"seq_offs": _copy_records(so, u + 1, np.dtype(np.uint64)), "lay_offs": _copy_records(lo, u + 1, np.dtype(np.uint64)),
               "uflags": _copy_records(uf, u, np.dtype(np.uint32)), "layout": _copy_records(lay, n, PLACEMENT_DTYPE), "status": status}
        out["useqs"] = _copy_records(us, int(out["seq_offs"][-1]), np.dtype(np.uint8)) if bases else None
    finally:
        for p in (so, lo, uf, lay, us):
            L.sigax_free(p)
    return out


def _rounds_opts(level, n, max_rounds, min_branch_length, min_branch_coverage, delta=0, careful=False, num_reads=None, genome_size=None,
                 uniq_threshold=13.0, min_chimeric_length=0, min_chimeric_coverage=None, chimeric_delta=0, chimeric_threshold=0.0,
                 max_bubble_span=0, bubble_divergence=50, max_edits=0, edit_permille=50, reduce=False):
    """The options object of the rounds call `level` ("trim", "prune", "chimeric", "bubble", "indel" or "reduce") over n reads."""
    none = _lib.SIGAX_TRIM_NO_COVERAGE
    branch = (int(max_rounds), int(min_branch_length), none if min_branch_coverage is None else int(min_branch_coverage))
    if level == "trim":
        return _lib.TrimOpts(*branch, 0)
    opts = _lib.PruneOpts(*branch, int(delta), int(careful), 0, n if num_reads is None else int(num_reads),
                          0 if genome_size is None else int(genome_size), float(uniq_threshold))
    if level == "prune":
        return opts
    opts = _lib.ChimericOpts(opts, int(min_chimeric_length), none if min_chimeric_coverage is None else int(min_chimeric_coverage),
                             int(chimeric_delta), 0, float(chimeric_threshold))
    if level == "chimeric":
        return opts
    opts = _lib.BubbleOpts(opts, int(max_bubble_span), _lib.SIGAX_BUBBLE_NO_BASES if bubble_divergence is None else int(bubble_divergence),
                           (C.c_uint32 * 2)(0, 0))
    if level == "bubble":
        return opts
    opts = _lib.IndelOpts(opts, int(max_edits), int(edit_permille), (C.c_uint32 * 2)(0, 0))
    if level == "indel":
        return opts
    return _lib.ReduceOpts(opts, int(reduce), (C.c_uint32 * 3)(0, 0, 0))


def _unitigs_rounds(level, n_status, with_cut, edges, lengths, seqs, offs, min_overlap, graph, bases, device, **opt):
    """One rounds call through its host entry point sigax_unitigs_<level>_host: the arrays prepared, the options built from
    `opt`, the call, and its outputs copied into a dict (status u64[n_status]; cut only for a call that has one)."""
    edges, lengths, buf, offs, n = _unitig_arrays(edges, lengths, seqs, offs)
    L = _lib.lib()
    name = "sigax_unitigs_%s_host" % level
    opts = _rounds_opts(level, n, **opt)
    nu = C.c_uint64()
    so, lo, uf, lay, us, rm, ct, ue = (C.c_void_p() for _ in range(8))
    status = np.zeros(n_status, dtype=np.uint64)
    _check(getattr(L, name)(device, edges.ctypes.data if len(edges) else None, len(edges), lengths.ctypes.data if n else None, buf[0],
                            offs.ctypes.data, n, int(min_overlap), C.byref(opts), C.byref(nu), C.byref(so), C.byref(lo), C.byref(uf),
                            C.byref(lay), C.byref(us) if bases else None, C.byref(rm), *([C.byref(ct)] if with_cut else []),
                            C.byref(ue) if graph else None, status.ctypes.data), name)
    try:
        u = int(nu.value)
        out = {"seq_offs": _copy_records(so, u + 1, np.dtype(np.uint64)), "lay_offs": _copy_records(lo, u + 1, np.dtype(np.uint64)),
               "uflags": _copy_records(uf, u, np.dtype(np.uint32)), "status": status, "removed": _copy_records(rm, n, np.dtype(np.uint32))}
        if with_cut:
            out["cut"] = _copy_records(ct, len(edges), np.dtype(np.uint32))
        out["layout"] = _copy_records(lay, int(out["lay_offs"][-1]), PLACEMENT_DTYPE)
        out["useqs"] = _copy_records(us, int(out["seq_offs"][-1]), np.dtype(np.uint8)) if bases else None
        out["uedges"] = _copy_records(ue, int(status[11]), EDGE_DTYPE) if graph else None
    finally:
        for p in (so, lo, uf, lay, us, rm, ct, ue):
            L.sigax_free(p)
    return out


def unitigs_trim(edges, lengths, seqs, offs, min_overlap, max_rounds, min_branch_length, min_branch_coverage=None, graph=True, bases=True,
                 device=0):
    """`unitigs` after tip trimming, with the graph between the unitigs (sigax_unitigs_trim_host, the rules in include/sigax.h):
    up to max_rounds rounds (the reference's -x) remove every unitig that is a dead end or an island of at most
    min_branch_length bases (-n) and, unless min_branch_coverage (-C) is None, of low coverage.  -> the dict of `unitigs`
    (layout holds the kept reads only) plus removed u32[n] (0, or the round a read went in), uedges EDGE_DTYPE (the records
    that were not merged, over unitig ids and unitig ends; None with graph=False) and status u64[12]: the six counts of
    `unitigs`, then {rounds that removed something, islands, dead ends, reads removed, kept records dropped with a removed
    read, lifted records}.  max_rounds = 0 is `unitigs` itself."""
    return _unitigs_rounds("trim", 12, False, edges, lengths, seqs, offs, min_overlap, graph, bases, device, max_rounds=max_rounds,
                           min_branch_length=min_branch_length, min_branch_coverage=min_branch_coverage)


def unitigs_prune(edges, lengths, seqs, offs, min_overlap, max_rounds, min_branch_length, min_branch_coverage=None, delta=0, careful=False,
                  num_reads=None, genome_size=None, uniq_threshold=13.0, graph=True, bases=True, device=0):
    """`unitigs_trim` with non-maximal overlap cutting in every round (sigax_unitigs_prune_host, the rules in include/sigax.h):
    at a unitig that scores as unique under (num_reads N, genome_size G, uniq_threshold T) a record shorter by delta or more than
    the longest of its read end is cut before the round's trim step; with careful it stays where, seen from its other end, the
    unitig is among the longest.  delta = 0 is `unitigs_trim`.  num_reads=None: len(lengths).  -> the dict of `unitigs_trim` plus
    cut u32[n_edges] (0, or the round a record was cut in); status u64[16]: as there with 6 = rounds that changed something,
    then {records cut, rounds that cut, unique unitigs seen by the first cut step, 0}."""
    return _unitigs_rounds("prune", 16, True, edges, lengths, seqs, offs, min_overlap, graph, bases, device, max_rounds=max_rounds,
                           min_branch_length=min_branch_length, min_branch_coverage=min_branch_coverage, delta=delta, careful=careful,
                           num_reads=num_reads, genome_size=genome_size, uniq_threshold=uniq_threshold)


def unitigs_chimeric(edges, lengths, seqs, offs, min_overlap, max_rounds, min_branch_length, min_branch_coverage=None, delta=0, careful=False,
                     num_reads=None, genome_size=None, uniq_threshold=13.0, min_chimeric_length=0, min_chimeric_coverage=None,
                     chimeric_delta=0, chimeric_threshold=0.0, graph=True, bases=True, device=0):
    """`unitigs_prune` with chimeric unitig removal as the last step of every round (sigax_unitigs_chimeric_host, the rules in
    include/sigax.h): a unitig of at most min_chimeric_length bases (and, unless min_chimeric_coverage is None, of low coverage)
    with one participant record at each end, both leading to branched read ends, goes where one of the two neighbours scores as
    unique under chimeric_threshold and every other unitig at that end is longer by more than chimeric_delta, or holds more than
    three reads more.  min_chimeric_length = 0 is `unitigs_prune`.  -> its dict; removed carries _lib.SIGAX_REMOVED_CHIMERIC on
    the reads a chimeric step removed; status u64[20]: as there, then {chimeric unitigs, their reads, rounds with one, 0}."""
    return _unitigs_rounds("chimeric", 20, True, edges, lengths, seqs, offs, min_overlap, graph, bases, device, max_rounds=max_rounds,
                           min_branch_length=min_branch_length, min_branch_coverage=min_branch_coverage, delta=delta, careful=careful,
                           num_reads=num_reads, genome_size=genome_size, uniq_threshold=uniq_threshold, min_chimeric_length=min_chimeric_length,
                           min_chimeric_coverage=min_chimeric_coverage, chimeric_delta=chimeric_delta, chimeric_threshold=chimeric_threshold)


def unitigs_bubble(edges, lengths, seqs, offs, min_overlap, max_rounds, min_branch_length, min_branch_coverage=None, delta=0, careful=False,
                   num_reads=None, genome_size=None, uniq_threshold=13.0, min_chimeric_length=0, min_chimeric_coverage=None,
                   chimeric_delta=0, chimeric_threshold=0.0, max_bubble_span=0, bubble_divergence=50, graph=True, bases=True, device=0):
    """`unitigs_chimeric` with bubble popping between the trim and the chimeric step of every round (sigax_unitigs_bubble_host, the
    rules in include/sigax.h): of the unitigs that join the same two read ends through one participant record at each end and hold
    the same number of bases between them, at most max_bubble_span, the one with the most reads (then the smallest first read) stays;
    another goes where its bases differ from the winner's in at most bubble_divergence per mille of that window (None: no bases
    test).  max_bubble_span = 0 is `unitigs_chimeric`.  -> its dict; removed carries _lib.SIGAX_REMOVED_BUBBLE on the reads a bubble
    step removed; status u64[24]: as there, then {arms popped, their reads, rounds with one, losers kept on divergence}."""
    return _unitigs_rounds("bubble", 24, True, edges, lengths, seqs, offs, min_overlap, graph, bases, device, max_rounds=max_rounds,
                           min_branch_length=min_branch_length, min_branch_coverage=min_branch_coverage, delta=delta, careful=careful,
                           num_reads=num_reads, genome_size=genome_size, uniq_threshold=uniq_threshold, min_chimeric_length=min_chimeric_length,
                           min_chimeric_coverage=min_chimeric_coverage, chimeric_delta=chimeric_delta, chimeric_threshold=chimeric_threshold,
                           max_bubble_span=max_bubble_span, bubble_divergence=bubble_divergence)


def unitigs_indel(edges, lengths, seqs, offs, min_overlap, max_rounds, min_branch_length, min_branch_coverage=None, delta=0, careful=False,
                  num_reads=None, genome_size=None, uniq_threshold=13.0, min_chimeric_length=0, min_chimeric_coverage=None,
                  chimeric_delta=0, chimeric_threshold=0.0, max_bubble_span=0, bubble_divergence=50, max_edits=0, edit_permille=50,
                  graph=True, bases=True, device=0):
    """`unitigs_bubble` with indel bubble popping between the bubble and the chimeric step of every round (sigax_unitigs_indel_host, the
    rules in include/sigax.h): the unitigs that join the same two read ends through one participant record at each end and hold 1 to
    max_bubble_span bases between them form one group whatever those spans; the one with the most reads (then the smallest first read)
    stays.  Another whose span differs from the winner's by 1 to max_edits goes where the edit distance ed between the two windows
    (unit cost, bytes as bytes, exact up to max_edits) is at most max_edits and ed * 1000 <= edit_permille * the bases of the shorter
    of the two unitigs.  One of the winner's span is the bubble step's business and stays.  max_edits = 0 is `unitigs_bubble`; with
    max_edits > 0 (at most 31) max_bubble_span must be 1 to 4096.  -> its dict; removed carries _lib.SIGAX_REMOVED_INDEL on the reads
    an indel step removed; status u64[32]: as there, then {arms popped, their reads, rounds with one, compared losers kept, losers
    not compared, 0, 0, 0} (_lib.INDEL_STATUS)."""
    return _unitigs_rounds("indel", 32, True, edges, lengths, seqs, offs, min_overlap, graph, bases, device, max_rounds=max_rounds,
                           min_branch_length=min_branch_length, min_branch_coverage=min_branch_coverage, delta=delta, careful=careful,
                           num_reads=num_reads, genome_size=genome_size, uniq_threshold=uniq_threshold, min_chimeric_length=min_chimeric_length,
                           min_chimeric_coverage=min_chimeric_coverage, chimeric_delta=chimeric_delta, chimeric_threshold=chimeric_threshold,
                           max_bubble_span=max_bubble_span, bubble_divergence=bubble_divergence, max_edits=max_edits, edit_permille=edit_permille)


def unitigs_reduce(edges, lengths, seqs, offs, min_overlap, max_rounds, min_branch_length, min_branch_coverage=None, delta=0, careful=False,
                   num_reads=None, genome_size=None, uniq_threshold=13.0, min_chimeric_length=0, min_chimeric_coverage=None,
                   chimeric_delta=0, chimeric_threshold=0.0, max_bubble_span=0, bubble_divergence=50, max_edits=0, edit_permille=50,
                   reduce=True, graph=True, bases=True, device=0):
    """`unitigs_indel` with a transitive reduction pass as the first step of every round and once more before the final unitigs
    (sigax_unitigs_reduce_host, the rules in include/sigax.h): a record between read ends a and b that is neither a containment nor a
    self edge is flagged where records a-w and (w ^ 1)-b through a third read exist whose extensions add up to its own, exactly.  A
    flagged record is not there for any step, for the unitigs or for uedges; every pass clears the flags and sets them anew over what
    is alive, so a record whose witness a round removed comes back.  With max_rounds = 0 it is "reduce, then `unitigs`": the way to
    turn exhaustive overlap records into a string graph.  reduce=False is `unitigs_indel`.  -> its dict; cut carries
    _lib.SIGAX_CUT_TRANSITIVE (bit 31) on the records flagged in the final graph, the low bits the round of a `delta` cut as before;
    status u64[40]: as there, then {records flagged by the first pass, records flagged in the final graph, passes that ran,
    participants of the last pass, 0, 0, 0, 0} (_lib.REDUCE_STATUS)."""
    return _unitigs_rounds("reduce", 40, True, edges, lengths, seqs, offs, min_overlap, graph, bases, device, max_rounds=max_rounds,
                           min_branch_length=min_branch_length, min_branch_coverage=min_branch_coverage, delta=delta, careful=careful,
                           num_reads=num_reads, genome_size=genome_size, uniq_threshold=uniq_threshold, min_chimeric_length=min_chimeric_length,
                           min_chimeric_coverage=min_chimeric_coverage, chimeric_delta=chimeric_delta, chimeric_threshold=chimeric_threshold,
                           max_bubble_span=max_bubble_span, bubble_divergence=bubble_divergence, max_edits=max_edits, edit_permille=edit_permille,
                           reduce=reduce)


def mates_by_name(names):
    """The mate of every read by name, as the reference's PairEnd::id finds it (src/reads.cpp:19-41): the mate's name is the
    read's with its last character swapped 1<->2, A<->B or f<->r.  -> u32[n]; SIGAX_NO_MATE where the name ends otherwise, the
    mate's name is absent, or either of the two names occurs more than once."""
    swap = {"1": "2", "2": "1", "A": "B", "B": "A", "f": "r", "r": "f"}
    ns = [n.decode("latin-1") if isinstance(n, (bytes, bytearray)) else str(n) for n in names]
    seen = {}
    for i, n in enumerate(ns):
        seen[n] = i if n not in seen else -1  # -1: more than once
    mate = np.full(len(ns), _lib.SIGAX_NO_MATE, dtype=np.uint32)
    for i, n in enumerate(ns):
        if n and n[-1] in swap and seen[n] == i:
            j = seen.get(n[:-1] + swap[n[-1]], -1)
            if j >= 0:
                mate[i] = j
    return mate


def pairs_estimate(status):
    """sigax_pairs_estimate over a status24 -> (insert_size, delta, span_mean, span_sd)."""
    status = np.ascontiguousarray(status, dtype=np.uint64)
    if len(status) != 24:
        raise ValueError("status must have 24 entries")
    ins, dl, sm, sd = C.c_uint64(), C.c_uint64(), C.c_double(), C.c_double()
    _check(_lib.lib().sigax_pairs_estimate(status.ctypes.data, C.byref(ins), C.byref(dl), C.byref(sm), C.byref(sd)), "sigax_pairs_estimate")
    return int(ins.value), int(dl.value), float(sm.value), float(sd.value)


def unitigs_consensus(res, lengths, seqs, offs, min_votes=1, support=False, device=0):
    """The consensus pass (sigax_consensus_host, the rules in include/sigax.h) over the dict `res` any `unitigs*` call returned
    with its bases, and the reads that call was given: every unitig column by majority vote over the reads the layout lays over
    it -> dict(useqs uint8 array, changed u32[U] columns replaced per unitig, support u8 array (votes for the byte a column
    holds, at most 255) or None, status u64[8] (named by _lib.CONSENSUS_STATUS)).  `res` is not modified."""
    _, lengths, buf, offs, n = _unitig_arrays(np.zeros(0, dtype=EDGE_DTYPE), lengths, seqs, offs)
    if res.get("useqs") is None:
        raise ValueError("the unitig call's bases are needed (bases=True)")
    so = np.ascontiguousarray(res["seq_offs"], dtype=np.uint64)
    lo = np.ascontiguousarray(res["lay_offs"], dtype=np.uint64)
    lay = np.ascontiguousarray(res["layout"], dtype=PLACEMENT_DTYPE)
    u = len(so) - 1
    if u < 0 or len(lo) != u + 1:
        raise ValueError("seq_offs and lay_offs must have one entry more than there are unitigs")
    if len(lay) < int(lo[u]):
        raise ValueError("layout shorter than lay_offs says")
    us = np.array(res["useqs"], dtype=np.uint8)  # (a copy: the call rewrites it in place)
    if len(us) < int(so[u]):
        raise ValueError("useqs shorter than seq_offs says")
    L = _lib.lib()
    opts = _lib.ConsensusOpts(int(min_votes), (0, 0, 0))
    cp, sp = C.c_void_p(), C.c_void_p()
    status = np.zeros(8, dtype=np.uint64)
    _check(L.sigax_consensus_host(device, u, so.ctypes.data, lo.ctypes.data, lay.ctypes.data if len(lay) else None,
                                  lengths.ctypes.data if n else None, buf[0], offs.ctypes.data, n, C.byref(opts),
                                  us.ctypes.data if len(us) else None, C.byref(cp), C.byref(sp) if support else None, status.ctypes.data),
           "sigax_consensus_host")
    try:
        out = {"useqs": us, "changed": _copy_records(cp, u, np.dtype(np.uint32)),
               "support": _copy_records(sp, int(so[u]), np.dtype(np.uint8)) if support else None, "status": status}
    finally:
        L.sigax_free(cp)
        L.sigax_free(sp)
    return out


def unitigs_place_contained(res, lengths, contained, containments, device=0):
    """Contained reads placed in a unitig call's layout (sigax_contained_place_host, the rules in include/sigax.h) over the dict
    `res` any `unitigs*` call returned: lengths u32[n], contained u8[n] and the containment records (_lib.MM_EDGE_DTYPE) of
    `FMIndexPair.overlap_mismatch(..., containments=True)` -> a copy of `res` whose lay_offs and layout hold the placed contained
    reads too (flags | _lib.PLACED_CONTAINED), ready for `unitigs_consensus` and `unitigs_pairs`, with place_class u8[n]
    (_lib.CP_CLASSES) and place_status u64[8] (_lib.CONTAINED_STATUS) beside them.  `res` is not modified."""
    lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
    contained = np.ascontiguousarray(contained, dtype=np.uint8)
    recs = np.ascontiguousarray(containments, dtype=_lib.MM_EDGE_DTYPE)
    n = len(lengths)
    if len(contained) != n:
        raise ValueError("contained must have one entry per read")
    so = np.ascontiguousarray(res["seq_offs"], dtype=np.uint64)
    lo = np.ascontiguousarray(res["lay_offs"], dtype=np.uint64)
    lay = np.ascontiguousarray(res["layout"], dtype=PLACEMENT_DTYPE)
    u = len(so) - 1
    if u < 0 or len(lo) != u + 1:
        raise ValueError("seq_offs and lay_offs must have one entry more than there are unitigs")
    if len(lay) < int(lo[u]):
        raise ValueError("layout shorter than lay_offs says")
    L = _lib.lib()
    opts = _lib.ContainedOpts()
    lo2, lay2, cls = C.c_void_p(), C.c_void_p(), C.c_void_p()
    status = np.zeros(8, dtype=np.uint64)
    _check(L.sigax_contained_place_host(device, u, so.ctypes.data, lo.ctypes.data, lay.ctypes.data if len(lay) else None,
                                        lengths.ctypes.data if n else None, n, contained.ctypes.data if n else None,
                                        recs.ctypes.data if len(recs) else None, len(recs), C.byref(opts), C.byref(lo2), C.byref(lay2), C.byref(cls),
                                        status.ctypes.data), "sigax_contained_place_host")
    try:
        out = dict(res)
        out["lay_offs"] = _copy_records(lo2, u + 1, np.dtype(np.uint64))
        out["layout"] = _copy_records(lay2, int(status[7]), PLACEMENT_DTYPE)
        out["place_class"] = _copy_records(cls, n, np.dtype(np.uint8))
        out["place_status"] = status
    finally:
        L.sigax_free(lo2)
        L.sigax_free(lay2)
        L.sigax_free(cls)
    return out


def unitigs_pairs(res, lengths, mate, hist_bins=1024, hist_shift=0, max_span=0, outward=False, device=0):
    """Mate-pair statistics and the links between unitig ends (sigax_unitigs_pairs_host, the rules in include/sigax.h) over the
    dict `res` any `unitigs*` call returned: lengths u32[n], mate u32[n] (`mates_by_name`; SIGAX_NO_MATE = none) -> dict(status
    u64[24] (named by _lib.PAIRS_STATUS), hist u64[hist_bins] of span >> hist_shift over the same-unitig pairs of the library's
    orientation, links PAIR_LINK_DTYPE records ascending by (a, b) with a = 2 * unitig + end (0 = B, 1 = E), insert_size,
    delta, span_mean, span_sd)."""
    lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
    mate = np.ascontiguousarray(mate, dtype=np.uint32)
    n = len(lengths)
    if len(mate) != n:
        raise ValueError("mate must have len(lengths) entries")
    so = np.ascontiguousarray(res["seq_offs"], dtype=np.uint64)
    lo = np.ascontiguousarray(res["lay_offs"], dtype=np.uint64)
    uf = np.ascontiguousarray(res["uflags"], dtype=np.uint32)
    lay = np.ascontiguousarray(res["layout"], dtype=PLACEMENT_DTYPE)
    u = len(uf)
    if len(so) != u + 1 or len(lo) != u + 1:
        raise ValueError("seq_offs and lay_offs must have len(uflags) + 1 entries")
    if len(lay) < int(lo[u]):
        raise ValueError("layout shorter than lay_offs says")
    L = _lib.lib()
    opts = _lib.PairsOpts(_lib.SIGAX_PAIRS_OUTWARD if outward else 0, int(hist_bins), int(hist_shift), 0, int(max_span))
    hp, lp = C.c_void_p(), C.c_void_p()
    status = np.zeros(24, dtype=np.uint64)
    _check(L.sigax_unitigs_pairs_host(device, mate.ctypes.data if n else None, lengths.ctypes.data if n else None, n, u, so.ctypes.data,
                                      lo.ctypes.data, uf.ctypes.data if u else None, lay.ctypes.data if len(lay) else None, C.byref(opts),
                                      C.byref(hp), C.byref(lp), status.ctypes.data), "sigax_unitigs_pairs_host")
    try:
        out = {"status": status, "hist": _copy_records(hp, int(hist_bins), np.dtype(np.uint64)),
               "links": _copy_records(lp, int(status[22]), _lib.PAIR_LINK_DTYPE)}
    finally:
        L.sigax_free(hp)
        L.sigax_free(lp)
    out["insert_size"], out["delta"], out["span_mean"], out["span_sd"] = pairs_estimate(status)
    return out


def unitigs_scaffold(res, links, insert_size=None, status=None, min_pairs=2, link_ratio=0, min_unitig_bases=0, min_gap=1, max_gap=1000000,
                     bases=True, device=0):
    """Unitigs joined into scaffolds through the link records of `unitigs_pairs` (sigax_scaffold_host, the rules in
    include/sigax.h): `res` is the dict any `unitigs*` call returned (seq_offs, uflags and, with bases, useqs), `links` and
    `status` the links and status of `unitigs_pairs` over it.  insert_size=None takes floor(status[15] / status[14]), the mean
    span of the library's pairs inside a unitig.  A link of at least min_pairs pairs between unitigs of at least
    min_unitig_bases bases that is the only strong one at both its ends joins them; link_ratio > 0 sets aside the links with
    count * link_ratio <= the largest count at either end.  -> dict(sc_offs u64[S + 1], sc_lay_offs u64[S + 1], sc_flags u32[S]
    (bit 0: a cycle, flags >> 1 its closing gap), layout PLACEMENT_DTYPE[unitigs] (read = the unitig), seqs u8 (None without
    bases: N in the gaps), status u64[16] named by _lib.SCAFFOLD_STATUS)."""
    so = np.ascontiguousarray(res["seq_offs"], dtype=np.uint64)
    uf = np.ascontiguousarray(res["uflags"], dtype=np.uint32)
    links = np.ascontiguousarray(links, dtype=_lib.PAIR_LINK_DTYPE)
    u = len(uf)
    if len(so) != u + 1:
        raise ValueError("seq_offs must have len(uflags) + 1 entries")
    us = None
    if bases:
        if res.get("useqs") is None:
            raise ValueError("bases=True needs the unitig bases (res['useqs'])")
        us = res["useqs"]
        us = np.frombuffer(bytes(us), dtype=np.uint8) if isinstance(us, (bytes, bytearray)) else np.ascontiguousarray(us, dtype=np.uint8)
        if len(us) < int(so[u]):
            raise ValueError("useqs shorter than seq_offs says")
    flags = 0
    if insert_size is None:
        if status is None:
            raise ValueError("insert_size=None needs the status of unitigs_pairs")
        flags = _lib.SIGAX_SCAFFOLD_INSERT_FROM_STATUS
    st24 = None
    if status is not None:
        st24 = np.ascontiguousarray(status, dtype=np.uint64)
        if len(st24) != 24:
            raise ValueError("status must have 24 entries")
    L = _lib.lib()
    opts = _lib.ScaffoldOpts(flags, int(min_pairs), int(link_ratio), int(min_unitig_bases), 0 if insert_size is None else int(insert_size),
                             int(min_gap), int(max_gap))
    ns = C.c_uint64()
    po, pl, pf, play, ps = (C.c_void_p() for _ in range(5))
    st16 = np.zeros(16, dtype=np.uint64)
    _check(L.sigax_scaffold_host(device, u, so.ctypes.data, uf.ctypes.data if u else None, us.ctypes.data if bases and len(us) else None,
                                 links.ctypes.data if len(links) else None, len(links), None if st24 is None else st24.ctypes.data,
                                 C.byref(opts), C.byref(ns), C.byref(po), C.byref(pl), C.byref(pf), C.byref(play),
                                 C.byref(ps) if bases else None, st16.ctypes.data), "sigax_scaffold_host")
    try:
        s = int(ns.value)
        out = {"sc_offs": _copy_records(po, s + 1, np.dtype(np.uint64)), "sc_lay_offs": _copy_records(pl, s + 1, np.dtype(np.uint64)),
               "sc_flags": _copy_records(pf, s, np.dtype(np.uint32)), "layout": _copy_records(play, u, PLACEMENT_DTYPE), "status": st16}
        out["seqs"] = _copy_records(ps, int(st16[1]), np.dtype(np.uint8)) if bases else None
    finally:
        for p in (po, pl, pf, play, ps):
            L.sigax_free(p)
    return out


def scaffolds_gapfill(pair, res, scaf, k=31, min_count=3, slack=100, max_fill=10000, max_walk_bases=None, bases=True):
    """The gaps of `unitigs_scaffold`'s scaffolds closed by k-mer walks over the reads' index (sigax_gapfill_host, the rules in
    include/sigax.h): `pair` is the FMIndexPair of the reads (the forward strand is enough), `res` the dict of the unitig call
    (seq_offs, useqs), `scaf` the dict `unitigs_scaffold` returned over it.  A gap is filled when the walk from the left unitig's
    last k-mer, taking the one next base that at least min_count reads (either strand) support, arrives at the right unitig's first
    k-mer within slack bases of the laid gap -- or the walk back from the right unitig does; gaps laid wider than max_fill are not
    tried.  max_walk_bases=None sizes the walk scratch so that every gap has room.  -> the dict shape of `unitigs_scaffold`
    (sc_lay_offs and sc_flags as they came in, status u64[24] named by _lib.GAPFILL_STATUS) plus gaps, one _lib.GAP_DTYPE record
    per gap in scaffold order: its class (_lib.GAP_CLASSES), the two walks' outcomes, the fill and where it starts."""
    so = np.ascontiguousarray(res["seq_offs"], dtype=np.uint64)
    u = len(so) - 1
    if res.get("useqs") is None:
        raise ValueError("the walks start from the unitig bases (res['useqs'])")
    us = res["useqs"]
    us = np.frombuffer(bytes(us), dtype=np.uint8) if isinstance(us, (bytes, bytearray)) else np.ascontiguousarray(us, dtype=np.uint8)
    if len(us) < int(so[u]):
        raise ValueError("useqs shorter than seq_offs says")
    slo = np.ascontiguousarray(scaf["sc_lay_offs"], dtype=np.uint64)
    lay = np.ascontiguousarray(scaf["layout"], dtype=PLACEMENT_DTYPE)
    s = len(slo) - 1
    if s < 0 or len(lay) < int(slo[s]):
        raise ValueError("layout shorter than sc_lay_offs says")
    L = _lib.lib()
    opts = _lib.GapfillOpts(0, int(k), int(min_count), int(slack), int(max_fill), 0)
    po, play, ps, pg = (C.c_void_p() for _ in range(4))
    ng = C.c_uint64()
    st = np.zeros(24, dtype=np.uint64)
    _check(L.sigax_gapfill_host(pair.handle, u, so.ctypes.data, us.ctypes.data if len(us) else None, s, slo.ctypes.data,
                                lay.ctypes.data if len(lay) else None, C.byref(opts),
                                _lib.SIGAX_GAPFILL_AUTO if max_walk_bases is None else int(max_walk_bases), C.byref(po), C.byref(play),
                                C.byref(ps) if bases else None, C.byref(pg), C.byref(ng), st.ctypes.data), "sigax_gapfill_host")
    try:
        out = {"sc_offs": _copy_records(po, s + 1, np.dtype(np.uint64)), "sc_lay_offs": slo.copy(),
               "sc_flags": np.array(scaf["sc_flags"], dtype=np.uint32), "layout": _copy_records(play, int(slo[s]) if u else 0, PLACEMENT_DTYPE),
               "status": st, "gaps": _copy_records(pg, int(ng.value), _lib.GAP_DTYPE)}
        out["seqs"] = _copy_records(ps, int(st[16]), np.dtype(np.uint8)) if bases else None
    finally:
        for p in (po, play, ps, pg):
            L.sigax_free(p)
    return out


def scaffolds_join(pair, res, scaf, min_overlap=16, max_overlap=1000, slack=100, k=31, min_count=3, bases=True, max_mismatches=0, mismatch_permille=50):
    """Neighbours of a scaffold that overlap written as one sequence (sigax_join_host, the rules in include/sigax.h): `pair` is
    the FMIndexPair of the reads (the forward strand is enough), `res` the dict of the unitig call (seq_offs, for the unitigs'
    lengths), `scaf` the dict `unitigs_scaffold` or `scaffolds_gapfill` returned over it, with its bases.  A gap of at most slack
    N is joined when exactly one length v in min_overlap .. max_overlap makes the left neighbour's last v bases the right
    neighbour's first v and every k-mer across the junction occurs min_count times in the reads (either strand); the N and one
    copy of the overlap then go.  -> the dict shape of `unitigs_scaffold` (sc_lay_offs and sc_flags as they came in, status
    u64[16] named by _lib.JOIN_STATUS) plus joins, one _lib.JOIN_DTYPE record per gap in scaffold order: its class
    (_lib.JOIN_CLASSES), the overlap, how many lengths matched, the junction windows looked up and where the gap lies now.
    max_mismatches > 0 (sigax_join_approx_host): where no length matches exactly, the one length whose ends differ in at most
    min(max_mismatches, v * mismatch_permille / 1000) bases is taken, each differing base settled by the reads; the dict gains
    "mm" (u32 per gap: mismatches | columns taken from the right << 8 | _lib.JOIN_MM_APPROX) and status is u64[24]
    (_lib.JOIN_APPROX_STATUS)."""
    so = np.ascontiguousarray(res["seq_offs"], dtype=np.uint64)
    u = len(so) - 1
    sco = np.ascontiguousarray(scaf["sc_offs"], dtype=np.uint64)
    slo = np.ascontiguousarray(scaf["sc_lay_offs"], dtype=np.uint64)
    lay = np.ascontiguousarray(scaf["layout"], dtype=PLACEMENT_DTYPE)
    s = len(slo) - 1
    if s < 0 or len(sco) != s + 1 or len(lay) < int(slo[s]):
        raise ValueError("sc_offs, sc_lay_offs and layout do not fit each other")
    if scaf.get("seqs") is None:
        raise ValueError("the overlaps are looked for in the scaffold bases (scaf['seqs'])")
    sq = scaf["seqs"]
    sq = np.frombuffer(bytes(sq), dtype=np.uint8) if isinstance(sq, (bytes, bytearray)) else np.ascontiguousarray(sq, dtype=np.uint8)
    if len(sq) < int(sco[s]):
        raise ValueError("seqs shorter than sc_offs says")
    L = _lib.lib()
    approx = int(max_mismatches) > 0
    po, play, ps, pj, pm = (C.c_void_p() for _ in range(5))
    nj = C.c_uint64()
    st = np.zeros(24 if approx else 16, dtype=np.uint64)
    tables = (pair.handle, u, so.ctypes.data, s, sco.ctypes.data, slo.ctypes.data, lay.ctypes.data if len(lay) else None,
              sq.ctypes.data if len(sq) else None)
    outs = (C.byref(po), C.byref(play), C.byref(ps) if bases else None, C.byref(pj), C.byref(nj))
    if approx:
        opts = _lib.JoinApproxOpts(0, int(min_overlap), int(max_overlap), int(slack), int(k), int(min_count), int(max_mismatches),
                                   int(mismatch_permille), 0)
        _check(L.sigax_join_approx_host(*tables, C.byref(opts), *outs, C.byref(pm), st.ctypes.data), "sigax_join_approx_host")
    else:
        opts = _lib.JoinOpts(0, int(min_overlap), int(max_overlap), int(slack), int(k), int(min_count), 0)
        _check(L.sigax_join_host(*tables, C.byref(opts), *outs, st.ctypes.data), "sigax_join_host")
    try:
        out = {"sc_offs": _copy_records(po, s + 1, np.dtype(np.uint64)), "sc_lay_offs": slo.copy(),
               "sc_flags": np.array(scaf["sc_flags"], dtype=np.uint32), "layout": _copy_records(play, int(slo[s]) if u else 0, PLACEMENT_DTYPE),
               "status": st, "joins": _copy_records(pj, int(nj.value), _lib.JOIN_DTYPE)}
        out["seqs"] = _copy_records(ps, int(st[11]), np.dtype(np.uint8)) if bases else None
        if approx:
            out["mm"] = _copy_records(pm, int(nj.value), np.dtype(np.uint32))
    finally:
        for p in (po, play, ps, pj, pm):
            L.sigax_free(p)
    return out


class ShardedResult(tuple):
    """What OverlapBuilder.overlap_sharded returns: the pair (edges, substring), which also answers to those two names as
    the result of `overlap` does -- `format_asqg` takes it as it is."""

    def __new__(cls, edges, substring):
        return super().__new__(cls, (edges, substring))

    def __getitem__(self, key):
        if isinstance(key, str):
            return super().__getitem__(("edges", "substring").index(key))
        return super().__getitem__(key)


class _DeviceBytes:
    """device memory through the HIP runtime libsigax.so is bound to (the process may hold a second one, PyTorch's own)"""

    def __init__(self, nbytes, device):
        hip = _lib.lib()
        hip.hipSetDevice.argtypes = [C.c_int]
        hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        hip.hipFree.argtypes = [C.c_void_p]
        self._hip = hip
        self.nbytes = int(nbytes)
        self.ptr = C.c_void_p()
        self._try(hip.hipSetDevice(device), "hipSetDevice")
        self._try(hip.hipMalloc(C.byref(self.ptr), max(self.nbytes, 16)), "hipMalloc")

    def _try(self, err, where):
        if err != 0:
            raise RuntimeError("%s failed: HIP error %d" % (where, err))

    def at(self, offset):
        return C.c_void_p(self.ptr.value + offset)

    def upload(self, arr):
        if arr.nbytes:
            self._try(self._hip.hipMemcpy(self.ptr, arr.ctypes.data, arr.nbytes, 1), "hipMemcpy")  # host to device
        return self

    def zero(self):
        self._try(self._hip.hipMemset(self.ptr, 0, max(self.nbytes, 16)), "hipMemset")
        return self

    def copy_from_device(self, offset, src, nbytes):
        if nbytes:
            self._try(self._hip.hipMemcpy(self.at(offset), src, nbytes, 3), "hipMemcpy")  # device to device

    def download(self, dtype, count):
        out = np.empty(count, dtype=dtype)
        if out.nbytes:
            self._try(self._hip.hipMemcpy(out.ctypes.data, self.ptr, out.nbytes, 2), "hipMemcpy")  # device to host
        return out

    def free(self):
        if self.ptr:
            self._hip.hipFree(self.ptr)
            self.ptr = C.c_void_p()


class FMIndexPair:
    """Both FM-indexes (+ .sai tables) resident on one GPU."""

    def __init__(self, handle):
        self._h = C.c_void_p(handle)

    @classmethod
    def load(cls, prefix, device=0, with_sai=True, resident=True):
        """resident: the index stays open for many more reads than it holds (tests, bench.py): sigax_index_prepare builds the
        extractor's row tables at once.  False = what one pass of `siga overlap` does: tables only after a full pass."""
        h = C.c_void_p()
        sai = (prefix + ".sai").encode() if with_sai else None
        rsai = (prefix + ".rsai").encode() if with_sai else None
        _check(_lib.lib().sigax_index_open((prefix + ".bwt").encode(), (prefix + ".rbwt").encode(), sai, rsai,
                                           device, C.byref(h)), "sigax_index_open")
        pair = cls(h.value)
        pair._prepare_pending = bool(resident)  # at set_reads() (the longest read is known then) or the first batch
        pair._resident = bool(resident)
        return pair

    @classmethod
    def load_forward(cls, prefix, device=0, with_sai=True):
        """<prefix>.bwt alone (what `siga index --no-reverse` writes), with <prefix>.sai unless with_sai is False: serves occ,
        kmer_counts, correct, match, kmer_spectrum and -- with the .sai table -- locate; overlap runs fail on it."""
        h = C.c_void_p()
        sai = (prefix + ".sai").encode() if with_sai else None
        _check(_lib.lib().sigax_index_open((prefix + ".bwt").encode(), None, sai, None, device, C.byref(h)), "sigax_index_open")
        pair = cls(h.value)
        pair._prepare_pending = False
        pair._resident = False
        return pair

    @classmethod
    def from_memory(cls, runs, rruns, n_symbols, n_strings, sai=None, rsai=None, device=0, resident=True):
        runs = np.ascontiguousarray(runs, dtype=np.uint8)
        rruns = np.ascontiguousarray(rruns, dtype=np.uint8)
        h = C.c_void_p()
        ps = pr = None
        if sai is not None:
            sai = np.ascontiguousarray(sai, dtype=np.uint32)
            rsai = np.ascontiguousarray(rsai, dtype=np.uint32)
            ps, pr = sai.ctypes.data, rsai.ctypes.data
        _check(_lib.lib().sigax_index_open_mem(runs.ctypes.data, len(runs), rruns.ctypes.data, len(rruns), n_symbols,
                                               n_strings, ps, pr, device, C.byref(h)), "sigax_index_open_mem")
        pair = cls(h.value)
        pair._prepare_pending = bool(resident)  # at set_reads() (the longest read is known then) or the first batch
        pair._resident = bool(resident)
        return pair

    def close(self):
        if self._h:
            if getattr(self, "_pile_ref", None) is not None:
                _lib.lib().sigax_pile_ref_destroy(self._pile_ref)
                self._pile_ref = None
            _lib.lib().sigax_index_close(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def info(self):
        inf = _lib.IndexInfo()
        _check(_lib.lib().sigax_index_info_get(self._h, C.byref(inf)), "sigax_index_info_get")
        return {"n_symbols": inf.n_symbols, "n_strings": inf.n_strings, "device_bytes": inf.device_bytes,
                "pred": list(inf.pred), "device": inf.device, "wide": inf.wide}

    def set_reads(self, lengths, ranks):
        lengths = np.ascontiguousarray(lengths, dtype=np.uint32)
        ranks = np.ascontiguousarray(ranks, dtype=np.uint32)
        _check(_lib.lib().sigax_index_set_reads(self._h, lengths.ctypes.data, ranks.ctypes.data, len(lengths)),
               "sigax_index_set_reads")
        if getattr(self, "_prepare_pending", False):
            self.prepare()

    def prepare(self):
        """sigax_index_prepare: the extractor's row tables in place now"""
        self._prepare_pending = False
        _check(_lib.lib().sigax_index_prepare(self._h), "sigax_index_prepare")

    def prepare_overlap(self, min_overlap):
        """sigax_index_prepare_overlap: row tables + the block finder's deep start table for this minimum overlap"""
        self._prepare_pending = False
        self._deep_for = min(getattr(self, "_deep_for", 1 << 30), int(min_overlap))
        _check(_lib.lib().sigax_index_prepare_overlap(self._h, int(min_overlap)), "sigax_index_prepare_overlap")

    def check_order(self, which=0):
        """sigax_index_check_order: (pairs of adjacent BWT rows out of suffix order, first such row, undecided pairs)"""
        bad, first, und = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(_lib.lib().sigax_index_check_order(self._h, which, C.byref(bad), C.byref(first), C.byref(und)), "sigax_index_check_order")
        return int(bad.value), int(first.value), int(und.value)

    def occ(self, positions, which=0):
        """FMIndex::getOcc for many positions -> [n,5] ($,A,C,G,T)."""
        pos = np.ascontiguousarray(positions, dtype=np.uint64)
        out = np.zeros((len(pos), 5), dtype=np.uint64)
        _check(_lib.lib().sigax_occ_batch(self._h, which, pos.ctypes.data, len(pos), out.ctypes.data), "sigax_occ_batch")
        return out

    def kmer_counts(self, kmers):
        k = len(kmers[0])
        buf = b"".join(x.encode() if isinstance(x, str) else x for x in kmers)
        out = np.zeros(len(kmers), dtype=np.uint64)
        _check(_lib.lib().sigax_kmer_count_batch(self._h, buf, k, len(kmers), out.ctypes.data), "sigax_kmer_count_batch")
        return out

    def match(self, seqs, max_length=None, rc=True):
        """`siga match` for a batch (src/match.cpp:54-62, sigax_match_batch) -> (head, tail), numpy u64 each: head[r] = the
        number of read r's `VT 0` line; tail = a masked array, its `VT 1` number where the read is split (longer than
        max_length), masked elsewhere.  max_length None: no read is split."""
        buf, offs = pack_reads(seqs)
        n = len(offs) - 1
        out = np.zeros(2 * n, dtype=np.uint64)
        if isinstance(buf, np.ndarray):
            buf = C.c_char_p(buf.ctypes.data) if buf.size else b""
        lim = MATCH_NONE if max_length is None else int(max_length)
        _check(_lib.lib().sigax_match_batch(self._h, buf, offs.ctypes.data, n, lim, SIGAX_RC if rc else 0, out.ctypes.data),
               "sigax_match_batch")
        lens = offs[1:] - offs[:-1]
        split = lens > np.uint64(lim)
        return out[0::2].copy(), np.ma.masked_array(out[1::2].copy(), mask=~split)

    def locate(self, seqs, rc=True, max_hits=1000, max_len=MAX_STRING_LEN):
        """Where every query occurs in the indexed reads (sigax_locate_batch) -> (totals u64[n], qflags u32[n], hit_offs
        u64[n+1], hits): totals[q] = match(seqs, rc=rc)'s head; hits (HIT_DTYPE: query, read, offset, flags) of query q are
        hits[hit_offs[q]:hit_offs[q+1]], listed iff the query is non-empty, all ACGT (else qflags & SIGAX_LOCATE_SKIPPED) and
        occurs at most max_hits times (else qflags & SIGAX_LOCATE_OVER): read[offset:offset+len] == query, or its reverse
        complement where flags & SIGAX_HIT_REV.  Walks of more than max_len steps are cut (flags & SIGAX_HIT_CUT).  Needs the
        .sai table and reads of ACGT only."""
        buf, offs = pack_reads(seqs)
        n = len(offs) - 1
        if isinstance(buf, np.ndarray):
            buf = C.c_char_p(buf.ctypes.data) if buf.size else b""
        t, f, o, h = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(_lib.lib().sigax_locate_batch(self._h, buf, offs.ctypes.data, n, SIGAX_RC if rc else 0, int(max_hits), int(max_len),
                                             C.byref(t), C.byref(f), C.byref(o), C.byref(h)), "sigax_locate_batch")
        try:
            totals = _copy_records(t, n, np.dtype(np.uint64))
            qflags = _copy_records(f, n, np.dtype(np.uint32))
            hit_offs = _copy_records(o, n + 1, np.dtype(np.uint64))
            hits = _copy_records(h, int(hit_offs[-1]), HIT_DTYPE)
        finally:
            for p in (t, f, o, h):
                _lib.lib().sigax_free(p)
        return totals, qflags, hit_offs, hits

    def correct_overlap(self, seqs, rounds=1, **pile):
        """`siga correct -a overlap` for a batch (sigax_pileup_batch, rules in include/sigax.h) -> (list of bytes: the corrected
        read where valid is 1, else the read as it went into its last round; valid u8[n]; changed u8[n]; status u64[8], the
        rounds' words added up; rounds run).  The fields of sigax_pile_params as keywords, the CLI's defaults otherwise.  The
        reference text is built from the index at the first call and kept.  Needs the .sai table and reads of ACGT only."""
        L = _lib.lib()
        if getattr(self, "_pile_ref", None) is None:
            ref = C.c_void_p()
            _check(L.sigax_pile_ref_create(self._h, C.byref(ref)), "sigax_pile_ref_create")
            self._pile_ref = ref
        params = _lib.PileParams(**pile)
        buf, offs = pack_reads(seqs)
        n = len(offs) - 1
        if isinstance(buf, np.ndarray):
            buf = C.c_char_p(buf.ctypes.data) if buf.size else b""
        out = np.zeros(int(offs[-1]) + 1, dtype=np.uint8)
        valid, changed = np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8)
        status, run = np.zeros(8, dtype=np.uint64), C.c_uint32()
        _check(L.sigax_pileup_batch(self._h, self._pile_ref, buf, offs.ctypes.data, n, C.byref(params), int(rounds), out.ctypes.data,
                                    valid.ctypes.data, changed.ctypes.data, status.ctypes.data, C.byref(run)), "sigax_pileup_batch")
        text = out.tobytes()
        return [text[int(offs[i]):int(offs[i + 1])] for i in range(n)], valid, changed, status, int(run.value)

    def overlap_mismatch(self, error_permille, min_overlap=45, containments=False, **seed):
        """`siga overlap -e` over every read of the index (sigax_mmoverlap_batch, rules in include/sigax.h) -> (edges, a structured
        array of _lib.MM_EDGE_DTYPE: the canonical dovetail records with num_diff, each once, in (query, target, af, length) order;
        contained u8[n_strings]; status u64[8], the pieces' words added up).  seed: seed_length, seed_stride, max_seed_hits,
        max_candidates, max_read_len as keywords, the CLI's defaults otherwise.  The reference text is built from the index at the
        first call and kept.  Needs the .sai table, reads of ACGT only and set_reads().  containments=True
        (SIGAX_MMO_CONTAINMENTS) -> (edges, contained, status, containments): the containment records of rule 9 in the same dtype
        and order -- query the contained read, target its container, af = 8 | 4 if reversed, reserved the first column of the
        container's forward text it covers -- split from the dovetails; status[7] counts both kinds."""
        L = _lib.lib()
        params = _lib.MmoParams(int(error_permille), min_overlap=int(min_overlap), flags=_lib.MMO_CONTAINMENTS if containments else 0, **seed)
        if getattr(self, "_pile_ref", None) is None:
            ref = C.c_void_p()
            _check(L.sigax_pile_ref_create(self._h, C.byref(ref)), "sigax_pile_ref_create")
            self._pile_ref = ref
        n = self.info()["n_strings"]
        contained = np.zeros(n, dtype=np.uint8)
        status = np.zeros(8, dtype=np.uint64)
        ptr, count = C.c_void_p(), C.c_uint64()
        _check(L.sigax_mmoverlap_batch(self._h, self._pile_ref, C.byref(params), C.byref(ptr), C.byref(count), contained.ctypes.data,
                                       status.ctypes.data), "sigax_mmoverlap_batch")
        try:
            edges = _copy_records(ptr, int(count.value), _lib.MM_EDGE_DTYPE)
        finally:
            L.sigax_free(ptr)
        if containments:
            is_cont = (edges["af"] & _lib.MM_CONTAINMENT) != 0
            return edges[~is_cont], contained, status, edges[is_cont]
        return edges, contained, status

    def get_strings(self, rows, which=0, max_len=MAX_STRING_LEN, stretch=False):
        """FMIndex::getString (src/fmindex.cpp:292-313, sigax_get_strings) for many BWT rows of strand `which` -> list of
        bytes, the text in front of each row's suffix; with stretch=True -> (that list, u64 array of the strings' stretch
        indexes: what the .sai table is indexed by, NO_STRETCH where a walk was cut at max_len or the row is out of range)."""
        rows = np.ascontiguousarray(rows, dtype=np.uint64)
        n = len(rows)
        seqs, offs = C.c_void_p(), C.c_void_p()
        st = np.zeros(n, dtype=np.uint64) if stretch else None
        _check(_lib.lib().sigax_get_strings(self._h, which, rows.ctypes.data, n, int(max_len), C.byref(seqs), C.byref(offs),
                                            st.ctypes.data if stretch else None), "sigax_get_strings")
        try:
            o = np.ctypeslib.as_array(C.cast(offs, C.POINTER(C.c_uint64)), shape=(n + 1,)).copy()
            text = C.string_at(seqs, int(o[-1]))
        finally:
            _lib.lib().sigax_free(seqs)
            _lib.lib().sigax_free(offs)
        out = [text[int(o[i]):int(o[i + 1])] for i in range(n)]
        return (out, st) if stretch else out

    def kmer_spectrum(self, k, n_bins=1024, seqs=None, rows=None, max_len=MAX_STRING_LEN, hist=None):
        """KmerDistribution::sample's loop (src/kmerdistr.cpp:12-33) over strings (`seqs`, sigax_kmer_spectrum_batch) or over the
        strings of BWT rows of the forward strand (`rows`, sigax_kmer_spectrum_rows: they never leave the device) ->
        (hist u64[n_bins], stats dict).  hist[c] = windows whose k-mer occurs c times on both strands together, the last bin
        "n_bins - 1 or more"; pass a previous call's `hist` to accumulate into it."""
        if (seqs is None) == (rows is None):
            raise ValueError("give either seqs or rows")
        if hist is None:
            hist = np.zeros(int(n_bins), dtype=np.uint64)
        elif hist.dtype != np.uint64 or len(hist) != int(n_bins) or not hist.flags.c_contiguous:
            raise ValueError("hist must be a contiguous uint64 array of n_bins entries")
        stat = np.zeros(4, dtype=np.uint64)
        if rows is not None:
            rows = np.ascontiguousarray(rows, dtype=np.uint64)
            _check(_lib.lib().sigax_kmer_spectrum_rows(self._h, rows.ctypes.data, len(rows), int(k), int(max_len), int(n_bins),
                                                       hist.ctypes.data, stat.ctypes.data), "sigax_kmer_spectrum_rows")
        else:
            buf, offs = pack_reads(seqs)
            if isinstance(buf, np.ndarray):
                buf = C.c_char_p(buf.ctypes.data) if buf.size else b""
            _check(_lib.lib().sigax_kmer_spectrum_batch(self._h, buf, offs.ctypes.data, len(offs) - 1, int(k), int(n_bins),
                                                        hist.ctypes.data, stat.ctypes.data), "sigax_kmer_spectrum_batch")
        return hist, {"strings": int(stat[0]), "bases": int(stat[1]), "windows": int(stat[2]), "sectors": int(stat[3])}


class OverlapBuilder:
    """src/overlap_builder.h:19-45 over the GPU library."""

    def __init__(self, fmi, prefix="default", irreducible=True, rc=True):
        self.fmi = fmi
        self.prefix = prefix
        self.irreducible = irreducible
        self.rc = rc

    def _flags(self, edges):
        return (SIGAX_IRREDUCIBLE if self.irreducible else 0) | (SIGAX_RC if self.rc else 0) | (SIGAX_EDGES if edges else 0)

    def duplicate(self, seqs, read_base=0, edges=False):
        """Batched OverlapBuilder::duplicate (src/overlap_builder.cpp:1184-1195)."""
        return self.overlap(seqs, 0, read_base, edges, _flags=SIGAX_DUPLICATE | (SIGAX_EDGES if edges else 0))

    def overlap(self, seqs, min_overlap, read_base=0, edges=False, _flags=None):
        """Batched OverlapBuilder::overlap.  Returns dict(block_offs, blocks, substring, edges, stats)."""
        buf, offs = pack_reads(seqs)
        if getattr(self.fmi, "_resident", False) and _flags is None and min_overlap < getattr(self.fmi, "_deep_for", 1 << 30):
            self.fmi.prepare_overlap(min_overlap)  # an index that stays open: tables for this minimum overlap (and larger ones)
        elif getattr(self.fmi, "_prepare_pending", False):
            self.fmi.prepare()
        res = _lib.Result()
        if isinstance(buf, np.ndarray):
            buf = C.c_char_p(buf.ctypes.data) if buf.size else b""
        _check(_lib.lib().sigax_overlap_batch(self.fmi.handle, buf, offs.ctypes.data, len(offs) - 1, read_base, min_overlap,
                                              self._flags(edges) if _flags is None else _flags, C.byref(res)),
               "sigax_overlap_batch")
        try:
            n = res.n_reads
            block_offs = np.ctypeslib.as_array(res.block_offs, shape=(n + 1,)).copy()
            nb = int(block_offs[-1])
            blocks = _copy_records(res.blocks, nb, BLOCK_DTYPE)
            substring = np.ctypeslib.as_array(res.substring, shape=(max(n, 1),))[:n].copy()
            ne = int(res.n_edges)
            eds = _copy_records(res.edges, ne, EDGE_DTYPE)
            stats = res.stats.as_dict()
        finally:
            _lib.lib().sigax_result_free(C.byref(res))
        return {"block_offs": block_offs, "blocks": blocks, "substring": substring, "edges": eds, "stats": stats}

    def overlap_sharded(self, seqs, min_overlap, shards):
        """`overlap(seqs, min_overlap, edges=True)` run shard by shard: `shards` is a list of arrays of read ids that together
        name every read once (key-range sharding: np.array_split(key_order(locality_keys(...)), N)).  Each shard runs as one
        batch under its ids, as one rank of a key-sharded run does; the shards' edge records are concatenated in device
        memory, put back into read order there (sigax_edges_restore_order) and downloaded once, and the substring flags go to
        their reads' places the same way (sigax_flags_by_read_id).  Returns (edges, substring): the one-batch run's, byte
        for byte.  The index must know its reads (FMIndexPair.set_reads)."""
        L = _lib.lib()
        seqs = list(seqs)
        n = len(seqs)
        shards = [np.ascontiguousarray(s, dtype=np.int64).reshape(-1) for s in shards]
        named = np.concatenate(shards) if shards else np.zeros(0, dtype=np.int64)
        if len(named) != n or (n and (named.min() < 0 or named.max() >= n or (np.bincount(named, minlength=n) != 1).any())):
            raise ValueError("shards must name every one of the %d reads exactly once" % n)
        if getattr(self.fmi, "_resident", False) and min_overlap < getattr(self.fmi, "_deep_for", 1 << 30):
            self.fmi.prepare_overlap(min_overlap)
        elif getattr(self.fmi, "_prepare_pending", False):
            self.fmi.prepare()
        device = self.fmi.info()["device"]
        shards = [s.astype(np.uint32) for s in shards if len(s)]
        bt = C.c_void_p()
        held = []

        def dev(nbytes):
            held.append(_DeviceBytes(nbytes, device))
            return held[-1]

        try:
            d_sub = dev(n).zero()
            d_status = dev(16)
            parts = []  # (device records, how many) per shard, in shard order
            if shards:
                _check(L.sigax_batch_create(self.fmi.handle, max(len(s) for s in shards), 0, max(len(seqs[i]) for i in range(n)), C.byref(bt)),
                       "sigax_batch_create")
            for ids in shards:
                buf, offs = pack_reads([seqs[i] for i in ids])
                d_ids = dev(ids.nbytes).upload(ids)
                _check(L.sigax_batch_upload(bt, buf, offs.ctypes.data, len(ids), None), "sigax_batch_upload")
                _check(L.sigax_batch_set_device_read_ids(bt, d_ids.ptr, len(ids)), "sigax_batch_set_device_read_ids")
                _check(L.sigax_batch_run(bt, 0, min_overlap, self._flags(True), None), "sigax_batch_run")
                stats = _lib.Stats()
                _check(L.sigax_batch_finish(bt, None, C.byref(stats)), "sigax_batch_finish")
                p_sub, p_edges = C.c_void_p(), C.c_void_p()
                _check(L.sigax_batch_device_outputs(bt, None, None, C.byref(p_sub), C.byref(p_edges)), "sigax_batch_device_outputs")
                _check(L.sigax_flags_by_read_id(device, p_sub, d_ids.ptr, len(ids), n, d_sub.ptr, d_status.ptr, None), "sigax_flags_by_read_id")
                if d_status.download(np.uint64, 1)[0]:
                    raise SigaxError(_lib.SIGAX_E_ARG, "sigax_flags_by_read_id (a read id beyond the reads)")
                part = dev(int(stats.n_edges) * EDGE_DTYPE.itemsize)  # the batch object's own buffer serves the next shard
                part.copy_from_device(0, p_edges, part.nbytes)
                parts.append((part, int(stats.n_edges)))
            total = sum(k for _, k in parts)
            d_cat, d_out = dev(total * EDGE_DTYPE.itemsize), dev(total * EDGE_DTYPE.itemsize)
            at = 0
            for part, k in parts:
                d_cat.copy_from_device(at, part.ptr, part.nbytes)
                at += part.nbytes
            need = C.c_uint64()
            _check(L.sigax_edges_order_workspace(total, n, C.byref(need)), "sigax_edges_order_workspace")
            d_work = dev(need.value)
            _check(L.sigax_edges_restore_order(device, d_cat.ptr, total, n, d_out.ptr, None, d_work.ptr, need.value, d_status.ptr, None),
                   "sigax_edges_restore_order")
            status = d_status.download(np.uint64, 2)  # (the copy waits for the kernels)
            if status[0] or status[1]:
                raise RuntimeError("sigax_edges_restore_order refused the shards' records: %d with a query beyond the reads, %d runs "
                                   "beyond the first of their query" % (status[0], status[1]))
            return ShardedResult(d_out.download(EDGE_DTYPE, total), d_sub.download(np.uint8, n))
        finally:
            if bt:
                L.sigax_batch_destroy(bt)
            for d in held:
                d.free()

    def build(self, input_path, min_overlap, output_path=None):
        """HT + VT + ED text exactly as OverlapBuilder::build writes it at -t 1 (src/overlap_builder.cpp:423-483).
        Returns the text; also writes it to output_path (gz if it ends with .gz)."""
        reads = read_sequences(input_path)
        names = [r[0] for r in reads]
        seqs = [r[2] for r in reads]
        lengths = np.array([len(s) for s in seqs], dtype=np.uint32)
        self.fmi.set_reads(lengths, name_ranks(names))
        res = self.overlap(seqs, min_overlap, 0, edges=True)
        text = format_asqg(reads, res, min_overlap)
        if output_path:
            opener = gzip.open if output_path.endswith(".gz") else open
            with opener(output_path, "wb") as f:
                f.write(text.encode("latin-1"))
        return text, res


def edge_coords(length, af, qlen, tlen):
    """OverlapBlock::overlap (src/overlap_builder.cpp:158-175)."""
    s0, e0 = qlen - length, qlen - 1
    s1, e1 = 0, length - 1
    if af & 1:
        s0, e0 = qlen - e0 - 1, qlen - s0 - 1
    if af & 2:
        s1, e1 = tlen - e1 - 1, tlen - s1 - 1
    return s0, e0, s1, e1


def _vertex_tags(comment):
    """OverlapPostProcess (src/overlap_builder.cpp:304-316) + VertexRecord << (src/asqg.cpp:171-186)."""
    cov = bar = ext = None
    if comment:
        for tok in comment.split(" "):
            parts = tok.split(":")
            if tok.startswith("BX"):
                if len(parts) == 3 and parts[1] == "Z":
                    w = parts[2].split()
                    bar = w[0] if w else ""
            elif tok.startswith("CR"):
                if len(parts) == 3 and parts[1] == "i":
                    cov = _parse_int(parts[2])
            elif tok.startswith("EX"):
                if len(parts) == 3 and parts[1] == "Z":
                    w = parts[2].split()
                    ext = w[0] if w else ""
    out = ""
    if cov is not None:
        out += "\tCR:i:%d" % cov
    if bar is not None:
        out += "\tBX:Z:%s" % bar
    if ext is not None:
        out += "\tEX:Z:%s" % ext
    return out


def _parse_int(s):
    """std::istream >> int: optional leading whitespace, sign, digits; 0 on failure; clamped on overflow."""
    s = s.lstrip(" \t\n\v\f\r")
    i = 0
    if i < len(s) and s[i] in "+-":
        i += 1
    j = i
    while j < len(s) and s[j].isdigit():
        j += 1
    if j == i:
        return 0
    v = int(s[:j])
    return max(-2**31, min(2**31 - 1, v))


def format_asqg(reads, res, min_overlap):
    lines = ["HT\tVN:i:1\tOL:i:%d\tCN:i:1" % min_overlap]
    sub = res["substring"]
    for i, (name, comment, seq) in enumerate(reads):
        lines.append("VT\t%s\t%s\tSS:i:%d%s" % (name, seq, 1 if sub[i] else 0, _vertex_tags(comment)))
    lens = [len(r[2]) for r in reads]
    for e in res["edges"]:
        q, t, ln, af = int(e["query"]), int(e["target"]), int(e["length"]), int(e["af"])
        s0, e0, s1, e1 = edge_coords(ln, af, lens[q], lens[t])
        lines.append("ED\t%s %s %d %d %d %d %d %d %d 0" % (reads[q][0], reads[t][0], s0, e0, lens[q], s1, e1, lens[t],
                                                          1 if af & 4 else 0))
    return "\n".join(lines) + "\n"


def format_hits(res):
    """Hits text (src/overlap_builder.cpp:234-241), one line per read."""
    out = []
    offs, b = res["block_offs"], res["blocks"]
    for r in range(len(offs) - 1):
        lo, hi = int(offs[r]), int(offs[r + 1])
        parts = ["%d %d %d " % (r, 1 if res["substring"][r] else 0, hi - lo)]
        for k in range(lo, hi):
            x = b[k]
            af = int(x["af"])
            parts.append("%d %d %d %d %d %d %d %d %d %d%d%d " % (
                x["capped0_lo"], x["capped0_hi"], x["capped1_lo"], x["capped1_hi"], x["raw0_lo"], x["raw0_hi"],
                x["raw1_lo"], x["raw1_hi"], x["length"], (af >> 2) & 1, (af >> 1) & 1, af & 1))
        out.append("".join(parts))
    return "\n".join(out) + "\n"
