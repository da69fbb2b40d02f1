"""Containment records of `siga overlap -e` on the GPU (SIGAX_MMO_CONTAINMENTS, csrc/sigax_mmoverlap.hip) bit for bit against the
serial restatement (tests/contained_cases.py): the batch form in one piece and in pieces, the device form with buffers of exactly
their size, the Python ends and the command line; and flags = 0 against the dovetail records of the same run."""
import ctypes as C
import functools
import gzip
import os

import numpy as np
import pytest

from tests import consensus_cases as cc
from tests import contained_cases as kc
from tests import mmoverlap_cases as mc
from tests import test_gpu_mmoverlap as tm

pytestmark = pytest.mark.gpu

FIELDS = ("query", "target", "length", "af", "num_diff", "reserved")


def _six(edges):
    return [tuple(int(e[k]) for k in FIELDS) for e in edges]


def _order(records):
    return sorted(set(records), key=lambda r: (r[0], r[1], r[3], r[2], r[5]))


@functools.lru_cache(maxsize=None)
def _noisy():
    case = cc.noisy_case(2, True)
    refs = [r.decode() for r in case["reads"]]
    return refs, case["names"], case["params"]


def _sets():
    """name -> (refs, names, params)"""
    out = {"b_" + k: v[:3] for k, v in mc.boundary_sets().items()}
    out.update({"h_" + k: v[:3] for k, v in kc.hand_sets().items()})
    out["chain"] = kc.duplicate_chain()
    return out


def _check_batch(refs, names, p):
    """flags = 1 against the restatement, and flags = 0 against the dovetails of that run -> (dovetails, containments, written)"""
    ranks = mc.name_ranks(names)
    want_dove, want_contained, want_st = mc.expected_mm_overlaps(refs, ranks, p)
    want_conts, written = kc.expected_containments(refs, ranks, p)
    pair = tm._open(refs, names)
    try:
        edges, contained, status, conts = pair.overlap_mismatch(p["P"], p["M"], containments=True, **tm._kw(p))
        assert _six(conts) == want_conts
        assert tm._tuples(edges) == want_dove and contained.tolist() == want_contained
        assert status.tolist() == want_st[:7] + [want_st[7] + written]
        plain = pair.overlap_mismatch(p["P"], p["M"], **tm._kw(p))
        assert plain[0].tobytes() == edges.tobytes() and plain[1].tolist() == want_contained and plain[2].tolist() == want_st
    finally:
        pair.close()
    return want_dove, want_conts, written


def test_every_hand_and_boundary_set():
    for name, (refs, names, p) in sorted(_sets().items()):
        _, conts, _ = _check_batch(refs, names, p)
        if name.startswith("h_"):
            assert conts == kc.hand_sets()[name[2:]][3], name
    assert _check_batch(*kc.duplicate_chain())[1] == [(k, k - 1, 100, 8, 1, 0) for k in range(1, 40)]


def test_noisy_mixed_lengths_in_one_piece_and_in_pieces(monkeypatch):
    refs, names, p = _noisy()
    dove, conts, written = _check_batch(refs, names, p)
    assert len(conts) > 300 and {r[3] for r in conts} == {8, 12} and any(r[4] for r in conts) and written > len(conts)
    monkeypatch.setenv("SIGAX_TEST_MMO_PIECE", "64")
    monkeypatch.setenv("SIGAX_TEST_MMO_EDGES_CAP", "1")
    assert _check_batch(refs, names, p) == (dove, conts, written)


def test_device_form_exact_buffers_and_overflow(monkeypatch):
    """one call with room for exactly its records, dovetails and containments; one record short, nothing is written"""
    from siga_amd import _lib
    refs, names, p = _noisy()
    ranks = mc.name_ranks(names)
    want_dove, want_contained, want_st = mc.expected_mm_overlaps(refs, ranks, p)
    want_conts, written = kc.expected_containments(refs, ranks, p)
    total = want_st[7] + written
    monkeypatch.setattr(tm, "_params", lambda q, max_len=True: _lib.MmoParams(q["P"], min_overlap=q["M"], max_read_len=q["max_len"],
                                                                             flags=_lib.MMO_CONTAINMENTS, **tm._kw(q)))
    pair = tm._open(refs, names)
    try:
        calls = tm._Calls(pair, refs, total - 1)
        try:
            st = calls.call(p, 0, len(refs), want_st[0])
            assert st == want_st[:7] + [total] and calls.cursor() == 0
            assert calls.raw().tobytes() == b"\xee" * (24 * (total - 1)) and not any(calls.contained())
        finally:
            calls.close()
        calls = tm._Calls(pair, refs, total)
        try:
            assert calls.call(p, 0, len(refs), want_st[0]) == want_st[:7] + [total] and calls.cursor() == total
            raw = calls.raw()
            assert b"\xee\xee\xee\xee" not in raw.tobytes()
            got = _six(raw)
            assert _order([r for r in got if r[3] & 8]) == want_conts
            assert _order([r for r in got if not r[3] & 8]) == [r + (0,) for r in want_dove]
            assert calls.contained() == want_contained
            # the finish: one ordered stream, every record once
            n_raw = calls.cursor()
            wb = C.c_uint64()
            assert calls.L.sigax_mmoverlap_finish_workspace(n_raw, C.byref(wb)) == 0
            d_n, d_work = calls.dev.buf(8), calls.dev.buf(wb.value)
            assert calls.L.sigax_mmoverlap_finish_device(calls.d_edges, n_raw, d_n, d_work, wb.value, calls.stream) == 0, _lib.last_error()
            assert calls.dev.hip.hipStreamSynchronize(calls.stream) == 0
            n = int(calls.dev.get(d_n, np.uint64, 1)[0])
            assert _six(calls.raw()[:n]) == _order([r + (0,) for r in want_dove] + want_conts)
        finally:
            calls.close()
    finally:
        pair.close()


def test_argument_errors():
    from siga_amd import _lib
    L = _lib.lib()
    wb = C.c_uint64()
    for flags in (2, 3, 0x80000000):
        params = _lib.MmoParams(40, flags=flags)
        assert L.sigax_mmoverlap_workspace(1, 100, C.byref(params), 10, C.byref(wb)) == _lib.SIGAX_E_ARG
        assert "flags" in _lib.last_error()
    assert L.sigax_mmoverlap_workspace(1, 100, C.byref(_lib.MmoParams(40, flags=1)), 10, C.byref(wb)) == 0 and wb.value > 0


def test_cli_and_host_write_the_containments(tmp_path):
    from siga_amd import host
    refs, names, p = _noisy()
    ranks = mc.name_ranks(names)
    want = mc.expected_mm_overlaps(refs, ranks, p)
    conts, written = kc.expected_containments(refs, ranks, p)
    d = str(tmp_path)
    prefix = tm._link_index(tm._index(refs, names), d)
    args = ["-e", str(p["P"]), "-m", str(p["M"]), "--seed-length=%d" % p["S"], "--seed-stride=%d" % p["T"]]
    r = tm._cli(args + ["--containments", "conts.tsv", "reads.fa"], d)
    assert r.returncode == 0, r.stderr.decode()
    assert b"%d containments" % len(conts) in r.stderr
    assert open(os.path.join(d, "conts.tsv")).read() == kc.containment_lines(names, conts)
    assert gzip.open(prefix + ".asqg.gz", "rt").read() == mc.asqg_text(names, refs, want[0], want[1], p["M"])
    out, cf = os.path.join(d, "two.asqg"), os.path.join(d, "two.tsv.gz")
    status = host.overlap_file(prefix + ".fa", prefix, p["M"], out, error_permille=p["P"], containments=cf, seed_length=p["S"], seed_stride=p["T"])
    assert status.tolist() == want[2][:7] + [want[2][7] + written]
    assert gzip.open(cf, "rt").read() == kc.containment_lines(names, conts)
    assert open(out).read() == mc.asqg_text(names, refs, want[0], want[1], p["M"])
    # the switch belongs to -e, and the help names it
    r = tm._cli(["--containments", "x.tsv", "reads.fa"], d)
    assert r.returncode == 1 and b"--containments" in r.stderr and not os.path.exists(os.path.join(d, "x.tsv"))
    assert b"--containments" in tm._cli(["--help"], d).stdout


# ---- the placement pass (csrc/sigax_contained.hip) -----------------------------------------------------------------------------------
def _np_tables(tables, n):
    from siga_amd import _lib
    lay = np.zeros(len(tables["layout"]), dtype=_lib.PLACEMENT_DTYPE)
    for k, (r, fl, o) in enumerate(tables["layout"]):
        lay[k] = (r, fl, o)
    return {"seq_offs": np.array(tables["seq_offs"], dtype=np.uint64), "lay_offs": np.array(tables["lay_offs"], dtype=np.uint64), "layout": lay}


def _np_records(recs):
    from siga_amd import _lib
    out = np.zeros(len(recs), dtype=_lib.MM_EDGE_DTYPE)
    for k, r in enumerate(recs):
        out[k] = r
    return out


def _same_placement(got, exp, what, layout=True):
    assert got["place_class"].tolist() == exp["place_class"], what
    assert got["place_status"].tolist() == exp["status"], what
    if layout:
        assert got["lay_offs"].tolist() == exp["lay_offs"], what
        assert [tuple(int(x) for x in p) for p in got["layout"]] == exp["layout"], what


def _host_case(lengths, contained, recs, tables, what):
    import siga_amd
    exp = kc.expected_placement(tables, lengths, contained, recs)
    got = siga_amd.unitigs_place_contained(_np_tables(tables, len(lengths)), lengths, contained, _np_records(recs))
    _same_placement(got, exp, what)
    return exp


def test_placement_parity_hand_cases_and_chain():
    for name, (lengths, contained, recs, tables, want) in sorted(kc.hand_placements().items()):
        exp = _host_case(lengths, contained, recs, tables, name)
        assert exp["status"][3] == len(want)
    refs, names, p = kc.duplicate_chain()
    recs, _ = kc.expected_containments(refs, mc.name_ranks(names), p)
    lengths = [len(r) for r in refs]
    exp = _host_case(lengths, [0] + [1] * 39, recs, kc.single_unitig(100)(lengths), "chain")
    assert exp["status"][6] == 39 and exp["status"][3] == 39


def test_placement_parity_crowded_tiled_and_unplaceable():
    assert _host_case(*kc.crowded_unitig(), "crowded")["status"][3] == 70  # more than a wave in one unitig
    exp = _host_case(*kc.tiled_unitigs(), "tiled")
    assert exp["status"][3] == 54 and exp["lay_offs"][:7] == [0, 12, 24, 36, 48, 60, 72]
    exp = _host_case(*kc.unplaceable(), "unplaceable")  # a root that a trim round removed among them
    assert exp["status"][5] == 1 and exp["status"][3] == 0


def test_placement_of_no_reads_and_of_none_contained():
    import siga_amd
    got = siga_amd.unitigs_place_contained({"seq_offs": [0], "lay_offs": [0], "layout": np.zeros(0, dtype=siga_amd._lib.PLACEMENT_DTYPE)}, [], [], [])
    assert got["place_status"].tolist() == [0] * 8 and len(got["layout"]) == 0 and got["lay_offs"].tolist() == [0]
    lengths = [50, 60, 70]
    tables = {"seq_offs": [0, 50, 110, 180], "lay_offs": [0, 1, 2, 3], "layout": [(0, 0, 0), (1, 1, 0), (2, 0, 0)]}
    exp = _host_case(lengths, [0, 0, 0], [], tables, "none contained")
    assert exp["layout"] == tables["layout"] and exp["status"] == [0, 0, 0, 0, 0, 0, 0, 3]


class _Guarded:
    """a device buffer with 256 bytes of 0xEE on either side of what the call is given"""

    def __init__(self, dev, nbytes, src=None):
        self.dev, self.nbytes = dev, nbytes
        self.base = dev.buf(nbytes + 512)
        self.ptr = C.c_void_p(self.base.value + 256)
        if src is not None and src.nbytes:
            assert dev.hip.hipMemcpy(self.ptr, src.ctypes.data, src.nbytes, 1) == 0

    def get(self, dtype, count):
        whole = self.dev.get(self.base, np.uint8, self.nbytes + 512)
        assert whole[:256].tobytes() == b"\xee" * 256 and whole[256 + self.nbytes:].tobytes() == b"\xee" * 256, "guard bytes overwritten"
        return np.frombuffer(whole[256:256 + np.dtype(dtype).itemsize * count].tobytes(), dtype=dtype)


def _device_case(lengths, contained, recs, tables, n_unitigs=None):
    """sigax_contained_place_device on a stream, every buffer of exactly its size between guard bytes -> dict as the host form's"""
    from siga_amd import _lib
    from tests.test_gpu_overlap_correct import _Device
    L, dev = _lib.lib(), _Device()
    n, m = len(lengths), len(tables["seq_offs"]) - 1
    t = _np_tables(tables, n)
    lay = np.full(n, 0xFF, dtype=np.uint8).repeat(16).view(_lib.PLACEMENT_DTYPE)
    lay[:min(n, len(t["layout"]))] = t["layout"][:n]
    r = _np_records(recs)
    stream = C.c_void_p()
    assert L.sigax_stream_create(0, C.byref(stream)) == 0
    try:
        wb = C.c_uint64()
        assert L.sigax_contained_place_workspace(n, m, len(r), C.byref(wb)) == 0, _lib.last_error()
        d_nu = dev.buf(8, np.array([m if n_unitigs is None else n_unitigs], dtype=np.uint64))
        d_so, d_lo, d_lay = dev.buf(8 * (m + 1), t["seq_offs"]), dev.buf(8 * (m + 1), t["lay_offs"]), dev.buf(16 * n, lay)
        d_len, d_cont = dev.buf(4 * n, np.array(lengths, dtype=np.uint32)), dev.buf(n, np.array(contained, dtype=np.uint8))
        d_recs = dev.buf(24 * len(r), r)
        lo2, lay2, cls, st = _Guarded(dev, 8 * (m + 1)), _Guarded(dev, 16 * n), _Guarded(dev, n), _Guarded(dev, 64)
        work = _Guarded(dev, wb.value)
        opts = _lib.ContainedOpts()
        assert dev.hip.hipDeviceSynchronize() == 0
        rc = L.sigax_contained_place_device(0, d_nu, m, d_so, d_lo, d_lay, d_len, n, d_cont, d_recs if len(r) else None, len(r), C.byref(opts),
                                            lo2.ptr, lay2.ptr, cls.ptr, st.ptr, work.ptr, wb.value, stream)
        assert rc == 0, _lib.last_error()
        assert dev.hip.hipStreamSynchronize(stream) == 0
        work.get(np.uint8, 0)
        status = st.get(np.uint64, 8)
        return {"lay_offs": lo2.get(np.uint64, m + 1)[:min(m, n) + 1], "layout": lay2.get(_lib.PLACEMENT_DTYPE, n)[:int(status[7])],
                "place_class": cls.get(np.uint8, n), "place_status": status}
    finally:
        dev.free()
        L.sigax_stream_destroy(0, stream)


def test_device_form_between_guard_bytes():
    for name, case in (("crowded", kc.crowded_unitig()), ("tiled", kc.tiled_unitigs()), ("unplaceable", kc.unplaceable())):
        _same_placement(_device_case(*case), kc.expected_placement(case[3], *case[:3]), name)
    # fewer unitigs than the tables have room for: the count is read on the device
    lengths, contained, recs, tables = kc.tiled_unitigs()
    exp = kc.expected_placement(tables, lengths, contained, recs, n_unitigs=4)
    got = _device_case(lengths, contained, recs, tables, n_unitigs=4)
    got["lay_offs"] = got["lay_offs"][:5]
    _same_placement(got, exp, "four unitigs")


def test_foreign_tables_touch_nothing_else():
    for name, (lengths, contained, recs, tables) in sorted(kc.foreign_tables().items()):
        got = _device_case(lengths, contained, recs, tables)  # (it checks the guard bytes of every output and of the workspace)
        _same_placement(got, kc.expected_placement(tables, lengths, contained, recs), name, layout=False)
    exp = kc.expected_placement(*[kc.foreign_tables()["cycles"][k] for k in (3, 0, 1, 2)])
    assert exp["place_class"] == [0, kc.NO_ROOT, kc.NO_ROOT, kc.NO_ROOT, kc.NO_RECORD, 0]


def test_placement_argument_errors():
    from siga_amd import _lib
    L = _lib.lib()
    wb = C.c_uint64()
    assert L.sigax_contained_place_workspace(4, 4, 0, None) == _lib.SIGAX_E_ARG
    assert L.sigax_contained_place_workspace(1 << 31, 4, 0, C.byref(wb)) == _lib.SIGAX_E_ARG
    assert L.sigax_contained_place_workspace(4, 4, 2, C.byref(wb)) == 0 and wb.value > 0
    st = np.zeros(8, dtype=np.uint64)
    ok, bad = _lib.ContainedOpts(), _lib.ContainedOpts()
    bad.reserved[2] = 1
    p16 = C.c_void_p(4096)  # never read: every call below is refused before anything is queued
    args = lambda **kw: [kw.get(k, v) for k, v in (("device", 0), ("nu", p16), ("m", 4), ("so", p16), ("lo", p16), ("lay", p16), ("len", p16), ("n", 4),
                                                  ("cont", p16), ("recs", p16), ("k", 2), ("opts", C.byref(ok)), ("lo2", p16), ("lay2", p16),
                                                  ("cls", p16), ("st", st.ctypes.data), ("work", p16), ("wb", wb.value), ("stream", None))]
    for kw, word in (({"nu": None}, "NULL"), ({"lay2": None}, "NULL"), ({"recs": None}, "NULL"), ({"st": None}, "NULL"), ({"opts": None}, "NULL"),
                     ({"opts": C.byref(bad)}, "reserved"), ({"work": C.c_void_p(4104)}, "16-byte"), ({"lay": C.c_void_p(4104)}, "16-byte"),
                     ({"lo2": C.c_void_p(4100)}, "8-byte"), ({"len": C.c_void_p(4098)}, "4-byte"), ({"wb": wb.value - 1}, "workspace"),
                     ({"n": 1 << 31}, "2^31")):
        assert L.sigax_contained_place_device(*args(**kw)) == _lib.SIGAX_E_ARG, kw
        assert word in _lib.last_error(), (kw, _lib.last_error())
    out = [C.c_void_p(), C.c_void_p(), C.c_void_p()]
    assert L.sigax_contained_place_host(0, 5, None, None, None, None, 4, None, None, 0, C.byref(ok), C.byref(out[0]), C.byref(out[1]), C.byref(out[2]),
                                        st.ctypes.data) == _lib.SIGAX_E_ARG  # more unitigs than reads
    assert L.sigax_contained_place_host(0, 0, None, None, None, None, 0, None, None, 0, C.byref(ok), None, None, None, st.ctypes.data) == _lib.SIGAX_E_ARG


@pytest.mark.parametrize("seed", (2, 3))
def test_end_to_end_the_dropped_variants_assemble_to_the_genome(seed):
    """overlaps with containment records, the reduction, the placement and the vote, all on the device, over the two variants
    whose one wrong base two placed reads could not outvote"""
    import siga_amd
    from siga_amd import _lib
    from tests.test_contained_cases import noisy_placed, wrong_bases
    case, exp, pl, cons = noisy_placed(seed, True)
    refs = [r.decode() for r in case["reads"]]
    p = case["params"]
    pair = tm._open(refs, case["names"])
    try:
        edges, contained, _, conts = pair.overlap_mismatch(p["P"], p["M"], containments=True, **tm._kw(p))
    finally:
        pair.close()
    keep = (contained[edges["query"]] == 0) & (contained[edges["target"]] == 0)
    e4 = np.zeros(int(keep.sum()), dtype=_lib.EDGE_DTYPE)
    for k in ("query", "target", "length", "af"):
        e4[k] = edges[k][keep]
    lengths, seqs, offs = cc.arrays(case)
    red = siga_amd.unitigs_reduce(e4, lengths, seqs, offs, p["M"], 0, 0)
    placed = siga_amd.unitigs_place_contained(red, lengths, contained, conts)
    _same_placement(placed, pl, "noisy")
    voted = siga_amd.unitigs_consensus(placed, lengths, seqs, offs)
    assert voted["useqs"].tobytes() == cons["useqs"] and voted["status"].tolist() == cons["status"]
    before = siga_amd.unitigs_consensus(red, lengths, seqs, offs)
    assert before["useqs"].tobytes() == exp["consensus"]["useqs"]
    # one unitig that is not a contained read on its own, and it is the genome; without the placement one base is wrong
    got = cc.assembled(case, dict(exp, consensus={"useqs": voted["useqs"].tobytes()}))
    assert [c for _, c in got] == [case["genome"]]
    old = cc.assembled(case, dict(exp, consensus={"useqs": before["useqs"].tobytes()}))
    assert len(old) == 1 and wrong_bases(old[0][1], case["genome"]) == 1


# ---- `siga unitig -e --place-contained`: the host class and the command line ---------------------------------------------------------
def _placed_files(case, exp, pl, cons):
    """the FASTA and layout texts of `siga unitig -e --place-contained`: what is hidden comes from the call's own layout, the
    counts and the lines from the pass's"""
    red, names = exp["reduced"], case["names"]
    fa, lay = [], []
    for u in range(len(red["uflags"])):
        a, b = red["lay_offs"][u], red["lay_offs"][u + 1]
        if b - a == 1 and exp["contained"][red["layout"][a][0]]:
            continue
        a, b = pl["lay_offs"][u], pl["lay_offs"][u + 1]
        seq = cons["useqs"][red["seq_offs"][u]:red["seq_offs"][u + 1]].decode()
        fa.append(">unitig-%d" % u + (" KC:i:%d" % (b - a) if b - a > 1 else "") + " changed=%d\n" % cons["changed"][u] + seq + "\n")
        lay += ["unitig-%d\t%s\t%s\t%d%s\n" % (u, names[r], "-" if fl & 1 else "+", o, "\tcontained" if fl & 2 else "") for r, fl, o in pl["layout"][a:b]]
    return "".join(fa), "".join(lay)


@pytest.mark.parametrize("seed", (2, 3))
def test_cli_and_host_place_contained(seed, tmp_path):
    from siga_amd import host
    from tests import test_gpu_unitig_consensus as tc
    from tests.test_contained_cases import noisy_placed
    case, exp, pl, cons = noisy_placed(seed, True)
    d = str(tmp_path)
    prefix = tc._files([r.decode() for r in case["reads"]], case["names"], d)
    fa, lay = _placed_files(case, exp, pl, cons)
    r = tc._cli(tc.NOISY_ARGS + ["--place-contained", "-o", "u.fa", "--layout", "u.lay", "reads.fa"], d)
    assert r.returncode == 0, r.stderr.decode()
    read = lambda name: open(os.path.join(d, name)).read()
    assert read("u.fa") == fa and fa.count(">") == 1 and fa.split("\n")[1].encode() in (case["genome"], cc.uc.revcomp(case["genome"]))
    assert read("u.lay") == lay and lay.count("\tcontained\n") == sum(exp["contained"])
    assert b"%d contained reads placed, 0 not" % sum(exp["contained"]) in r.stderr
    # without the switch the output is what it was: one wrong base
    r = tc._cli(tc.NOISY_ARGS + ["-o", "old.fa", "--layout", "old.lay", "reads.fa"], d)
    assert r.returncode == 0, r.stderr.decode()
    old_fa, old_lay = tc._expected_files(case, exp)[:2]
    assert read("old.fa") == old_fa and read("old.lay") == old_lay
    assert sum(1 for a, b in zip(old_fa.split("\n")[1], fa.split("\n")[1]) if a != b) == 1
    # the wrapper
    st = host.unitig_file(prefix + ".fa", prefix, 30, out=os.path.join(d, "w.fa"), layout=os.path.join(d, "w.lay"), reduce=True, error_permille=40,
                          place_contained=True, seed_length=12, seed_stride=4)
    assert (read("w.fa"), read("w.lay")) == (fa, lay)
    assert st["contained_placed"] == st["contained_reads"] == sum(exp["contained"]) and st["columns_changed"] == cons["status"][2]


def test_cli_place_contained_refusals_and_pairs(tmp_path):
    """the switch needs -e; a pair whose contained mate is placed is a pair again, and a unitig without placements -- the hidden
    unitig of a placed read -- goes through the pairs kernels' bisection"""
    import json
    from siga_amd import host
    from tests import test_gpu_unitig_consensus as tc
    case, exp = cc.noisy_case(1, True), cc.noisy_expected(1, True)
    n = len(case["reads"])
    names = ["p%d/%d" % (k // 2, 1 + k % 2) for k in range(n)]  # reads 2k and 2k + 1 are mates
    d = str(tmp_path)
    prefix = tc._files([r.decode() for r in case["reads"]], names, d)
    r = tc._cli(["--place-contained", "-o", "no.fa", "reads.fa"], d)
    assert r.returncode == 1 and b"--place-contained" in r.stderr and not os.path.exists(os.path.join(d, "no.fa"))
    with pytest.raises(ValueError):
        host.unitig_file(prefix + ".fa", prefix, 30, out=os.path.join(d, "no.fa"), place_contained=True)
    assert b"--place-contained" in tc._cli(["--help"], d).stdout
    r = tc._cli(tc.NOISY_ARGS + ["--place-contained", "-o", "u.fa", "--pairs", "p.json", "reads.fa"], d)
    assert r.returncode == 0, r.stderr.decode()
    got = json.load(open(os.path.join(d, "p.json")))["pairs"]
    c = exp["contained"]
    regained = sum(1 for k in range(0, n - 1, 2) if c[k] or c[k + 1])
    assert regained > 0 and got["contained_mates"] == 0
    assert got["pairs"] == n // 2 and got["mate_entries"] == 2 * got["pairs"] and got["malformed"] == 0
    assert got["unplaced"] == 0 and got["same"] == got["pairs"]
    # the same set without the switch: those pairs are no pairs, and the difference is exactly the regained ones
    r = tc._cli(tc.NOISY_ARGS + ["-o", "old.fa", "--pairs", "old.json", "reads.fa"], d)
    assert r.returncode == 0, r.stderr.decode()
    old = json.load(open(os.path.join(d, "old.json")))["pairs"]
    assert old["contained_mates"] == regained and got["pairs"] - old["pairs"] == regained and old["same"] == old["pairs"]


def test_container_longer_than_65536_bases():
    """the offset of a containment is as wide as its container is long: a read of 70 000 bases, too long to be a query, is found by
    the reads inside it, and they are placed at columns 66 000 and 69 850"""
    import siga_amd
    refs, names, p, want = kc.long_container_set()
    assert _check_batch(refs, names, p)[1] == want
    lengths = [len(r) for r in refs]
    tables = kc.single_unitig(lengths[0], True, 5, lengths[0] + 9)(lengths)
    exp = _host_case(lengths, [0, 1, 1], want, tables, "long container")
    L = lengths[0]
    assert exp["layout"] == [(0, 1, 5), (2, 2, 5), (1, 3, 5 + L - 66000 - 150)] and exp["status"][3] == 2


def test_trim_rounds_remove_a_root(tmp_path):
    """`-x 2 --place-contained`: the contained reads are islands that the trim rounds remove, yet they are placed and --removed
    does not list them; a read whose container went in a round is ROOT_REMOVED, stays listed and is counted in the summary"""
    import siga_amd
    from siga_amd import _lib
    from tests import test_gpu_unitig_consensus as tc
    case, refs, ranks, contained, edges, conts, red, pl = kc.trimmed_case()
    assert pl["status"][5] == 1 and pl["status"][3] == sum(contained) - 1 > 100
    lengths, seqs, offs = cc.arrays(case)
    e4 = np.zeros(len(edges), dtype=_lib.EDGE_DTYPE)
    for k, e in enumerate(edges):
        e4[k] = e
    got = siga_amd.unitigs_reduce(e4, lengths, seqs, offs, 30, 2, 150)
    assert got["lay_offs"].tolist() == red["lay_offs"] and got["removed"].tolist() == red["removed"]
    placed = siga_amd.unitigs_place_contained(got, lengths, contained, _np_records(conts))
    _same_placement(placed, pl, "after trim rounds")
    d = str(tmp_path)
    tc._files(refs, case["names"], d)
    r = tc._cli(tc.NOISY_ARGS + ["-x", "2", "--place-contained", "-o", "u.fa", "--removed", "r.txt", "reads.fa"], d)
    assert r.returncode == 0, r.stderr.decode()
    want = "".join("%s\t%d\n" % (case["names"][k], x) for k, x in enumerate(red["removed"]) if x and pl["place_class"][k] != kc.PLACED)
    assert open(os.path.join(d, "r.txt")).read() == want and want.count("\n") == 2  # the island and the read inside it
    assert b"%d contained reads placed, 1 not: 0 without a record, 0 without a root, 1 with a removed root, 0 invalid" % pl["status"][3] in r.stderr
    r = tc._cli(tc.NOISY_ARGS + ["-x", "2", "-o", "v.fa", "--removed", "old.txt", "reads.fa"], d)
    assert r.returncode == 0, r.stderr.decode()
    assert open(os.path.join(d, "old.txt")).read() == "".join("%s\t%d\n" % (case["names"][k], x) for k, x in enumerate(red["removed"]) if x)
