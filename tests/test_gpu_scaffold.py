"""Scaffolds of `siga unitig --scaffold` on the GPU (csrc/sigax_scaffold.hip) against the serial restatement of its rules
(tests/scaffold_cases.py::expected_scaffolds): the host form, and the device form over output buffers of exactly their size with
canaries behind them; once the unitig call, the pairs call and the scaffold call enqueued on one stream with nothing in between;
hand-built inputs for the bases pass, the ranking, contended ends, the classes, the gaps and the capacity; hostile tables;
refusals; a hundred random graphs through all three calls; the command line once."""
import ctypes as C
import functools
import os
import random
import subprocess

import numpy as np
import pytest
import torch  # before the library loads: one HIP runtime per process

from oracle import pyoracle as po
from tests import pair_cases as pp
from tests import scaffold_cases as sc
from tests import unitig_cases as uc
from tests.fixtures import CACHE
from tests.golden import make_reads as mr

pytestmark = pytest.mark.gpu
CANARY = 64


def _sopts(o=None):
    from siga_amd import _lib
    o = dict(sc.DEFAULT_OPTS, **(o or {}))
    from_status = o["insert_size"] is None
    return _lib.ScaffoldOpts(_lib.SIGAX_SCAFFOLD_INSERT_FROM_STATUS if from_status else 0, o["min_pairs"], o["link_ratio"], o["min_unitig_bases"],
                             0 if from_status else o["insert_size"], o["min_gap"], o["max_gap"])


def _up(a):
    dev = torch.device("cuda:0")
    a = np.frombuffer(a, dtype=np.uint8) if isinstance(a, bytes) else np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return torch.from_numpy(a.copy()).to(dev) if a.size else torch.zeros(16, dtype=torch.uint8, device=dev)


def _out(nbytes):
    return torch.full((nbytes + CANARY,), 0xEE, dtype=torch.uint8, device="cuda:0")


def _links_array(links):
    from siga_amd import _lib
    return np.array([tuple(r) for r in sc._plain(links)], dtype=_lib.PAIR_LINK_DTYPE)


def _same(got, exp, what, seqs=True):
    print(what, "status", [int(x) for x in got["status"]], "expected", exp["status"])
    assert [int(x) for x in got["status"]] == exp["status"], what
    assert [int(x) for x in got["sc_offs"]] == exp["sc_offs"], what
    assert [int(x) for x in got["sc_lay_offs"]] == exp["sc_lay_offs"], what
    assert [int(x) for x in got["sc_flags"]] == exp["sc_flags"], what
    assert [tuple(int(x) for x in p) for p in got["layout"].tolist()] == exp["layout"], what
    if seqs and exp["seqs"] is not None:
        assert got["seqs"] is not None and bytes(got["seqs"]) == exp["seqs"], what


def _enqueue(L, mu, ml, nu_ptr, so_ptr, uf_ptr, us_ptr, us_bytes, links_ptr, nl_ptr, st24_ptr, o, capacity, stream):
    """sigax_scaffold_device over output buffers of exactly their size plus CANARY bytes of 0xEE -> (buffers, sizes)"""
    from siga_amd import _lib
    wb = C.c_uint64()
    assert L.sigax_scaffold_workspace(mu, ml, C.byref(wb)) == 0
    sizes = {"sc_offs": 8 * (mu + 1), "sc_lay_offs": 8 * (mu + 1), "sc_flags": 4 * mu, "layout": 16 * mu, "status": 128, "work": wb.value}
    if capacity is not None:
        sizes["seqs"] = capacity
    d = {k: _out(v) for k, v in sizes.items()}
    torch.cuda.synchronize()
    opts = _sopts(o)
    rc = L.sigax_scaffold_device(0, nu_ptr, mu, so_ptr, uf_ptr, us_ptr, us_bytes, links_ptr, nl_ptr, ml, st24_ptr, C.byref(opts), d["sc_offs"].data_ptr(),
                                 d["sc_lay_offs"].data_ptr(), d["sc_flags"].data_ptr(), d["layout"].data_ptr(),
                                 d["seqs"].data_ptr() if capacity is not None else None, capacity or 0, d["status"].data_ptr(), d["work"].data_ptr(),
                                 wb.value, stream)
    assert rc == 0, _lib.last_error()
    return d, sizes


def _collect(d, sizes, nu, what):
    """the results, and that nothing behind them was written: the canaries, the table entries beyond the scaffolds, and all of
    the bases buffer when the status says they were not written"""
    from siga_amd import _lib
    h = {k: v.cpu().numpy() for k, v in d.items()}
    status = h["status"][:128].view(np.uint64)
    s, total = int(status[0]), int(status[1])
    assert s <= nu
    used = {"sc_offs": 8 * (s + 1), "sc_lay_offs": 8 * (s + 1), "sc_flags": 4 * s, "layout": 16 * nu, "status": 128}
    got = {"status": status, "sc_offs": h["sc_offs"][:used["sc_offs"]].view(np.uint64), "sc_lay_offs": h["sc_lay_offs"][:used["sc_lay_offs"]].view(np.uint64),
           "sc_flags": h["sc_flags"][:used["sc_flags"]].view(np.uint32), "layout": h["layout"][:used["layout"]].view(_lib.PLACEMENT_DTYPE), "seqs": None}
    if "seqs" in sizes:
        written = int(status[15]) == 0
        assert written == (total <= sizes["seqs"])
        used["seqs"] = total if written else 0
        got["seqs"] = h["seqs"][:total].tobytes() if written else None
    for k in used:
        rest = h[k][used[k]:].tobytes()
        assert len(rest) >= CANARY and rest == b"\xee" * len(rest), "%s: bytes after %s were written" % (what, k)
    assert h["work"][sizes["work"]:].tobytes() == b"\xee" * CANARY, what
    return got


def _device(res, links, st24, o=None, what="", nu_dev=None, nl_dev=None, capacity="exact", seqs=True):
    """the device form over `res` and `links` in buffers of exactly their size -> expected_scaffolds' dict"""
    from siga_amd import _lib
    L = _lib.lib()
    mu, ml = len(res["uflags"]), len(links)
    useqs = bytes(res["useqs"]) if seqs and res.get("useqs") is not None else None
    plain = dict(res) if useqs is not None else {k: v for k, v in res.items() if k != "useqs"}
    exp = sc.expected_scaffolds(plain, links, st24, o, n_unitigs=nu_dev, n_links=nl_dev)
    cap = exp["status"][1] if capacity == "exact" else capacity
    if useqs is None:
        cap = None
    exp = sc.expected_scaffolds(plain, links, st24, o, n_unitigs=nu_dev, n_links=nl_dev, sseqs_capacity=cap or 0)
    counts = _up(np.array([mu if nu_dev is None else nu_dev, ml if nl_dev is None else nl_dev], dtype=np.uint64))
    d_so, d_uf = _up(np.array(res["seq_offs"], dtype=np.uint64)), _up(np.array(res["uflags"], dtype=np.uint32))
    d_us = _up(useqs) if useqs is not None else None
    d_links, d_s24 = _up(_links_array(links)), _up(np.array(st24, dtype=np.uint64))
    d, sizes = _enqueue(L, mu, ml, counts.data_ptr(), d_so.data_ptr(), d_uf.data_ptr(), d_us.data_ptr() if d_us is not None else None,
                        len(useqs) if useqs is not None else 0, d_links.data_ptr(), counts.data_ptr() + 8, d_s24.data_ptr(), o, cap, None)
    torch.cuda.synchronize()
    got = _collect(d, sizes, min(mu, mu if nu_dev is None else nu_dev), what)
    _same(got, exp, what + ", device", seqs=exp["status"][15] == 0)
    if exp["status"][15]:
        assert got["seqs"] is None
    return exp


def _both(res, links, st24=None, o=None, what=""):
    """the host form and the device form against expected_scaffolds"""
    import siga_amd
    st24 = [0] * 24 if st24 is None else st24
    oo = dict(sc.DEFAULT_OPTS, **(o or {}))
    exp = sc.expected_scaffolds(res, links, st24, o)
    got = siga_amd.unitigs_scaffold(res, _links_array(links), status=st24, **oo)
    _same(got, exp, what + ", host")
    _device(res, links, st24, o, what)
    lay = siga_amd.unitigs_scaffold(res, _links_array(links), status=st24, bases=False, **oo)
    assert lay["seqs"] is None
    _same(lay, exp, what + ", host, layout alone", seqs=False)
    return exp


# ---- the bases pass, the ranking ----
@pytest.mark.parametrize("name", [c[0] for c in sc.hand_built()])
def test_hand_built(name):
    _, res, links, o = sc.case_named(name)
    exp = _both(res, links, None, o, name)
    if name == "gap_in_a_piece":
        assert exp["seqs"][16:32] == exp["seqs"][16:20] + b"NNN" + exp["seqs"][23:32] and b"N" not in exp["seqs"][:20]
    if name == "one_unitig":
        assert exp["seqs"] == res["useqs"] and exp["status"][:2] == [1, 37]
    if name == "non_acgt_reversed":
        assert exp["layout"][1][1] == 1 and any(c in exp["seqs"][41:] for c in b"NRYacgt")


def test_chain_of_300_across_waves_and_workgroups():
    res, links, order, rev = sc.shuffled_chain(300, 5)
    exp = _both(res, links, None, {"insert_size": 100}, "chain of 300")
    assert exp["status"][0] == 1 and exp["status"][10] == 299
    got = [p[0] for p in exp["layout"]]
    assert got in (order, order[::-1]) and got[0] == min(order[0], order[-1])
    res, links, _, _ = sc.shuffled_chain(300, 6, lens=[random.Random(k).randint(1, 700) for k in range(300)])  # whole pieces in most unitigs
    _both(res, links, None, {"insert_size": 200}, "chain of 300, long unitigs")


# ---- contention ----
def test_one_end_with_300_links():
    res = sc.make_res([20] * 301, seed=4)
    many = [sc.link(1, 2 * u, count=4) for u in range(1, 301)]
    o = {"insert_size": 200}
    for ratio, weak, ambiguous in ((0, 0, 300), (1, 300, 0), (2, 0, 300)):  # ties: no link stands out, so none joins
        exp = _both(res, many, None, dict(o, link_ratio=ratio), "300 equal links, ratio %d" % ratio)
        assert (exp["status"][8], exp["status"][9], exp["status"][10], exp["status"][0]) == (weak, ambiguous, 0, 301)
    one = [sc.link(1, 2 * 150, count=9)] + many[:149] + many[150:]
    random.Random(1).shuffle(one)
    exp = _both(res, one, None, dict(o, link_ratio=2), "one link dominating 299")
    assert (exp["status"][8], exp["status"][9], exp["status"][10], exp["status"][0]) == (299, 0, 1, 300)


# ---- classes, gaps ----
def test_classes_in_precedence_order():
    res = sc.make_res([30, 40, 50, 60], circular=(3,), seed=3)
    o = {"insert_size": 100, "min_pairs": 2, "min_unitig_bases": 31}
    links = [(9, 2, 5, 1, 5), (2, 3, 1, 1, 1), (0, 6, 1, 1, 1), (1, 2, 1, 1, 1), (3, 4, 1, 50, 50), (3, 5, 2, 50, 100)]
    exp = _both(res, links, None, o, "one link per class")
    assert exp["status"][2:8] == [6, 1, 1, 1, 1, 1] and exp["status"][10] == 1
    for mb, joined in ((40, 1), (41, 0)):  # min_unitig_bases at exactly bases(u) and one above
        exp = _both(res, [sc.link(3, 4)], None, dict(o, min_unitig_bases=mb), "min_unitig_bases %d" % mb)
        assert exp["status"][10] == joined and exp["status"][6] == 1 - joined
    assert _both(res, [sc.link(3, 4, count=1)], None, dict(o, min_pairs=1), "min_pairs 1")["status"][10] == 1
    assert _both(res, [sc.link(3, 4, count=1)], None, o, "thin")["status"][7] == 1
    exp = _both(res, [sc.link(3, 4)] * 2, None, o, "a key given twice")
    assert exp["status"][9] == 2 and exp["status"][10] == 0


def test_gaps():
    res = sc.make_res([30, 40, 50], seed=12)
    big = (1 << 62) - 100
    for span, ins, gap, below, clamped in ((100, 100, 1, 1, 0), (99, 100, 1, 0, 0), (10, 100, 60, 0, 1), (big, big + 7, 7, 0, 0), (100, 90, 1, 1, 0)):
        exp = _both(res, [(3, 4, 2, 9, 2 * span + 1)], None, {"insert_size": ins, "max_gap": 60}, "span %d insert %d" % (span, ins))
        assert (max(exp["gaps"]), exp["status"][13], exp["status"][14], exp["status"][12]) == (gap, below, clamped, gap)
    exp = _both(res, [sc.link(1, 2, span=100)], None, {"insert_size": 103, "min_gap": 5, "max_gap": 5}, "lower clamp")
    assert (max(exp["gaps"]), exp["status"][13], exp["status"][14]) == (5, 1, 0)
    st24 = [7] * 24
    st24[14], st24[15] = 3, 500  # 166 and a remainder
    exp = _both(res, [sc.link(3, 4, span=100)], st24, {"insert_size": None}, "insert size from the status")
    assert max(exp["gaps"]) == 66
    st24[14] = 0
    exp = _both(res, [sc.link(3, 4, span=100)], st24, {"insert_size": None}, "no pair of the orientation")
    assert exp["status"][13] == 1 and max(exp["gaps"]) == 1


# ---- capacity ----
def test_capacity():
    _, res, links, o = sc.case_named("sizes_mixed")
    total = sc.expected_scaffolds(res, links, [0] * 24, o)["status"][1]
    exp = _device(res, links, [0] * 24, o, "one byte short", capacity=total - 1)
    assert exp["status"][15] == 1
    assert _device(res, links, [0] * 24, o, "exact", capacity=total)["status"][15] == 0
    assert _device(res, links, [0] * 24, o, "room to spare", capacity=total + 100)["status"][15] == 0
    assert _device(res, links, [0] * 24, o, "no bases asked for", seqs=False)["status"][15] == 1


# ---- hostile tables ----
def test_hostile_tables():
    res = sc.make_res([30, 40, 50, 20], seed=13)
    o = {"insert_size": 100}
    links = [sc.link(1, 2), (8, 9, 3, 1, 3), (2, 800, 3, 1, 3), (0xFFFFFFFF, 3, 3, 1, 3), (5, 4, 3, 1, 3), (3, 4, 0, 1, 3), (3, 5, 4, 1, 3)]
    exp = _both(res, links, None, o, "links beyond the unitigs, a > b, count 0")
    assert exp["status"][3] == 5 and exp["status"][4] == 0 and exp["status"][10] == 2  # 0 E - 1 B and 1 E - 2 E
    # counts on the device above their capacities are taken as the capacities
    exp = _device(res, links, [0] * 24, o, "counts beyond the capacities", nu_dev=1 << 40, nl_dev=1 << 33)
    assert exp["status"][0] == 2 and exp["status"][2] == len(links)
    # and counts below them leave the rest of the tables unread
    exp = _device(res, links, [0] * 24, o, "fewer unitigs and links than room", nu_dev=2, nl_dev=1)
    assert exp["status"][:3] == [1, 71, 1] and len(exp["layout"]) == 2
    # seq_offs that do not ascend: bases(u) wraps; the call ends, the layout is the rules', and nothing behind a buffer is written
    bad = dict(res, seq_offs=[0, 30, 10, 120, 90])
    joined = [sc.link(1, 2), sc.link(3, 4), sc.link(5, 6)]
    exp = _device(bad, joined, [0] * 24, o, "descending seq_offs", seqs=False)
    assert exp["status"][10] == 3
    bad = dict(res, seq_offs=[0, 30, 10, 120, 150])  # ... and a total that fits, whatever lies between
    from siga_amd import _lib
    L = _lib.lib()
    counts = _up(np.array([4, 3], dtype=np.uint64))
    d_so, d_uf, d_us = _up(np.array(bad["seq_offs"], dtype=np.uint64)), _up(np.array(bad["uflags"], dtype=np.uint32)), _up(bad["useqs"])
    d_links = _up(_links_array(joined))
    for cap in (0, 150, 453, 1 << 16):
        d, sizes = _enqueue(L, 4, 3, counts.data_ptr(), d_so.data_ptr(), d_uf.data_ptr(), d_us.data_ptr(), len(bad["useqs"]), d_links.data_ptr(),
                            counts.data_ptr() + 8, None, o, cap, None)
        torch.cuda.synchronize()
        h = {k: v.cpu().numpy() for k, v in d.items()}
        for k, v in sizes.items():
            assert h[k][v:].tobytes() == b"\xee" * CANARY, (cap, k)
        exp = sc.expected_scaffolds({k: v for k, v in bad.items() if k != "useqs"}, joined, [0] * 24, o, sseqs_capacity=cap)
        assert h["status"][:128].view(np.uint64).tolist() == exp["status"], cap
        if exp["status"][15]:
            assert h["seqs"].tobytes() == b"\xee" * (cap + CANARY)


def test_no_unitigs_and_no_links():
    import siga_amd
    from siga_amd import _lib
    none = {"seq_offs": [0], "uflags": [], "useqs": b""}
    got = siga_amd.unitigs_scaffold(none, [], insert_size=100)
    assert got["status"].tolist() == [0] * 16 and got["sc_offs"].tolist() == [0] and len(got["layout"]) == 0 and len(got["seqs"]) == 0
    st = _out(128)
    opts = _sopts({"insert_size": 5})
    assert _lib.lib().sigax_scaffold_device(0, None, 0, None, None, None, 0, None, None, 0, None, C.byref(opts), None, None, None, None, None, 0,
                                            st.data_ptr(), None, 0, None) == 0
    torch.cuda.synchronize()
    assert st.cpu().numpy().tobytes() == b"\0" * 128 + b"\xee" * CANARY
    res = sc.make_res([17, 5, 40], circular=(1,), seed=14)
    exp = _both(res, [], None, {"insert_size": 100}, "no links")
    assert exp["status"][0] == 3 and exp["seqs"] == res["useqs"]


# ---- the three calls on one stream ----
def _host_chimeric(case):
    import siga_amd
    edges, lengths, seqs, offs = uc.arrays(case)
    return siga_amd.unitigs_chimeric(edges, lengths, seqs, offs, case["m"], case["x"], case["L"], case["C"], delta=case["delta"],
                                     careful=case["careful"], num_reads=case["N"], genome_size=case["G"], uniq_threshold=case["T"],
                                     min_chimeric_length=case["Lc"], min_chimeric_coverage=case["Ac"], chimeric_delta=case["delta_c"],
                                     chimeric_threshold=case["Tc"], graph=False)


def _chained(case, o, capacity, what):
    """sigax_unitigs_chimeric_device, sigax_unitigs_pairs_device and sigax_scaffold_device enqueued on one stream, nothing in
    between: the scaffold call reads both counts, the tables, the bases, the links and the pairs status where the calls before
    it leave them -> its result"""
    from siga_amd import _lib
    from tests import test_gpu_unitig_pairs as tp
    L = _lib.lib()
    edges, lengths, seqs, offs = uc.arrays(case)
    n, ne, nb = len(lengths), len(edges), len(seqs)
    d_edges, d_len, d_seqs, d_offs = _up(edges), _up(lengths), _up(seqs), _up(offs)
    d_mate = _up(np.array(case["mate"], dtype=np.uint32))
    wb = C.c_uint64()
    assert L.sigax_unitigs_chimeric_workspace(n, ne, 0, int(case["careful"]), C.byref(wb)) == 0
    u = {k: _out(v) for k, v in {"seq_offs": 8 * (n + 1), "lay_offs": 8 * (n + 1), "uflags": 4 * n, "layout": 16 * n, "useqs": nb, "removed": 4 * n,
                                 "cut": 4 * ne, "status": 160, "work": wb.value}.items()}
    st = tp._stream()
    torch.cuda.synchronize()
    try:
        prune = _lib.PruneOpts(case["x"], case["L"], _lib.SIGAX_TRIM_NO_COVERAGE if case["C"] is None else case["C"], case["delta"],
                               int(case["careful"]), 0, case["N"], case["G"], case["T"])
        copts = _lib.ChimericOpts(prune, case["Lc"], _lib.SIGAX_TRIM_NO_COVERAGE if case["Ac"] is None else case["Ac"], case["delta_c"], 0, case["Tc"])
        rc = L.sigax_unitigs_chimeric_device(0, d_edges.data_ptr(), ne, d_len.data_ptr(), d_seqs.data_ptr(), d_offs.data_ptr(), n, case["m"],
                                             C.byref(copts), u["seq_offs"].data_ptr(), u["lay_offs"].data_ptr(), u["uflags"].data_ptr(),
                                             u["layout"].data_ptr(), u["useqs"].data_ptr(), u["removed"].data_ptr(), u["cut"].data_ptr(), None,
                                             u["status"].data_ptr(), u["work"].data_ptr(), wb.value, st)
        assert rc == 0, _lib.last_error()
        p, _ = tp._enqueue_pairs(L, n, d_mate, d_len, u["status"].data_ptr(), u["seq_offs"].data_ptr(), u["lay_offs"].data_ptr(),
                                 u["uflags"].data_ptr(), u["layout"].data_ptr(), {"max_span": 0}, st)
        d, sizes = _enqueue(L, n, n // 2, u["status"].data_ptr(), u["seq_offs"].data_ptr(), u["uflags"].data_ptr(), u["useqs"].data_ptr(), nb,
                            p["links"].data_ptr() if n // 2 else None, p["status"].data_ptr() + 22 * 8, p["status"].data_ptr(), o, capacity, st)
        torch.cuda.synchronize()
    finally:
        L.sigax_stream_destroy(0, st)
    nu = int(u["status"].cpu().numpy()[:8].view(np.uint64)[0])
    return _collect(d, sizes, nu, what)


def _through_the_calls(seed):
    """graph `seed` through the host forms of the unitig call and the pairs call -> (case, res, the pairs result, options)"""
    import siga_amd
    case = pp.random_case(seed)
    res = _host_chimeric(case)
    pairs = siga_amd.unitigs_pairs(res, [len(r) for r in case["reads"]], case["mate"], max_span=0)
    return case, res, pairs, sc.pipeline_options(seed)


def test_three_calls_on_one_stream():
    for seed in (3, 7, 18):
        case, res, pairs, o = _through_the_calls(seed)
        exp = sc.expected_scaffolds(res, pairs["links"], pairs["status"], o)
        got = _chained(case, o, exp["status"][1], case["name"])
        _same(got, exp, case["name"] + ", chained")


def test_random_graphs_through_the_calls():
    import siga_amd
    seen = [0] * 16
    for seed in range(100):
        case, res, pairs, o = _through_the_calls(seed)
        extra = sc.pipeline_extra_links(seed, len(res["uflags"]), sc._plain(pairs["links"]))
        links = sc._plain(pairs["links"]) + extra
        exp = sc.expected_scaffolds(res, links, pairs["status"], o)
        got = siga_amd.unitigs_scaffold(res, _links_array(links), status=pairs["status"], **o)
        _same(got, exp, case["name"] + ", host")
        _device(res, links, [int(x) for x in pairs["status"]], o, case["name"])
        if not extra:
            _same(_chained(case, o, exp["status"][1], case["name"]), exp, case["name"] + ", chained")
        seen = [a + b for a, b in zip(seen, exp["status"])]
    print("over the 100 graphs", seen)
    assert all(seen[k] > 0 for k in (4, 7, 8, 9, 10, 13)), seen


# ---- refusals ----
def test_refusals():
    from siga_amd import _lib
    L = _lib.lib()
    E = _lib.SIGAX_E_ARG
    wb = C.c_uint64()
    assert L.sigax_scaffold_workspace(1 << 31, 10, C.byref(wb)) == E and "max_unitigs" in _lib.last_error()
    assert L.sigax_scaffold_workspace(10, 1 << 32, C.byref(wb)) == E and "max_links" in _lib.last_error()
    assert L.sigax_scaffold_workspace(10, 10, None) == E
    assert L.sigax_scaffold_workspace(0, 0, C.byref(wb)) == 0 and wb.value == 0
    mu, ml = 8, 4
    assert L.sigax_scaffold_workspace(mu, ml, C.byref(wb)) == 0
    b = [torch.zeros(4096, dtype=torch.uint8, device="cuda:0") for _ in range(13)]
    p = [t.data_ptr() for t in b]
    work = torch.zeros(wb.value, dtype=torch.uint8, device="cuda:0")
    z = None
    names = ("nu", "so", "uf", "us", "links", "nl", "st24", "sco", "scl", "scf", "lay", "seqs", "st16")
    full = {"nu": "d_n_unitigs", "so": "d_seq_offs", "uf": "d_uflags", "us": "d_useqs", "links": "d_links", "nl": "d_n_links", "st24": "d_status24",
            "sco": "d_sc_offs", "scl": "d_sc_lay_offs", "scf": "d_sc_flags", "lay": "d_sc_layout", "seqs": "d_sseqs", "st16": "d_status16"}

    def opts(flags=1, min_pairs=2, ratio=0, mb=0, ins=0, min_gap=1, max_gap=100):
        return C.byref(_lib.ScaffoldOpts(flags, min_pairs, ratio, mb, ins, min_gap, max_gap))

    def dev(o="usual", w=work.data_ptr(), nbytes=wb.value, nmu=mu, nml=ml, cap=64, **over):
        a = dict(zip(names, p))
        a.update(over)
        return L.sigax_scaffold_device(0, a["nu"], nmu, a["so"], a["uf"], a["us"], 4096, a["links"], a["nl"], nml, a["st24"], opts() if o == "usual" else o,
                                       a["sco"], a["scl"], a["scf"], a["lay"], a["seqs"], cap, a["st16"], w, nbytes, z)

    assert dev(o=None) == E
    assert dev(o=opts(flags=2)) == E and "flags" in _lib.last_error()
    assert dev(o=opts(flags=1, ins=5)) == E and "insert_size" in _lib.last_error()
    assert dev(o=opts(flags=0, ins=1 << 62)) == E and "insert_size" in _lib.last_error()
    assert dev(o=opts(min_gap=0)) == E and "min_gap" in _lib.last_error()
    assert dev(o=opts(min_gap=5, max_gap=4)) == E and "max_gap" in _lib.last_error()
    assert dev(o=opts(max_gap=1 << 31)) == E and "max_gap" in _lib.last_error()
    assert dev(nmu=1 << 31) == E and "max_unitigs" in _lib.last_error()
    assert dev(nml=1 << 32) == E and "max_links" in _lib.last_error()
    assert dev(cap=1 << 43) == E and "sseqs_capacity" in _lib.last_error()
    assert dev(nbytes=wb.value - 1) == E and "workspace" in _lib.last_error()
    for k in names:
        if k != "seqs":
            assert dev(**{k: z}) == E and full[k] in _lib.last_error(), k
    assert dev(seqs=z) == E and "d_sseqs" in _lib.last_error()  # NULL with a capacity
    assert dev(seqs=z, cap=0) == 0 and dev(seqs=z, us=z, cap=0) == 0  # the layout alone
    assert dev(o=opts(flags=0, ins=7), st24=z) == 0 and dev(links=z, nl=z, nml=0) == 0
    assert dev(w=z) == E and "d_work" in _lib.last_error()
    for k, off in (("uf", 2), ("scf", 2), ("nu", 4), ("so", 4), ("links", 4), ("nl", 4), ("st24", 4), ("sco", 4), ("scl", 4), ("st16", 4), ("lay", 8),
                   ("us", 8), ("seqs", 8)):
        assert dev(**{k: p[0] + 2048 + off}) == E and "aligned" in _lib.last_error() and full[k] in _lib.last_error(), k
    assert dev(w=work.data_ptr() + 8) == E and "aligned" in _lib.last_error()
    assert dev() == 0, _lib.last_error()  # (everything zero: no unitigs)
    torch.cuda.synchronize()
    assert b[names.index("st16")].cpu().numpy()[:128].view(np.uint64).tolist() == [0] * 16
    # the host form
    ns = C.c_uint64()
    ptrs = [C.c_void_p() for _ in range(5)]
    s16 = (C.c_uint64 * 16)()
    so, uf = (C.c_uint64 * 3)(0, 5, 9), (C.c_uint32 * 2)()
    us = C.create_string_buffer(b"ACGTACGTA")

    def host(o, nu=2, so_=so, uf_=uf, us_=us, links=z, nl=0, st24=z, ns_=C.byref(ns), out=None, s16_=s16):
        out = [C.byref(x) for x in ptrs] if out is None else out
        return L.sigax_scaffold_host(0, nu, so_, uf_, us_, links, nl, st24, o, ns_, out[0], out[1], out[2], out[3], out[4], s16_)

    def free():
        for x in ptrs:
            L.sigax_free(x)

    assert host(opts(flags=0, ins=9)) == 0 and ns.value == 2 and list(s16)[:2] == [2, 9]
    free()
    assert host(None) == E and host(opts(flags=0, min_gap=0)) == E
    assert host(opts()) == E and "status24" in _lib.last_error()  # from the status, and none given
    assert host(opts(flags=0), ns_=None) == E and host(opts(flags=0), s16_=None) == E
    assert host(opts(flags=0), out=[None] + [C.byref(x) for x in ptrs[1:]]) == E
    assert host(opts(flags=0), so_=z) == E and host(opts(flags=0), uf_=z) == E
    assert host(opts(flags=0), us_=z) == E and "useqs" in _lib.last_error()
    assert host(opts(flags=0), nl=3) == E and "links" in _lib.last_error()
    assert host(opts(flags=0), nu=1 << 31) == E
    assert host(opts(flags=0), us_=z, out=[C.byref(x) for x in ptrs[:4]] + [None]) == 0  # the layout alone
    free()
    assert host(opts(flags=0), nu=0, so_=z, uf_=z, us_=z) == 0 and ns.value == 0 and list(s16) == [0] * 16
    free()


# ---- the command line, once: a genome with a repeat of two copies that breaks the unitigs and that the pairs span ----
E2E_GENOME, E2E_LEN, E2E_INSERT, E2E_REPEAT, E2E_STEP, E2E_M = 6000, 60, 400, 150, 6, 25


@functools.lru_cache(maxsize=None)
def _e2e(seed):
    """-> (genome, names, reads): a read pair every E2E_STEP bases, the mates in random order"""
    rng = random.Random(seed)
    while True:
        g = bytearray(rng.choice(b"ACGT") for _ in range(E2E_GENOME))
        g[4000:4000 + E2E_REPEAT] = g[1500:1500 + E2E_REPEAT]
        g = bytes(g)
        masked = g[:4000] + g[4000 + E2E_REPEAT:]
        if not uc.longest_repeat_at_least(masked, E2E_M):
            break
    names, reads = [], []
    for k, p in enumerate(range(0, E2E_GENOME - E2E_INSERT + 1, E2E_STEP)):
        fwd, back = g[p:p + E2E_LEN], uc.revcomp(g[p + E2E_INSERT - E2E_LEN:p + E2E_INSERT])
        if rng.random() < 0.5:
            fwd, back = back, fwd
        names += ["pair%d/1" % k, "pair%d/2" % k]
        reads += [fwd, back]
    return g, names, reads


def _e2e_files(seed):
    d = os.path.join(CACHE, "unitig_scaffold_e2e_%d" % seed)
    os.makedirs(d, exist_ok=True)
    prefix = os.path.join(d, "reads")
    _, names, reads = _e2e(seed)
    if not all(os.path.exists(prefix + e) for e in (".bwt", ".rbwt", ".sai", ".rsai", ".fa")):
        seqs = [s.decode() for s in reads]
        po.Index.build(seqs).save(prefix + ".bwt", prefix + ".sai")
        po.Index.build(seqs, reverse=True).save(prefix + ".rbwt", prefix + ".rsai")
        with open(prefix + ".fa", "w") as f:
            f.write(mr.fasta_text(list(zip(names, seqs))))
    return prefix


E2E_SEED, E2E_MIN_UNITIG = 21, 300


def _matches(scaffold, text):
    """does `scaffold`, its N taken as wildcards, occur in `text`?"""
    import re
    return re.search(b"".join(b"." if c == 78 else re.escape(bytes([c])) for c in scaffold), text, re.S) is not None


def test_cli(tmp_path):
    import siga_amd
    from siga_amd import host
    prefix = _e2e_files(E2E_SEED)
    genome, names, reads = _e2e(E2E_SEED)
    fa0, fa, lay, pj, lk, sfa, slay = (str(tmp_path / f) for f in ("plain.fa", "u.fa", "u.layout", "u.pairs.json", "u.links", "s.fa", "s.layout"))
    base = [host.CLI_PATH, "unitig", "-m", str(E2E_M), "-p", prefix]
    r = subprocess.run(base + ["-o", fa0, prefix + ".fa"], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    r = subprocess.run(base + ["-o", fa, "--layout", lay, "--pairs", pj, "--links", lk, "--scaffold", sfa, "--scaffold-layout", slay, "--insert-size",
                               str(E2E_INSERT), "--min-scaffold-unitig", str(E2E_MIN_UNITIG), prefix + ".fa"], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    assert open(fa, "rb").read() == open(fa0, "rb").read() and b"scaffolds" in r.stderr and b"gap bases" in r.stderr
    # the unitigs as the layout and the FASTA give them, the links as the restatement of the pairs call gives them
    ids = {n: i for i, n in enumerate(names)}
    lines = open(fa).read().split("\n")
    useqs = [l.strip().encode() for l in lines[1::2] if l.strip()]
    res = {"seq_offs": [0], "lay_offs": [0], "uflags": [uc.CIRCULAR if "circular=" in h else 0 for h in lines if h.startswith(">")], "layout": [],
           "useqs": b"".join(useqs)}
    for b in useqs:
        res["seq_offs"].append(res["seq_offs"][-1] + len(b))
    per = [0] * len(useqs)
    for line in open(lay).read().splitlines():
        u, name, strand, off = line.split("\t")
        per[int(u.split("-")[1])] += 1
        res["layout"].append((ids[name], uc.PLACED_REV if strand == "-" else 0, int(off)))
    for c in per:
        res["lay_offs"].append(res["lay_offs"][-1] + c)
    pairs = pp.expected_pairs(res, [len(s) for s in reads], siga_amd.mates_by_name(names), {})
    want = "".join("LK\tunitig-%d\t%s\tunitig-%d\t%s\t%d\t%d\t%d\n" % (a >> 1, "BE"[a & 1], b >> 1, "BE"[b & 1], c, mn, sm)
                   for a, b, c, mn, sm in pairs["links"])
    assert open(lk).read() == want
    o = {"insert_size": E2E_INSERT, "min_unitig_bases": E2E_MIN_UNITIG}
    exp = sc.expected_scaffolds(res, pairs["links"], pairs["status"], o)
    repeat = genome[1500:1500 + E2E_REPEAT]
    inside = [len(s) for s in useqs if s in repeat or uc.revcomp(s) in repeat or repeat in s or repeat in uc.revcomp(s)]
    print("unitigs", [len(s) for s in useqs], "in or over the repeat", inside, "status", exp["status"], "gaps", exp["gaps"])
    assert inside and max(inside) < E2E_MIN_UNITIG  # the option lies above the repeat unitig's length
    joined = [s for s in range(exp["status"][0]) if exp["sc_lay_offs"][s + 1] - exp["sc_lay_offs"][s] >= 2]
    assert joined and all(g > 1 for g in exp["gaps"] if g), exp["gaps"]  # every gap above min_gap
    efa, elay = sc.render(exp)
    assert open(sfa).read() == efa and open(slay).read() == elay
    # one exact insert: the gap estimates are exact, so every scaffold lies in the genome with its N as wildcards
    both = genome + b"\n" + uc.revcomp(genome)
    for s in range(exp["status"][0]):
        assert _matches(exp["seqs"][exp["sc_offs"][s]:exp["sc_offs"][s + 1]], both), s
    # the insert size from the pairs call gives the same scaffolds here: every pair inside a unitig spans the insert
    r = subprocess.run(base + ["-o", fa, "--pairs", pj, "--scaffold", sfa, "--min-scaffold-unitig", str(E2E_MIN_UNITIG), prefix + ".fa"],
                       capture_output=True)
    assert r.returncode == 0 and open(sfa).read() == efa, r.stderr.decode()
    # refusals and the help text
    r = subprocess.run(base + ["-o", fa, "--scaffold", sfa, prefix + ".fa"], capture_output=True)
    assert r.returncode == 1 and b"--pairs" in r.stderr
    for opt in (["--scaffold-layout", slay], ["--min-pairs", "3"], ["--link-ratio", "2"], ["--min-scaffold-unitig", "9"], ["--insert-size", "400"],
                ["--min-gap", "2"], ["--max-gap", "50"]):
        r = subprocess.run(base + ["-o", fa, "--pairs", pj] + opt + [prefix + ".fa"], capture_output=True)
        assert r.returncode == 1 and b"--scaffold" in r.stderr, opt
    r = subprocess.run(base, capture_output=True)  # no READSFILE: the help text
    assert r.returncode == 0 and all(w in r.stdout for w in (b"--scaffold=FILE", b"--scaffold-layout=FILE", b"--min-pairs", b"--link-ratio",
                                                              b"--min-scaffold-unitig", b"--insert-size", b"--min-gap", b"--max-gap"))
