"""Mate-pair statistics and links of `siga unitig --pairs` on the GPU (csrc/sigax_pairs.hip) against the serial restatement of
its rules (tests/pair_cases.py::expected_pairs): the host form, and the device form enqueued on one stream straight behind the
unitig call that feeds it, its count of unitigs read from that call's status block on the device; synthetic layouts for what no
small graph gives (distances near 2^32, hostile tables); canaries behind every output; refusals; the command line once."""
import ctypes as C
import functools
import json
import os
import random
import subprocess

import numpy as np
import pytest
import torch  # before the library loads: one HIP runtime per process

from oracle import pyoracle as po
from tests import chimeric_cases as cc
from tests import pair_cases as pp
from tests import unitig_cases as uc
from tests.fixtures import CACHE
from tests.golden import make_reads as mr

pytestmark = pytest.mark.gpu
CANARY = 64
NO = pp.NO_MATE


def _popts(o=None):
    from siga_amd import _lib
    o = dict(pp.DEFAULT_OPTS, **(o or {}))
    return _lib.PairsOpts(_lib.SIGAX_PAIRS_OUTWARD if o["outward"] else 0, o["hist_bins"], o["hist_shift"], 0, o["max_span"])


def _same(got, exp, what):
    """got: dict(status, hist, links) of arrays; exp: expected_pairs()'s"""
    print(what, "status", [int(x) for x in got["status"]], "expected", exp["status"])
    assert [int(x) for x in got["status"]] == exp["status"], what
    assert [int(x) for x in got["hist"]] == exp["hist"], what
    assert [tuple(int(x) for x in r) for r in got["links"].tolist()] == exp["links"], what


def _untouched(tails, what):
    for k, t in tails.items():
        assert t == b"\xee" * len(t), "%s: bytes after %s were written" % (what, k)


def _up(a):
    dev = torch.device("cuda:0")
    a = np.frombuffer(a, dtype=np.uint8) if isinstance(a, bytes) else np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return torch.from_numpy(a.copy()).to(dev) if a.size else torch.zeros(16, dtype=torch.uint8, device=dev)


def _out(nbytes):
    return torch.full((nbytes + CANARY,), 0xEE, dtype=torch.uint8, device="cuda:0")


def _enqueue_pairs(L, n, d_mate, d_len, nu_ptr, so_ptr, lo_ptr, uf_ptr, lay_ptr, o, stream):
    """sigax_unitigs_pairs_device over output buffers of exactly their size plus CANARY bytes of 0xEE -> (buffers, sizes)"""
    o = dict(pp.DEFAULT_OPTS, **(o or {}))
    wb = C.c_uint64()
    assert L.sigax_unitigs_pairs_workspace(0, n, C.byref(wb)) == 0
    sizes = {"hist": 8 * o["hist_bins"], "links": 24 * (n // 2), "status": 192, "work": wb.value}
    d = {k: _out(v) for k, v in sizes.items()}
    torch.cuda.synchronize()
    opts = _popts(o)
    rc = L.sigax_unitigs_pairs_device(0, d_mate.data_ptr(), d_len.data_ptr(), n, nu_ptr, so_ptr, lo_ptr, uf_ptr, lay_ptr, C.byref(opts),
                                      d["hist"].data_ptr(), d["links"].data_ptr(), d["status"].data_ptr(), d["work"].data_ptr(), wb.value, stream)
    from siga_amd import _lib
    assert rc == 0, _lib.last_error()
    return d, sizes


def _collect(d, sizes, n):
    from siga_amd import _lib
    h = {k: v.cpu().numpy() for k, v in d.items()}
    status = h["status"][:192].view(np.uint64)
    recs = int(status[22])
    assert recs <= n // 2
    got = {"status": status, "hist": h["hist"][:sizes["hist"]].view(np.uint64), "links": h["links"][:24 * recs].view(_lib.PAIR_LINK_DTYPE)}
    tails = {k: h[k][sizes[k]:].tobytes() for k in sizes}
    tails["links_rest"] = h["links"][24 * recs:sizes["links"]].tobytes()
    return got, tails


def _stream():
    from siga_amd import _lib
    st = C.c_void_p()
    assert _lib.lib().sigax_stream_create(0, C.byref(st)) == 0
    return st


def _chained(case, o=None, chimeric=False):
    """the unitig call (sigax_unitigs_device, or sigax_unitigs_chimeric_device with the case's round options) and the pairs call
    enqueued behind it on one stream, nothing in between -> (the pairs result, tails)"""
    from siga_amd import _lib
    L = _lib.lib()
    edges, lengths, seqs, offs = uc.arrays(case)
    n, ne, nb = len(lengths), len(edges), len(seqs)
    d_edges, d_len, d_seqs, d_offs = _up(edges), _up(lengths), _up(seqs), _up(offs)
    d_mate = _up(np.array(case["mate"], dtype=np.uint32))
    wb = C.c_uint64()
    if chimeric:
        assert L.sigax_unitigs_chimeric_workspace(n, ne, 0, int(case["careful"]), C.byref(wb)) == 0
    else:
        assert L.sigax_unitigs_workspace(n, ne, C.byref(wb)) == 0
    u = {k: _out(v) for k, v in {"seq_offs": 8 * (n + 1), "lay_offs": 8 * (n + 1), "uflags": 4 * n, "layout": 16 * n, "useqs": nb, "removed": 4 * n,
                                 "cut": 4 * ne, "status": 160, "work": wb.value}.items()}
    st = _stream()
    torch.cuda.synchronize()
    try:
        if chimeric:
            prune = _lib.PruneOpts(case["x"], case["L"], _lib.SIGAX_TRIM_NO_COVERAGE if case["C"] is None else case["C"], case["delta"],
                                   int(case["careful"]), 0, case["N"], case["G"], case["T"])
            copts = _lib.ChimericOpts(prune, case["Lc"], _lib.SIGAX_TRIM_NO_COVERAGE if case["Ac"] is None else case["Ac"], case["delta_c"], 0,
                                      case["Tc"])
            rc = L.sigax_unitigs_chimeric_device(0, d_edges.data_ptr(), ne, d_len.data_ptr(), d_seqs.data_ptr(), d_offs.data_ptr(), n, case["m"],
                                                 C.byref(copts), u["seq_offs"].data_ptr(), u["lay_offs"].data_ptr(), u["uflags"].data_ptr(),
                                                 u["layout"].data_ptr(), u["useqs"].data_ptr(), u["removed"].data_ptr(), u["cut"].data_ptr(), None,
                                                 u["status"].data_ptr(), u["work"].data_ptr(), wb.value, st)
        else:
            rc = L.sigax_unitigs_device(0, d_edges.data_ptr(), ne, d_len.data_ptr(), d_seqs.data_ptr(), d_offs.data_ptr(), n, case["m"],
                                        u["seq_offs"].data_ptr(), u["lay_offs"].data_ptr(), u["uflags"].data_ptr(), u["layout"].data_ptr(),
                                        u["useqs"].data_ptr(), u["status"].data_ptr(), u["work"].data_ptr(), wb.value, st)
        assert rc == 0, _lib.last_error()
        d, sizes = _enqueue_pairs(L, n, d_mate, d_len, u["status"].data_ptr(), u["seq_offs"].data_ptr(), u["lay_offs"].data_ptr(),
                                  u["uflags"].data_ptr(), u["layout"].data_ptr(), o, st) if n else (None, None)
        torch.cuda.synchronize()
    finally:
        L.sigax_stream_destroy(0, st)
    return _collect(d, sizes, n)


def _both(case, exp_unitigs, o=None, chimeric=False, what=None):
    """the host form over `exp_unitigs` (the serial unitigs) and the chained device form, against expected_pairs"""
    import siga_amd
    what = what or case["name"]
    lengths = [len(r) for r in case["reads"]]
    exp = pp.expected_pairs(exp_unitigs, lengths, case["mate"], o)
    oo = dict(pp.DEFAULT_OPTS, **(o or {}))
    got = siga_amd.unitigs_pairs(exp_unitigs, lengths, case["mate"], **oo)
    _same(got, exp, what + ", host")
    assert (got["insert_size"], got["delta"], got["span_mean"], got["span_sd"]) == (exp["insert_size"], exp["delta"], exp["span_mean"], exp["span_sd"])
    res, tails = _chained(case, o, chimeric)
    _same(res, exp, what + ", device")
    _untouched(tails, what)
    return exp


# ---- synthetic layouts handed straight to the pairs call ----
def _layout(unitigs):
    """unitigs: [(bases, circular, [(read, rev, offset)])] -> the dict a unitig call returns"""
    seq_offs, lay_offs, uflags, layout = [0], [0], [], []
    for bases, circular, placed in unitigs:
        layout += [(r, uc.PLACED_REV if rev else 0, off) for r, rev, off in placed]
        seq_offs.append(seq_offs[-1] + bases)
        lay_offs.append(len(layout))
        uflags.append(uc.CIRCULAR if circular else 0)
    return {"seq_offs": seq_offs, "lay_offs": lay_offs, "uflags": uflags, "layout": layout}


def _mates(n, pairs, extra=None):
    mate = [NO] * n
    for a, b in pairs:
        mate[a], mate[b] = b, a
    for i, v in (extra or {}).items():
        mate[i] = v
    return mate


def _direct(res, lengths, mate, o=None, what="", host=True, n_unitigs_dev=None):
    """res handed to the device form in buffers of the sizes the unitig calls use (n + 1 offsets, n flags, n placements: what
    lies beyond the result is padded, offsets with their last value) and, unless it is refused there, to the host form"""
    from siga_amd import _lib
    import siga_amd
    L = _lib.lib()
    n, nu = len(lengths), len(res["uflags"])
    so = np.full(n + 1, res["seq_offs"][-1], dtype=np.uint64)
    so[:len(res["seq_offs"])] = res["seq_offs"]
    lo = np.full(n + 1, res["lay_offs"][-1], dtype=np.uint64)
    lo[:len(res["lay_offs"])] = res["lay_offs"]
    uf = np.zeros(max(n, 1), dtype=np.uint32)
    uf[:nu] = res["uflags"]
    lay = np.zeros(max(n, 1), dtype=_lib.PLACEMENT_DTYPE)
    lay[:len(res["layout"])] = np.array([tuple(p) for p in res["layout"]], dtype=_lib.PLACEMENT_DTYPE)
    padded = {"seq_offs": so, "lay_offs": lo, "uflags": uf[:n], "layout": lay}
    exp = pp.expected_pairs(padded, lengths, mate, o, n_unitigs=nu if n_unitigs_dev is None else n_unitigs_dev)
    if host:
        assert exp["status"] == pp.expected_pairs(res, lengths, mate, o)["status"]
        oo = dict(pp.DEFAULT_OPTS, **(o or {}))
        got = siga_amd.unitigs_pairs({"seq_offs": so[:nu + 1], "lay_offs": lo[:nu + 1], "uflags": uf[:nu], "layout": lay[:len(res["layout"])]}, lengths,
                                     mate, **oo)
        _same(got, exp, what + ", host")
    d_nu = _up(np.array([nu if n_unitigs_dev is None else n_unitigs_dev], dtype=np.uint64))
    d_mate, d_len = _up(np.array(mate, dtype=np.uint32)), _up(np.array(lengths, dtype=np.uint32))
    d_so, d_lo, d_uf, d_lay = _up(so), _up(lo), _up(uf), _up(lay)
    d, sizes = _enqueue_pairs(L, n, d_mate, d_len, d_nu.data_ptr(), d_so.data_ptr(), d_lo.data_ptr(), d_uf.data_ptr(), d_lay.data_ptr(), o, None)
    torch.cuda.synchronize()
    got, tails = _collect(d, sizes, n)
    _same(got, exp, what + ", device")
    _untouched(tails, what)
    return exp


def test_no_mates_and_no_reads():
    import siga_amd
    case = dict(uc.hand_built()[3])
    case["mate"] = [NO] * len(case["reads"])
    exp = _both(case, uc.expected(case["reads"], case["edges"], case["m"]))
    assert exp["status"] == [0] * 24 and exp["links"] == []
    none = {"seq_offs": [0], "lay_offs": [0], "uflags": [], "layout": np.zeros(0, dtype=siga_amd._lib.PLACEMENT_DTYPE)}
    got = siga_amd.unitigs_pairs(none, [], [], hist_bins=7)
    assert got["status"].tolist() == [0] * 24 and got["hist"].tolist() == [0] * 7 and len(got["links"]) == 0
    assert (got["insert_size"], got["delta"], got["span_mean"], got["span_sd"]) == (0, 0, 0.0, 0.0)
    from siga_amd import _lib
    st, hist = _out(192), _out(56)
    opts = _popts({"hist_bins": 7})
    assert _lib.lib().sigax_unitigs_pairs_device(0, None, None, 0, None, None, None, None, None, C.byref(opts), hist.data_ptr(), None, st.data_ptr(),
                                                 None, 0, None) == 0
    torch.cuda.synchronize()
    assert st.cpu().numpy().tobytes() == b"\0" * 192 + b"\xee" * CANARY and hist.cpu().numpy().tobytes() == b"\0" * 56 + b"\xee" * CANARY


@pytest.mark.parametrize("rc,entry", [((False, True), 5), ((True, False), 6), ((False, False), 7), ((True, True), 7)],
                         ids=["inward", "outward", "tandem_forward", "tandem_reversed"])
def test_two_reads_in_one_unitig(rc, entry):
    b = uc._Build(900 + entry + int(rc[0]))
    ids = b.chain(2, lens=[60, 60], rc=list(rc))
    case = pp._with(b, "two_reads", [(ids[0], ids[1])])
    for outward in (False, True):
        exp = _both(case, uc.expected(case["reads"], case["edges"], case["m"]), {"outward": outward}, what="two reads %s outward=%s" % (rc, outward))
        assert exp["status"][2] == exp["status"][4] == exp["status"][entry] == exp["status"][10] == 1
        assert exp["status"][14] == (entry == (6 if outward else 5)) and sum(exp["hist"]) == exp["status"][14]


@pytest.mark.parametrize("name", ["ring", "singles", "two_chains", "branch", "chain_mixed", "containment", "unequal_flip"])
def test_hand_built_graphs(name):
    case = pp.case_named(name)
    for o in ({}, {"outward": True, "hist_bins": 64, "hist_shift": 2}):
        exp = _both(case, uc.expected(case["reads"], case["edges"], case["m"]), o, what="%s %s" % (name, o))
    if name == "ring":  # a pair in the ring of three, a link into it, a pair beside it
        assert exp["status"][8] == 1 and exp["status"][19] == 1 and exp["status"][4] == 1 and exp["links"] == []
    if name == "singles":  # two malformed entries: self, out of range
        assert exp["status"][1] == 2 and exp["status"][18] == 2 and len(exp["links"]) == 2


def test_a_mate_a_round_removed():
    base = cc.case_named("bridge")
    exp_u = cc.expected_of("bridge")
    gone = [r for r, x in enumerate(exp_u["removed"]) if x]
    kept = [r for r, x in enumerate(exp_u["removed"]) if not x]
    assert gone and len(exp_u["layout"]) == len(kept) < len(base["reads"])
    case = dict(base, mate=_mates(len(base["reads"]), [(gone[0], kept[0]), (kept[1], kept[2])]))
    exp = _both(case, exp_u, chimeric=True)
    assert exp["status"][2] == 2 and exp["status"][3] == 1


def test_more_malformed_entries_than_pairs():
    res = _layout([(300, False, [(r, False, 20 * r) for r in range(10)])])
    mate = _mates(10, [(0, 9)], {1: 1, 2: 10, 3: 0xFFFFFFFE, 4: 0, 5: 6, 6: 7, 7: 5})  # self, out of range, and not reciprocal
    exp = _direct(res, [100] * 10, mate, what="malformed")
    assert exp["status"][:3] == [9, 7, 1] and exp["status"][7] == 1


def _two_unitigs():
    """U0: reads 0 1 2 forward (they face E), 3 reversed (B).  U1: 4 5 6 7 reversed (B).  U2: 8 forward (E), 9 reversed (B)."""
    return _layout([(1000, False, [(0, False, 100), (1, False, 300), (2, False, 500), (3, True, 50)]),
                    (800, False, [(4, True, 10), (5, True, 200), (6, True, 400), (7, True, 600)]),
                    (500, False, [(8, False, 250), (9, True, 100)])])


def test_links_two_records_the_swap_and_max_span():
    res, lengths = _two_unitigs(), [100] * 10
    # three pairs join U0's E end and U1's B end, one U0's B and U1's B
    mate = _mates(10, [(0, 4), (1, 5), (2, 6), (3, 7)])
    exp = _direct(res, lengths, mate, what="two records")
    assert [r[:3] for r in exp["links"]] == [(0, 2, 1), (1, 2, 3)]
    s = [900 + 110, 700 + 300, 500 + 500]
    assert exp["links"][1][3:] == (min(s), sum(s)) and exp["links"][0][3:] == (150 + 700, 150 + 700)
    swapped = _mates(10, [(3, 8), (2, 9)])
    exp = _direct(res, lengths, swapped, what="swap")
    assert [r[:2] for r in exp["links"]] == [(0, 5), (1, 4)]
    up = _layout([(500, False, [(5, False, 0)]), (500, False, [(1, True, 0)])])  # the smaller id lies in the later unitig: (2, 1) becomes (1, 2)
    exp = _direct(up, [100] * 6, _mates(6, [(1, 5)]), what="the a <= b swap")
    assert exp["links"] == [(1, 2, 1, 600, 600)]
    for outward in (False, True):  # outward: every read faces its other end
        for ms, linked in ((min(s), 2), (min(s) - 1, 0), (max(s), 3)):
            o = {"max_span": ms, "outward": outward}
            exp = _direct(res, lengths, mate, o, what="max_span %d outward=%s" % (ms, outward))
            if not outward:
                assert exp["status"][18] == 4 and exp["status"][20] + exp["status"][21] == 4
                assert ([r for r in exp["links"] if r[:2] == (1, 2)] or [(0, 0, 0)])[0][2] == linked
    exp = _direct(res, lengths, mate, {"outward": True}, what="outward links")
    assert [r[:3] for r in exp["links"]] == [(0, 3, 3), (1, 3, 1)]


def test_a_link_into_a_ring():
    res = _layout([(400, True, [(0, False, 0), (1, False, 150)]), (300, False, [(2, True, 0), (3, False, 100)])])
    exp = _direct(res, [100] * 4, _mates(4, [(0, 2), (1, 3)]), what="ring link")
    assert exp["status"][18] == exp["status"][19] == 2 and exp["links"] == [] and exp["status"][21] == 0


def test_histogram_edges():
    # inward pairs of spans 48 .. 63 (bin 3 of 4 at shift 4), 64 and 1000 (above it), and 16 (bin 1)
    spans = [48, 63, 64, 1000, 16]
    placed, pairs = [], []
    for k, sp in enumerate(spans):
        placed += [(2 * k, False, 2000 * k), (2 * k + 1, True, 2000 * k + sp - 10)]
        pairs.append((2 * k, 2 * k + 1))
    res = _layout([(20000, False, placed)])
    n = 2 * len(spans)
    exp = _direct(res, [10] * n, _mates(n, pairs), {"hist_bins": 4, "hist_shift": 4}, what="bins 4 shift 4")
    assert exp["hist"] == [0, 1, 0, 4]
    exp = _direct(res, [10] * n, _mates(n, pairs), {"hist_bins": 1, "hist_shift": 0}, what="one bin")
    assert exp["hist"] == [5]
    exp = _direct(res, [10] * n, _mates(n, pairs), {"hist_bins": 8192, "hist_shift": 31}, what="shift 31")
    assert exp["hist"][0] == 5
    exp = _direct(res, [10] * n, _mates(n, pairs), {"hist_bins": 8192, "hist_shift": 0}, what="8192 bins")
    assert exp["hist"][1000] == 1 and exp["hist"][8191] == 0


@pytest.mark.parametrize("k", [65, 300])
def test_one_key_and_one_bin_contended(k):
    """k pairs in one link key and k pairs of one span, ids shuffled: whole waves of one run, workgroups of one bin"""
    rng = random.Random(k)
    ids = list(range(4 * k))
    rng.shuffle(ids)
    a, b, c, d = ids[:k], ids[k:2 * k], ids[2 * k:3 * k], ids[3 * k:]
    u0 = [(r, False, 7 * i) for i, r in enumerate(a)] + [(r, False, 10000 + 3 * i) for i, r in enumerate(c)] + \
         [(r, True, 10000 + 3 * i + 400) for i, r in enumerate(d)]
    u1 = [(r, True, 5 * i) for i, r in enumerate(b)]
    res = _layout([(20000, False, u0), (9000, False, u1)])
    mate = _mates(4 * k, list(zip(a, b)) + list(zip(c, d)))
    exp = _direct(res, [100] * (4 * k), mate, what="contended %d" % k)
    assert len(exp["links"]) == 1 and exp["links"][0][:3] == (1, 2, k)
    assert exp["hist"][500] == k == exp["status"][14] and exp["status"][5] == k and exp["status"][7] == 0


def test_300_distinct_keys():
    n = 600
    res = _layout([(100 + r, False, [(r, r % 3 == 0, 0)]) for r in range(n)])
    rng = random.Random(3)
    ids = list(range(n))
    rng.shuffle(ids)
    exp = _direct(res, [100] * n, _mates(n, [(ids[2 * k], ids[2 * k + 1]) for k in range(300)]), what="300 keys")
    assert len(exp["links"]) == 300 and all(r[2] == 1 for r in exp["links"]) and exp["links"] == sorted(exp["links"])


def test_sums_carry_and_far():
    d = (1 << 32) - 200
    res = _layout([((1 << 33) + 5000, False, [(0, False, 0), (1, True, d), (2, False, 1000), (3, True, 1000 + d), (4, False, 5000),
                                               (5, True, 5000 + (1 << 32) - 100)])])
    exp = _direct(res, [100] * 6, _mates(6, [(0, 1), (2, 3), (4, 5)]), what="carry")
    assert exp["status"][4] == 3 and exp["status"][9] == 1 and exp["status"][10] == 2 and exp["status"][11] == 2 * d
    assert exp["status"][13] == 1 and exp["status"][12] + (1 << 64) == 2 * d * d
    assert exp["status"][17] == 1 and exp["status"][15] == 2 * (d + 100) and exp["hist"][1023] == 2
    assert exp["insert_size"] == d and exp["delta"] == 0


def test_hostile_tables():
    lengths = [50] * 8
    mate = _mates(8, [(0, 1), (2, 3), (4, 5), (6, 7)])
    # a placement whose read is beyond the reads: it is no read's placement
    res = _layout([(500, False, [(0, False, 0), (1, True, 100), (9, False, 150), (0xFFFFFFFF, True, 160)]), (300, False, [(2, False, 0), (4, True, 20)]),
                   (200, False, [(5, False, 5)])])
    exp = _direct(res, lengths, mate, what="read beyond the reads", host=True)
    assert exp["status"][2:5] == [4, 2, 1] and exp["status"][18] == 1
    # offsets that do not ascend: the bisection still ends inside the table
    bad = dict(res, lay_offs=[0, 6, 4, 7])
    exp = _direct(bad, lengths, mate, what="descending lay_offs", host=False)
    assert exp["status"][2] == 4
    # a count of unitigs beyond the reads is taken as the reads; the padded tables are what it then reads
    exp = _direct(res, lengths, mate, what="count beyond the reads", host=False, n_unitigs_dev=1 << 40)
    assert exp["status"][2] == 4
    few = _layout([(500, False, [(0, False, 0), (1, True, 100)])])
    _direct(few, [50, 50], _mates(2, [(0, 1)]), what="count beyond two reads", host=False, n_unitigs_dev=3)


def _host_chimeric(case):
    import siga_amd
    edges, lengths, seqs, offs = uc.arrays(case)
    return siga_amd.unitigs_chimeric(edges, lengths, seqs, offs, case["m"], case["x"], case["L"], case["C"], delta=case["delta"],
                                     careful=case["careful"], num_reads=case["N"], genome_size=case["G"], uniq_threshold=case["T"],
                                     min_chimeric_length=case["Lc"], min_chimeric_coverage=case["Ac"], chimeric_delta=case["delta_c"],
                                     chimeric_threshold=case["Tc"], graph=False)


def test_random_graphs_through_the_rounds():
    import siga_amd
    seen = [0] * 24
    for seed in range(100):
        case = pp.random_case(seed)
        lengths = [len(r) for r in case["reads"]]
        o = {"hist_bins": 32, "hist_shift": 3, "max_span": (0, 150)[seed % 2], "outward": seed % 3 == 0}
        res = _host_chimeric(case)
        exp = pp.expected_pairs(res, lengths, case["mate"], o)
        _same(siga_amd.unitigs_pairs(res, lengths, case["mate"], **o), exp, case["name"] + ", host")
        got, tails = _chained(case, o, chimeric=True)
        _same(got, exp, case["name"] + ", device")
        _untouched(tails, case["name"])
        seen = [a + b for a, b in zip(seen, exp["status"])]
    print("over the 100 graphs", seen)
    assert all(seen[k] > 0 for k in (1, 2, 3, 4, 5, 6, 7, 14, 18, 20, 21, 22)), seen


def test_refusals():
    from siga_amd import _lib
    L = _lib.lib()
    E = _lib.SIGAX_E_ARG
    wb = C.c_uint64()
    assert L.sigax_unitigs_pairs_workspace(0, 1 << 31, C.byref(wb)) == E
    assert L.sigax_unitigs_pairs_workspace(0, 100, None) == E
    assert L.sigax_unitigs_pairs_workspace(0, 0, C.byref(wb)) == 0
    n = 8
    assert L.sigax_unitigs_pairs_workspace(0, n, C.byref(wb)) == 0
    b = [torch.zeros(4096, dtype=torch.uint8, device="cuda:0") for _ in range(10)]
    p = [t.data_ptr() for t in b]
    work = torch.zeros(wb.value, dtype=torch.uint8, device="cuda:0")
    z = None

    def opts(flags=0, bins=16, shift=0, reserved=0, max_span=0):
        return C.byref(_lib.PairsOpts(flags, bins, shift, reserved, max_span))

    def dev(nr=n, o="usual", w=work.data_ptr(), nbytes=wb.value, **over):
        a = {"mate": p[0], "len": p[1], "nu": p[2], "so": p[3], "lo": p[4], "uf": p[5], "lay": p[6], "hist": p[7], "links": p[8], "st": p[9]}
        a.update(over)
        return L.sigax_unitigs_pairs_device(0, a["mate"], a["len"], nr, a["nu"], a["so"], a["lo"], a["uf"], a["lay"], opts() if o == "usual" else o, a["hist"],
                                            a["links"], a["st"], w, nbytes, z)

    assert dev(o=None) == E
    assert dev(o=opts(reserved=1)) == E and "reserved" in _lib.last_error()
    assert dev(o=opts(flags=2)) == E and "flags" in _lib.last_error()
    assert dev(o=opts(bins=0)) == E and "hist_bins" in _lib.last_error()
    assert dev(o=opts(bins=8193)) == E and "hist_bins" in _lib.last_error()
    assert dev(o=opts(shift=32)) == E and "hist_shift" in _lib.last_error()
    assert dev(nr=1 << 31) == E
    assert dev(nbytes=wb.value - 1) == E and "workspace" in _lib.last_error()
    for k in ("mate", "len", "nu", "so", "lo", "uf", "lay", "hist", "links", "st"):
        assert dev(**{k: z}) == E, k
    assert dev(w=z) == E
    for k, off in (("mate", 2), ("len", 2), ("uf", 2), ("nu", 4), ("so", 4), ("lo", 4), ("hist", 4), ("links", 4), ("st", 4), ("lay", 8)):
        assert dev(**{k: p[0] + 2048 + off}) == E and "aligned" in _lib.last_error(), k
    assert dev(w=work.data_ptr() + 8) == E and "aligned" in _lib.last_error()
    assert dev() == 0, _lib.last_error()  # (everything zero: no unitigs, every mate entry 0 -> read 0 is its own mate, the rest not reciprocal)
    torch.cuda.synchronize()
    st = b[9].cpu().numpy()[:192].view(np.uint64).tolist()
    assert st[:3] == [8, 8, 0] and st[3:] == [0] * 21
    hp, lp = C.c_void_p(), C.c_void_p()
    s24 = (C.c_uint64 * 24)()
    host = lambda nr, nu, o, ph, ps: L.sigax_unitigs_pairs_host(0, z, z, nr, nu, z, z, z, z, o, ph, C.byref(lp), ps)  # noqa: E731
    assert host(0, 0, opts(), C.byref(hp), s24) == 0 and list(s24) == [0] * 24
    L.sigax_free(hp)
    L.sigax_free(lp)
    assert host(0, 0, opts(), None, s24) == E
    assert host(0, 0, opts(), C.byref(hp), None) == E
    assert host(0, 0, None, C.byref(hp), s24) == E
    assert host(0, 0, opts(bins=0), C.byref(hp), s24) == E
    assert host(3, 0, opts(), C.byref(hp), s24) == E  # NULL buffers
    m3 = (C.c_uint32 * 3)(NO, NO, NO)
    o2 = (C.c_uint64 * 5)(0, 0, 0, 0, 9)
    uf = (C.c_uint32 * 4)()
    call = lambda nu: L.sigax_unitigs_pairs_host(0, m3, m3, 3, nu, o2, o2, uf, z, opts(), C.byref(hp), C.byref(lp), s24)  # noqa: E731
    assert call(4) == E and "unitigs" in _lib.last_error()
    assert call(3) == 0
    L.sigax_free(hp)
    L.sigax_free(lp)
    o2[3] = 9
    assert call(3) == E and "placements" in _lib.last_error()


# ---- the command line, once: paired reads of one length at a fixed insert over a small random genome ----
E2E_SEED, E2E_GENOME, E2E_LEN, E2E_INSERT, E2E_PAIRS, E2E_M = 11, 5000, 60, 240, 330, 25


@functools.lru_cache(maxsize=None)
def _e2e_reads():
    rng = random.Random(E2E_SEED)
    while True:
        g = bytes(rng.choice(b"ACGT") for _ in range(E2E_GENOME))
        if not uc.longest_repeat_at_least(g, E2E_M):
            break
    names, reads = [], []
    for k, p in enumerate(rng.sample(range(E2E_GENOME - E2E_INSERT + 1), E2E_PAIRS)):
        fwd, back = g[p:p + E2E_LEN], uc.revcomp(g[p + E2E_INSERT - E2E_LEN:p + E2E_INSERT])
        if rng.random() < 0.5:
            fwd, back = back, fwd
        names += ["pair%d/1" % k, "pair%d/2" % k]
        reads += [fwd, back]
    return names, reads


def _e2e_files():
    d = os.path.join(CACHE, "unitig_pairs_e2e")
    os.makedirs(d, exist_ok=True)
    prefix = os.path.join(d, "reads")
    names, reads = _e2e_reads()
    if not all(os.path.exists(prefix + e) for e in (".bwt", ".rbwt", ".sai", ".rsai", ".fa")):
        seqs = [s.decode() for s in reads]
        po.Index.build(seqs).save(prefix + ".bwt", prefix + ".sai")
        po.Index.build(seqs, reverse=True).save(prefix + ".rbwt", prefix + ".rsai")
        with open(prefix + ".fa", "w") as f:
            f.write(mr.fasta_text(list(zip(names, seqs))))
    return prefix


def test_cli(tmp_path):
    import siga_amd
    from siga_amd import host
    prefix = _e2e_files()
    names, reads = _e2e_reads()
    fa0, fa, lay, pj, lk = (str(tmp_path / f) for f in ("plain.fa", "u.fa", "u.layout", "u.pairs.json", "u.links"))
    base = [host.CLI_PATH, "unitig", "-m", str(E2E_M), "-p", prefix]
    r = subprocess.run(base + ["-o", fa0, prefix + ".fa"], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    r = subprocess.run(base + ["-o", fa, "--layout", lay, "--pairs", pj, "--links", lk, "--max-span", "2000", "--pairs-bins", "64", "--pairs-shift",
                               "3", prefix + ".fa"], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    assert open(fa, "rb").read() == open(fa0, "rb").read() and b"pairs" in r.stderr
    # the unitigs as the layout and the FASTA give them
    ids = {n: i for i, n in enumerate(names)}
    bases = [len(l.strip()) for l in open(fa).read().split("\n")[1::2] if l.strip()]
    res = {"seq_offs": [0], "lay_offs": [0], "uflags": [], "layout": []}
    for h in [l for l in open(fa).read().split("\n") if l.startswith(">")]:
        res["uflags"].append(uc.CIRCULAR if "circular=" in h else 0)
    for b in bases:
        res["seq_offs"].append(res["seq_offs"][-1] + b)
    per = [0] * len(bases)
    for line in open(lay).read().splitlines():
        u, name, strand, off = line.split("\t")
        per[int(u.split("-")[1])] += 1
        res["layout"].append((ids[name], uc.PLACED_REV if strand == "-" else 0, int(off)))
    for c in per:
        res["lay_offs"].append(res["lay_offs"][-1] + c)
    mate = siga_amd.mates_by_name(names)
    assert mate.tolist() == [i ^ 1 for i in range(len(names))]
    exp = pp.expected_pairs(res, [len(s) for s in reads], mate, {"hist_bins": 64, "hist_shift": 3, "max_span": 2000})
    assert exp["status"][4] > 0 and exp["status"][21] > 0, exp["status"]
    got = json.loads(open(pj).read())["pairs"]
    from siga_amd import _lib
    assert [got[k] for k in _lib.PAIRS_STATUS] == exp["status"]
    assert (got["insert_size"], got["delta"], got["span_mean"], got["span_sd"]) == (exp["insert_size"], exp["delta"], exp["span_mean"], exp["span_sd"])
    assert got["hist_bins"] == 64 and got["hist_shift"] == 3
    hist = [0] * 64
    for bin_, cnt in got["histogram"]:
        hist[bin_] = cnt
    assert hist == exp["hist"]
    # error-free reads at one insert: every inward pair inside a unitig spans the insert
    assert exp["insert_size"] == E2E_INSERT - E2E_LEN and exp["delta"] == 0 and exp["hist"][E2E_INSERT >> 3] == exp["status"][14] > 0
    want = "".join("LK\tunitig-%d\t%s\tunitig-%d\t%s\t%d\t%d\t%d\n" % (a >> 1, "BE"[a & 1], b >> 1, "BE"[b & 1], c, mn, sm)
                   for a, b, c, mn, sm in exp["links"])
    assert open(lk).read() == want
    r = subprocess.run(base + ["-o", fa, "--links", lk, prefix + ".fa"], capture_output=True)
    assert r.returncode == 1 and b"--pairs" in r.stderr
    r = subprocess.run(base, capture_output=True)  # no READSFILE: the help text
    assert r.returncode == 0 and all(w in r.stdout for w in (b"--pairs=FILE", b"--links=FILE", b"--max-span", b"--outward", b"--pairs-bins",
                                                              b"--pairs-shift"))
