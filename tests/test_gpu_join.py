"""Overlap joining of `siga unitig --scaffold --join-overlaps` on the GPU (csrc/sigax_join.hip) against the serial restatement of its
rules (tests/join_cases.py::expected_join): every case through the host form and through the device form over output buffers of
exactly their size with canaries behind them, on the forward-only and on the two-strand index; a subset in child processes
without the two-step tables and with 64-bit positions over small superblocks; once the unitig, pairs, scaffold, gapfill and join
calls enqueued on one stream with nothing in between; capacity; hostile tables; refusals; the command line."""
import ctypes as C
import functools
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch  # before the library loads: one HIP runtime per process

from tests import gapfill_cases as gc
from tests import join_cases as jc
from tests import pair_cases as pp
from tests import scaffold_cases as sc
from tests import unitig_cases as uc
from tests.fixtures import ROOT

pytestmark = pytest.mark.gpu
CANARY = 64


def _tg():
    from tests import test_gpu_gapfill as tg
    return tg


def _open(reads, both):
    return _tg()._open(reads, both)


def _up(a):
    a = np.frombuffer(a, dtype=np.uint8) if isinstance(a, bytes) else np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return torch.from_numpy(a.copy()).to("cuda:0") if a.size else torch.zeros(16, dtype=torch.uint8, device="cuda:0")


def _out(nbytes):
    return torch.full((nbytes + CANARY,), 0xEE, dtype=torch.uint8, device="cuda:0")


def _jopts(o):
    from siga_amd import _lib
    return _lib.JoinOpts(0, o["min_overlap"], o["max_overlap"], o["slack"], o["k"], o["min_count"], 0)


def _same(got, exp, what, seqs=True):
    st = [int(x) for x in got["status"]]
    print(what, "status", st, "expected", exp["status"])
    assert st == exp["status"], what
    assert [int(x) for x in got["sc_offs"]] == exp["sc_offs"], what
    assert [tuple(int(x) for x in p) for p in got["layout"].tolist()] == exp["layout"], what
    assert [tuple(int(x) for x in g) for g in got["joins"].tolist()] == exp["joins"], what
    if seqs and exp["seqs"] is not None:
        assert got["seqs"] is not None and bytes(got["seqs"]) == exp["seqs"], what


def _padded(values, n, dtype):
    a = np.zeros(n, dtype=dtype)
    v = np.array(values, dtype=dtype)[:n]
    a[:len(v)] = v
    return a


def _enqueue(L, ix, mu, nu_ptr, so_ptr, ns_ptr, sco_ptr, slo_ptr, lay_ptr, seqs_ptr, seqs_bytes, o, capacity, stream):
    """sigax_join_device over output buffers of exactly their size plus CANARY bytes of 0xEE -> (buffers, sizes)"""
    from siga_amd import _lib
    wb = C.c_uint64()
    assert L.sigax_join_workspace(mu, C.byref(wb)) == 0
    sizes = {"sc_offs": 8 * (mu + 1), "layout": 16 * mu, "joins": 32 * mu, "status": 128, "work": wb.value}
    if capacity is not None:
        sizes["seqs"] = capacity
    d = {k: _out(v) for k, v in sizes.items()}
    torch.cuda.synchronize()
    opts = _jopts(o)
    rc = L.sigax_join_device(ix.handle, nu_ptr, mu, so_ptr, ns_ptr, sco_ptr, slo_ptr, lay_ptr, seqs_ptr, seqs_bytes, C.byref(opts), d["sc_offs"].data_ptr(),
                             d["layout"].data_ptr(), d["seqs"].data_ptr() if capacity is not None else None, capacity or 0, d["joins"].data_ptr(),
                             d["status"].data_ptr(), d["work"].data_ptr(), wb.value, stream)
    assert rc == 0, _lib.last_error()
    return d, sizes


def _collect(d, sizes, what):
    """the results, and that nothing behind them was written: the canaries, the table entries beyond the scaffolds, the placements
    and the gaps, and all of the bases buffer when the status says they were not written"""
    from siga_amd import _lib
    h = {k: v.cpu().numpy() for k, v in d.items()}
    status = h["status"][:128].view(np.uint64)
    ng, total, s = int(status[0]), int(status[11]), int(status[15])
    got = {"status": status, "sc_offs": h["sc_offs"][:8 * (s + 1)].view(np.uint64), "joins": h["joins"][:32 * ng].view(_lib.JOIN_DTYPE), "seqs": None}
    lay = h["layout"][:sizes["layout"]].view(_lib.PLACEMENT_DTYPE)
    placed = len(lay)
    while placed and h["layout"][16 * (placed - 1):16 * placed].tobytes() == b"\xee" * 16:
        placed -= 1
    got["layout"] = lay[:placed]
    used = {"sc_offs": 8 * (s + 1), "layout": 16 * placed, "joins": 32 * ng, "status": 128}
    if "seqs" in sizes:
        written = int(status[14]) == 0
        assert written == (total <= sizes["seqs"])
        used["seqs"] = total if written else 0
        got["seqs"] = h["seqs"][:total].tobytes() if written else None
    for k in used:
        rest = h[k][used[k]:].tobytes()
        assert len(rest) >= CANARY and rest == b"\xee" * len(rest), "%s: bytes after %s were written" % (what, k)
    assert h["work"][sizes["work"]:].tobytes() == b"\xee" * CANARY, what
    return got


def _device(ix, c, what, capacity="exact", nu_dev=None, ns_dev=None, seqs_bytes=None, compare=True, bases=True):
    """the device form over the case's tables in buffers of exactly their size -> (expected_join's dict, what came back)"""
    from siga_amd import _lib
    L = _lib.lib()
    res, scaf = c["res"], c["scaf"]
    mu = len(res["seq_offs"]) - 1
    s = len(scaf["sc_lay_offs"]) - 1
    kw = dict(n_unitigs=nu_dev, n_scaffolds=ns_dev, sseqs_bytes=seqs_bytes, bases=bases)
    exp, cap = None, capacity
    if compare:
        exp = jc.expected_join(c["reads"], res, scaf, c["opts"], **kw)
        cap = exp["status"][11] if capacity == "exact" else capacity
        exp = jc.expected_join(c["reads"], res, scaf, c["opts"], sseqs_capacity=cap or 0, **kw)
    counts = _up(np.array([mu if nu_dev is None else nu_dev, s if ns_dev is None else ns_dev], dtype=np.uint64))
    d_so = _up(np.array(res["seq_offs"], dtype=np.uint64))
    d_sco = _up(_padded(scaf["sc_offs"], mu + 1, np.uint64))
    d_slo = _up(_padded(scaf["sc_lay_offs"], mu + 1, np.uint64))
    lay = np.zeros(mu, dtype=_lib.PLACEMENT_DTYPE)
    for i, p in enumerate(scaf["layout"][:mu]):
        lay[i] = tuple(p)
    d_lay, d_seqs = _up(lay), _up(scaf["seqs"])
    d, sizes = _enqueue(L, ix, mu, counts.data_ptr(), d_so.data_ptr(), counts.data_ptr() + 8, d_sco.data_ptr(), d_slo.data_ptr(), d_lay.data_ptr(),
                        d_seqs.data_ptr(), len(scaf["seqs"]) if seqs_bytes is None else seqs_bytes, c["opts"], cap, None)
    torch.cuda.synchronize()
    got = _collect(d, sizes, what)
    if compare:
        _same(got, exp, what + ", device", seqs=bases and exp["status"][14] == 0)
        if exp["status"][14]:
            assert got["seqs"] is None
    return exp, got


def _host_call(ix, c):
    import siga_amd
    o = c["opts"]
    scaf = dict(c["scaf"], layout=np.array([tuple(p) for p in c["scaf"]["layout"]], dtype=siga_amd._lib.PLACEMENT_DTYPE))
    return siga_amd.scaffolds_join(ix, c["res"], scaf, min_overlap=o["min_overlap"], max_overlap=o["max_overlap"], slack=o["slack"], k=o["k"],
                                   min_count=o["min_count"])


def _host(ix, c, what):
    exp = jc.case_expected(c)
    got = _host_call(ix, c)
    _same(got, exp, what + ", host")
    assert got["sc_lay_offs"].tolist() == c["scaf"]["sc_lay_offs"] and got["sc_flags"].tolist() == c["scaf"]["sc_flags"]
    return exp, got


def _run_cases(cases, again=False):
    """every case through both forms on both kinds of index, one pair of indexes per read set; again: what the host form gave
    through the device form once more, which must give it back"""
    by_reads = {}
    for c in cases:
        by_reads.setdefault(c["reads_key"], []).append(c)
    for key, group in by_reads.items():
        for both in (False, True):
            ix = _open(group[0]["reads"], both)
            try:
                for c in group:
                    what = "%s, %s index" % (c["name"], "two-strand" if both else "forward-only")
                    exp, got = _host(ix, c, what)
                    _device(ix, c, what)
                    if again and both:
                        c2 = jc.joined_again(c, exp)
                        exp2, got2 = _device(ix, c2, what + ", again")
                        assert exp2["status"][1] == 0 and got2["seqs"] == exp["seqs"] and exp2["layout"] == exp["layout"] and exp2["sc_offs"] == exp["sc_offs"]
            finally:
                ix.close()


@pytest.mark.parametrize("k", jc.KS)
def test_hand_built(k):
    _run_cases(jc.hand_built(k), again=True)


@pytest.mark.parametrize("count", [70, 300])
def test_many_gaps_across_waves_and_workgroups(count):
    c = jc.many_gaps(count)
    _run_cases([c], again=True)
    assert jc.case_expected(c)["status"][0] == count + 1


@pytest.mark.parametrize("block", range(5))
def test_random_cases(block):
    _run_cases([jc.random_case(s) for s in range(20 * block, 20 * block + 20)], again=True)


LIMITS = ("hi_4096_by_both_lengths", "hi_66_words")


@pytest.mark.parametrize("part", ["limits", "rest"])
def test_long_overlaps(part):
    """k_join_match with up to 4096 candidates a gap: all 129 LDS words, lanes that pack two and three words, hi clipped by
    max_overlap, |M| beyond 255 (tests/join_cases.py::long_overlaps)"""
    _run_cases([c for c in jc.long_overlaps(31) if (c["kind"] in LIMITS) == (part == "limits")], again=True)


def test_more_open_gaps_than_the_match_grid():
    """16 * n_cu + 300 gaps: the one-wave workgroups of k_join_match and k_join_support take a second gap, the one over the hole
    in the reads among them"""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    c, exp, hole = jc.beyond_the_grid(n_cu)
    opened = jc.came_to_the_match(exp)
    print("n_cu", n_cu, "gaps", exp["status"][0], "came to the match", len(opened), "windows", exp["status"][13], "hole under gap", hole)
    assert exp["status"][0] == 16 * n_cu + 301 and len(opened) > 16 * n_cu and exp["status"][13] > 0
    assert exp["joins"][hole][5] == jc.C["UNSUPPORTED"] and opened.index(hole) >= 16 * n_cu
    total = exp["status"][11]
    for both in (False, True):
        ix = _open(c["reads"], both)
        try:
            what = "%s, %s index" % (c["name"], "two-strand" if both else "forward-only")
            got = _device(ix, c, what, capacity=total, compare=False)[1]
            _same(got, exp, what + ", device")
            if both:
                _same(_host_call(ix, c), exp, what + ", host")
        finally:
            ix.close()


# ---- other forms of the index, in child processes ----
def _child(env_extra, ids):
    env = dict(os.environ, **env_extra)
    what = [os.path.join(ROOT, "tests", "test_gpu_join.py") + "::" + i for i in ids]
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q"] + what, cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


SUBSET = ["test_hand_built[15]", "test_hand_built[64]", "test_random_cases[0]", "test_long_overlaps[limits]"]


def test_without_two_step_tables():
    _child({"SIGAX_TWO_STEP": "0"}, SUBSET)


def test_wide_positions_small_superblocks():
    lib = os.path.join(ROOT, "build", "libsigax_super12.so")
    assert os.path.exists(lib)
    _child({"SIGAX_FORCE_WIDE": "1", "SIGAX_LIB": lib}, SUBSET)


def test_wide_positions_without_two_step_tables():
    lib = os.path.join(ROOT, "build", "libsigax_super12.so")
    assert os.path.exists(lib)
    _child({"SIGAX_FORCE_WIDE": "1", "SIGAX_LIB": lib, "SIGAX_TWO_STEP": "0"}, SUBSET[1:2])


# ---- capacity ----
def test_capacity():
    c = next(x for x in jc.hand_built(31) if x["kind"] == "three_joins_in_a_row")
    ix = _open(c["reads"], False)
    try:
        total = jc.case_expected(c)["status"][11]
        assert total < len(c["scaf"]["seqs"])
        assert _device(ix, c, "one byte short", capacity=total - 1)[0]["status"][14] == 1  # (_collect: nothing was written)
        assert _device(ix, c, "exact", capacity=total)[0]["status"][14] == 0
        assert _device(ix, c, "room to spare", capacity=total + 100)[0]["status"][14] == 0
        assert _device(ix, c, "no bases asked for", capacity=None)[0]["status"][14] == 1
    finally:
        ix.close()


# ---- hostile tables ----
def test_hostile_tables():
    c = dict(next(x for x in jc.hand_built(15) if x["kind"] == "three_joins_in_a_row"))
    ix = _open(c["reads"], False)
    try:
        mu = len(c["res"]["seq_offs"]) - 1
        # counts on the device above their capacities are taken as the capacities; below them, the rest of the tables is unread
        assert _device(ix, c, "unitigs beyond the capacity", nu_dev=1 << 40)[0]["status"][0] == 3
        exp, _ = _device(ix, c, "scaffolds beyond the capacity", ns_dev=1 << 33, bases=False)  # (the table's last entry, a zero here, is the placements)
        assert exp["status"][15] == mu and exp["status"][0] == 0
        exp, _ = _device(ix, c, "fewer unitigs than the layout names", nu_dev=2)
        assert exp["status"][1 + jc.C["MALFORMED"]] >= 1
        assert _device(ix, c, "no scaffolds", ns_dev=0)[0]["status"][:1] == [0]
        # scaffold offsets that claim more bases than there are: every placement of the scaffold is bad
        exp, _ = _device(ix, c, "bases cut short", seqs_bytes=len(c["scaf"]["seqs"]) - 5, capacity=0)
        assert exp["status"][1 + jc.C["MALFORMED"]] == 3
        # offsets and tables that do not ascend: the call ends, the status is the rules', nothing behind a buffer is written
        lay, so = c["scaf"]["layout"], c["res"]["seq_offs"]
        for name, scaf, res in (
                ("descending offsets", dict(c["scaf"], layout=[(p[0], p[1], (1 << 40) - 7 * i * p[2]) for i, p in enumerate(lay)]), c["res"]),
                ("offsets that wrap", dict(c["scaf"], layout=[(p[0], p[1], (p[2] - 30) & jc.M64) for p in lay]), c["res"]),
                ("a placement beyond its scaffold", dict(c["scaf"], layout=lay[:3] + [(lay[3][0], 0, lay[3][2] + 1)]), c["res"]),
                ("lay_offs that do not ascend", dict(c["scaf"], sc_lay_offs=[0, 3, 1, 4], sc_flags=[0, 0, 0], sc_offs=[0, 100, 150, len(c["scaf"]["seqs"])]),
                 c["res"]),
                ("lay_offs beyond the placements", dict(c["scaf"], sc_lay_offs=[2, 1 << 50]), c["res"]),
                ("descending sc_offs", dict(c["scaf"], sc_lay_offs=[0, 2, 4], sc_flags=[0, 0], sc_offs=[0, 400, 250]), c["res"]),
                ("sc_offs beyond the bases", dict(c["scaf"], sc_offs=[0, 1 << 45]), c["res"]),
                ("descending seq_offs", c["scaf"], dict(c["res"], seq_offs=[0, 90, 40, 200, so[-1]]))):
            exp = jc.expected_join(c["reads"], res, scaf, c["opts"], sseqs_capacity=0)
            for cap in (0, 64, 1 << 16):
                got = _device(ix, dict(c, scaf=scaf, res=res), name, capacity=cap, compare=False)[1]
                st = [int(x) for x in got["status"]]
                print(name, cap, st, exp["status"])
                assert st[:14] + st[15:] == exp["status"][:14] + exp["status"][15:] and st[14] == (1 if st[11] > cap else 0), (name, cap)
                assert [tuple(int(x) for x in g) for g in got["joins"].tolist()] == exp["joins"], (name, cap)
                assert [int(x) for x in got["sc_offs"]] == exp["sc_offs"], (name, cap)
    finally:
        ix.close()


def test_no_unitigs():
    import siga_amd
    from siga_amd import _lib
    c = next(x for x in jc.hand_built(15) if x["kind"] == "v_16")
    ix = _open(c["reads"], False)
    try:
        got = siga_amd.scaffolds_join(ix, {"seq_offs": [0]}, {"sc_offs": [0], "sc_lay_offs": [0], "sc_flags": [], "layout": [], "seqs": b""}, k=15)
        assert got["status"].tolist() == [0] * 16 and got["sc_offs"].tolist() == [0] and len(got["joins"]) == 0 and len(got["seqs"]) == 0
        st = _out(128)
        opts = _jopts(c["opts"])
        assert _lib.lib().sigax_join_device(ix.handle, None, 0, None, None, None, None, None, None, 0, C.byref(opts), None, None, None, 0, None,
                                            st.data_ptr(), None, 0, None) == 0
        torch.cuda.synchronize()
        assert st.cpu().numpy().tobytes() == b"\0" * 128 + b"\xee" * CANARY
    finally:
        ix.close()


# ---- the five calls on one stream ----
def test_five_calls_on_one_stream():
    """sigax_unitigs_chimeric_device, sigax_unitigs_pairs_device, sigax_scaffold_device, sigax_gapfill_device and sigax_join_device
    enqueued on one stream, nothing in between: the join call reads both counts and the gapfill call's tables and bases where the
    calls before it leave them"""
    from siga_amd import _lib
    from tests import test_gpu_scaffold as ts
    from tests import test_gpu_unitig_pairs as tp
    tg = _tg()
    L = _lib.lib()
    seen = 0
    for seed in (3, 7, 18):
        case, res, pairs, o = ts._through_the_calls(seed)
        exp_sc = sc.expected_scaffolds(res, pairs["links"], pairs["status"], o)
        scaf = {"sc_lay_offs": exp_sc["sc_lay_offs"], "sc_flags": exp_sc["sc_flags"], "layout": exp_sc["layout"]}
        reads = tuple(bytes(r) if not isinstance(r, str) else r.encode() for r in case["reads"])
        go = dict(gc.DEFAULT_OPTS, k=15, min_count=1, slack=20)
        jo = dict(jc.DEFAULT_OPTS, k=15, min_count=1, min_overlap=8)
        n = len(reads)
        # the tables as the calls leave them: n-entry buffers, so the restatements see the same capacity
        res_n = {"seq_offs": tg._padded(res["seq_offs"], n + 1, np.uint64).tolist(), "useqs": bytes(res["useqs"])}
        nu = len(res["uflags"])
        exp_gf = gc.expected_gapfill(reads, res_n, scaf, go, n_unitigs=nu, n_scaffolds=exp_sc["status"][0], max_walk_bases=1 << 16,
                                     useqs_bytes=len(bytes(res["useqs"])))
        scaf_gf = {"sc_offs": exp_gf["sc_offs"], "sc_lay_offs": exp_gf["sc_lay_offs"], "sc_flags": exp_gf["sc_flags"], "layout": exp_gf["layout"],
                   "seqs": exp_gf["seqs"]}
        exp = jc.expected_join(reads, res_n, scaf_gf, jo, n_unitigs=nu, n_scaffolds=exp_sc["status"][0])
        ix = _open(reads, True)
        edges, lengths, seqs, offs = uc.arrays(case)
        ne, nb = len(edges), len(seqs)
        d_edges, d_len, d_seqs, d_offs = ts._up(edges), ts._up(lengths), ts._up(seqs), ts._up(offs)
        d_mate = ts._up(np.array(case["mate"], dtype=np.uint32))
        wb = C.c_uint64()
        assert L.sigax_unitigs_chimeric_workspace(n, ne, 0, int(case["careful"]), C.byref(wb)) == 0
        u = {k: ts._out(v) for k, v in {"seq_offs": 8 * (n + 1), "lay_offs": 8 * (n + 1), "uflags": 4 * n, "layout": 16 * n, "useqs": nb, "removed": 4 * n,
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
            s, _ = ts._enqueue(L, n, n // 2, u["status"].data_ptr(), u["seq_offs"].data_ptr(), u["uflags"].data_ptr(), u["useqs"].data_ptr(), nb,
                               p["links"].data_ptr() if n // 2 else None, p["status"].data_ptr() + 22 * 8, p["status"].data_ptr(), o,
                               exp_sc["status"][1], st)
            g, _ = tg._enqueue(L, ix, n, u["status"].data_ptr(), u["seq_offs"].data_ptr(), u["useqs"].data_ptr(), nb, s["status"].data_ptr(),
                               s["sc_lay_offs"].data_ptr(), s["layout"].data_ptr(), go, exp_gf["status"][16], 1 << 16, st)
            d, sizes = _enqueue(L, ix, n, u["status"].data_ptr(), u["seq_offs"].data_ptr(), g["status"].data_ptr() + 22 * 8, g["sc_offs"].data_ptr(),
                                s["sc_lay_offs"].data_ptr(), g["layout"].data_ptr(), g["seqs"].data_ptr(), exp_gf["status"][16], jo, exp["status"][11], st)
            torch.cuda.synchronize()
        finally:
            L.sigax_stream_destroy(0, st)
            ix.close()
        got = _collect(d, sizes, case["name"])
        _same(got, exp, case["name"] + ", chained")
        seen += exp["status"][0]
    assert seen > 0


# ---- refusals ----
def test_refusals():
    from siga_amd import _lib
    L = _lib.lib()
    E = _lib.SIGAX_E_ARG
    c = next(x for x in jc.hand_built(15) if x["kind"] == "v_16")
    ix = _open(c["reads"], False)
    try:
        wb = C.c_uint64()
        assert L.sigax_join_workspace(1 << 31, C.byref(wb)) == E and "max_unitigs" in _lib.last_error()
        assert L.sigax_join_workspace(10, None) == E
        assert L.sigax_join_workspace(0, C.byref(wb)) == 0 and wb.value == 0
        mu = 8
        assert L.sigax_join_workspace(mu, C.byref(wb)) == 0
        names = ("nu", "so", "ns", "sco", "slo", "lay", "sq", "scoo", "layo", "sqo", "joins", "st")
        b = [torch.zeros(4096, dtype=torch.uint8, device="cuda:0") for _ in names]
        p = [t.data_ptr() for t in b]
        work = torch.zeros(wb.value, dtype=torch.uint8, device="cuda:0")
        z = None
        full = {"nu": "d_n_unitigs", "so": "d_seq_offs", "ns": "d_n_scaffolds", "sco": "d_sc_offs", "slo": "d_sc_lay_offs", "lay": "d_sc_layout",
                "sq": "d_sseqs", "scoo": "d_sc_offs_out", "layo": "d_sc_layout_out", "sqo": "d_sseqs_out", "joins": "d_joins", "st": "d_status16"}

        def opts(flags=0, lo=16, hi=100, slack=10, k=15, mc=3, reserved=0):
            return C.byref(_lib.JoinOpts(flags, lo, hi, slack, k, mc, reserved))

        def dev(o="usual", handle=ix.handle, w=work.data_ptr(), nbytes=wb.value, nmu=mu, sbytes=1024, cap=64, **over):
            a = dict(zip(names, p))
            a.update(over)
            return L.sigax_join_device(handle, a["nu"], nmu, a["so"], a["ns"], a["sco"], a["slo"], a["lay"], a["sq"], sbytes, opts() if o == "usual" else o,
                                       a["scoo"], a["layo"], a["sqo"], cap, a["joins"], a["st"], w, nbytes, z)

        assert dev(o=None) == E and dev(handle=None) == E
        assert dev(o=opts(flags=1)) == E and "flags" in _lib.last_error()
        assert dev(o=opts(reserved=1)) == E
        for lo in (0, 7, 4097):
            assert dev(o=opts(lo=lo, hi=4096)) == E and "min_overlap" in _lib.last_error()
        for hi in (15, 4097):
            assert dev(o=opts(hi=hi)) == E and "max_overlap" in _lib.last_error()
        for k in (0, 7, 129):
            assert dev(o=opts(k=k)) == E and "k " in _lib.last_error()
        assert dev(o=opts(mc=0)) == E and "min_count" in _lib.last_error()
        assert dev(o=opts(slack=1 << 31)) == E and "slack" in _lib.last_error()
        assert dev(nmu=1 << 31) == E and "max_unitigs" in _lib.last_error()
        assert dev(cap=1 << 43) == E and "sseqs_capacity" in _lib.last_error()
        assert dev(sbytes=1 << 43) == E and "sseqs_bytes" in _lib.last_error()
        assert dev(nbytes=wb.value - 1) == E and "workspace" in _lib.last_error()
        for k in names:
            if k not in ("sq", "sqo"):
                assert dev(**{k: z}) == E and full[k] in _lib.last_error(), k
        assert dev(sqo=z) == E and "d_sseqs_out" in _lib.last_error()  # NULL with a capacity
        assert dev(sq=z) == E and "d_sseqs:" in _lib.last_error()  # NULL with bytes
        assert dev(sqo=z, cap=0) == 0
        assert dev(w=z) == E and "d_work" in _lib.last_error()
        at = names.index
        assert dev(layo=p[at("lay")]) == E and "d_sc_layout_out overlaps" in _lib.last_error()
        assert dev(layo=p[at("lay")] + 16 * (mu - 1)) == E and "overlaps" in _lib.last_error()
        assert dev(scoo=p[at("sco")] + 8 * mu) == E and "d_sc_offs_out overlaps" in _lib.last_error()
        assert dev(sqo=p[at("sq")] + 1008) == E and "d_sseqs_out overlaps" in _lib.last_error()
        assert dev(sqo=p[at("sq")] + 1024) == 0
        for k, off in (("nu", 4), ("so", 4), ("ns", 4), ("sco", 4), ("slo", 4), ("scoo", 4), ("st", 4), ("lay", 8), ("layo", 8), ("joins", 8), ("sq", 8),
                       ("sqo", 8)):
            assert dev(**{k: p[0] + 2048 + off}) == E and "aligned" in _lib.last_error() and full[k] in _lib.last_error(), k
        assert dev(w=work.data_ptr() + 8) == E and "aligned" in _lib.last_error()
        assert dev(o=opts(lo=8, hi=8, k=8)) == 0 and dev(o=opts(lo=4096, hi=4096, k=128)) == 0, _lib.last_error()  # (everything zero: no scaffolds)
        torch.cuda.synchronize()
        assert b[at("st")].cpu().numpy()[:128].view(np.uint64).tolist() == [0] * 16
        # the host form
        ptrs = [C.c_void_p() for _ in range(4)]
        ng = C.c_uint64()
        s16 = (C.c_uint64 * 16)()
        g = c["genome"]
        so, sco, slo = (C.c_uint64 * 3)(0, 40, 80), (C.c_uint64 * 2)(0, 83), (C.c_uint64 * 2)(0, 2)
        lay = np.array([(0, 0, 0), (1, 0, 43)], dtype=_lib.PLACEMENT_DTYPE)
        sq = C.create_string_buffer(g[100:140] + b"NNN" + g[120:160])

        def host(o, handle=ix.handle, nu=2, so_=so, ns=1, sco_=sco, slo_=slo, lay_=lay.ctypes.data, sq_=sq, out=None, ng_=C.byref(ng), s16_=s16):
            out = [C.byref(x) for x in ptrs] if out is None else out
            return L.sigax_join_host(handle, nu, so_, ns, sco_, slo_, lay_, sq_, o, out[0], out[1], out[2], out[3], ng_, s16_)

        def free():
            for x in ptrs:
                L.sigax_free(x)

        assert host(opts()) == 0 and ng.value == 1 and list(s16)[:2] == [1, 1] and s16[11] == 60 and s16[14] == 0, (_lib.last_error(), list(s16))
        assert C.string_at(ptrs[2], 60) == g[100:160]
        free()
        assert host(None) == E and host(opts(k=7)) == E and host(opts(), handle=None) == E
        assert host(opts(), ng_=None) == E and host(opts(), s16_=None) == E
        assert host(opts(), out=[None] + [C.byref(x) for x in ptrs[1:]]) == E
        assert host(opts(), so_=z) == E and host(opts(), slo_=z) == E and host(opts(), sco_=z) == E
        assert host(opts(), sq_=z) == E and "sseqs" in _lib.last_error()
        assert host(opts(), lay_=z) == E and "sc_layout" in _lib.last_error()
        assert host(opts(), ns=3) == E and "n_scaffolds" in _lib.last_error()
        assert host(opts(), slo_=(C.c_uint64 * 2)(0, 3)) == E and "sc_lay_offs" in _lib.last_error()
        assert host(opts(), nu=1 << 31) == E
        assert host(opts(), out=[C.byref(ptrs[0]), C.byref(ptrs[1]), None, C.byref(ptrs[3])]) == 0  # the tables alone
        free()
        assert host(opts(), nu=0, so_=z, ns=0, sco_=z, slo_=z, lay_=z, sq_=z) == 0 and ng.value == 0 and list(s16) == [0] * 16
        free()
    finally:
        ix.close()


# ---- the command line, once: a genome with one repeat of two copies that is longer than the minimum overlap, so that it breaks
# the unitigs: the unitig before a copy ends where the copy ends, the one behind it begins where the copy begins.  The pairs link
# the two, the estimate between them is negative, the gap laid is --min-gap, and the join finds the repeat ----
E2E_COPIES, E2E_SEED = (1500, 4000), 41


@functools.lru_cache(maxsize=None)
def _e2e(seed):
    """-> (genome, names, reads): a read pair every E2E_STEP bases of the gapfill test's shape, the mates in random order"""
    tg = _tg()
    rng = random.Random(seed)
    while True:
        g = bytearray(rng.choice(b"ACGT") for _ in range(tg.E2E_GENOME))
        src, dst = E2E_COPIES
        g[dst:dst + tg.E2E_REPEAT] = g[src:src + tg.E2E_REPEAT]
        g = bytes(g)
        if not uc.longest_repeat_at_least(g[:dst] + g[dst + tg.E2E_REPEAT:], tg.E2E_M):
            break
    names, reads = [], []
    for k, p in enumerate(range(0, tg.E2E_GENOME - tg.E2E_INSERT + 1, tg.E2E_STEP)):
        fwd, back = g[p:p + tg.E2E_LEN], uc.revcomp(g[p + tg.E2E_INSERT - tg.E2E_LEN:p + tg.E2E_INSERT])
        if rng.random() < 0.5:
            fwd, back = back, fwd
        names += ["pair%d/1" % k, "pair%d/2" % k]
        reads += [fwd, back]
    return g, names, reads


def _e2e_files(seed):
    from oracle import pyoracle as po
    from tests.fixtures import CACHE
    from tests.golden import make_reads as mr
    d = os.path.join(CACHE, "unitig_join_e2e_%d" % seed)
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


def _unitig_tables(fa, lay, names):
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
    return res


def test_cli(tmp_path):
    import siga_amd
    from siga_amd import host
    tg = _tg()
    prefix = _e2e_files(E2E_SEED)
    genome, names, reads = _e2e(E2E_SEED)
    f = {k: str(tmp_path / k) for k in ("u.fa", "u.layout", "u.pairs.json", "s.fa", "s.layout", "g.fa", "g.layout", "g.gaps", "j.fa", "j.layout", "j.joins",
                                         "gj.fa", "gj.layout", "gj.gaps", "gj.joins")}
    base = [host.CLI_PATH, "unitig", "-m", str(tg.E2E_M), "-p", prefix, "-o", f["u.fa"], "--layout", f["u.layout"], "--pairs", f["u.pairs.json"],
            "--insert-size", str(tg.E2E_INSERT), "--min-scaffold-unitig", "100"]
    r = subprocess.run(base + ["--scaffold", f["s.fa"], "--scaffold-layout", f["s.layout"], prefix + ".fa"], capture_output=True)
    assert r.returncode == 0 and b"joined" not in r.stderr, r.stderr.decode()
    res = _unitig_tables(f["u.fa"], f["u.layout"], names)
    pairs = pp.expected_pairs(res, [len(s) for s in reads], siga_amd.mates_by_name(names), {})
    exp_sc = sc.expected_scaffolds(res, pairs["links"], pairs["status"], {"insert_size": tg.E2E_INSERT, "min_unitig_bases": 100})
    # without --join-overlaps every byte is the scaffold call's, and with --gapfill alone the gapfill call's
    efa, elay = sc.render(exp_sc)
    assert open(f["s.fa"]).read() == efa and open(f["s.layout"]).read() == elay
    scaf = {"sc_offs": exp_sc["sc_offs"], "sc_lay_offs": exp_sc["sc_lay_offs"], "sc_flags": exp_sc["sc_flags"], "layout": exp_sc["layout"],
            "seqs": exp_sc["seqs"]}
    exp_gf = gc.expected_gapfill(tuple(reads), res, scaf)
    r = subprocess.run(base + ["--scaffold", f["g.fa"], "--scaffold-layout", f["g.layout"], "--gapfill", "--gaps", f["g.gaps"], prefix + ".fa"],
                       capture_output=True)
    assert r.returncode == 0 and b"joined" not in r.stderr, r.stderr.decode()
    gfa, glay, ggaps = gc.render(exp_gf, res["seq_offs"])
    assert open(f["g.fa"]).read() == gfa and open(f["g.layout"]).read() == glay and open(f["g.gaps"]).read() == ggaps
    # the join behind the scaffold call
    r = subprocess.run(base + ["--scaffold", f["j.fa"], "--scaffold-layout", f["j.layout"], "--join-overlaps", "--joins", f["j.joins"], prefix + ".fa"],
                       capture_output=True)
    assert r.returncode == 0 and b" joined over " in r.stderr, r.stderr.decode()
    exp = jc.expected_join(tuple(reads), res, scaf)
    print("unitigs", np.diff(res["seq_offs"]).tolist(), "scaffold status", exp_sc["status"], "join status", exp["status"], exp["joins"])
    jfa, jlay, jjn = jc.render(exp, res["seq_offs"])
    assert open(f["j.fa"]).read() == jfa and open(f["j.layout"]).read() == jlay and open(f["j.joins"]).read() == jjn
    assert exp["status"][1] >= 1 and any(l.split("\t")[4].startswith("-") for l in jlay.splitlines())  # a joined pair: its gap before is negative
    both = genome + b"\n" + uc.revcomp(genome)
    for s in range(exp["status"][15]):
        if all(j[5] == jc.C["JOINED"] for j in exp["joins"] if j[0] == s):
            assert exp["seqs"][exp["sc_offs"][s]:exp["sc_offs"][s + 1]] in both, s
    # ... and behind the gapfill call: the GP lines keep the gapfill call's offsets
    r = subprocess.run(base + ["--scaffold", f["gj.fa"], "--scaffold-layout", f["gj.layout"], "--gapfill", "--gaps", f["gj.gaps"], "--join-overlaps",
                               "--join-min-overlap", "20", "--join-max-overlap", "500", "--join-slack", "50", "--join-kmer", "25", "--join-min-count", "2",
                               "--joins", f["gj.joins"], prefix + ".fa"], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    scaf_gf = {"sc_offs": exp_gf["sc_offs"], "sc_lay_offs": exp_gf["sc_lay_offs"], "sc_flags": exp_gf["sc_flags"], "layout": exp_gf["layout"],
               "seqs": exp_gf["seqs"]}
    exp2 = jc.expected_join(tuple(reads), res, scaf_gf, {"min_overlap": 20, "max_overlap": 500, "slack": 50, "k": 25, "min_count": 2})
    filled = [0] * exp_gf["status"][22]
    for g in exp_gf["gaps"]:
        filled[g[0]] += g[5] == gc.C["FILLED"]
    jfa, jlay, jjn = jc.render(exp2, res["seq_offs"], filled)
    assert open(f["gj.fa"]).read() == jfa and open(f["gj.layout"]).read() == jlay and open(f["gj.joins"]).read() == jjn
    assert open(f["gj.gaps"]).read() == ggaps
    # refusals and the help text
    r = subprocess.run(base + ["--join-overlaps", prefix + ".fa"], capture_output=True)
    assert r.returncode == 1 and b"--scaffold" in r.stderr
    for opt in (["--join-min-overlap", "20"], ["--join-max-overlap", "50"], ["--join-slack", "5"], ["--join-kmer", "21"], ["--join-min-count", "2"],
                ["--joins", f["j.joins"]]):
        r = subprocess.run(base + ["--scaffold", f["j.fa"]] + opt + [prefix + ".fa"], capture_output=True)
        assert r.returncode == 1 and b"--join-overlaps" in r.stderr, opt
    for opt in (["--join-min-overlap", "7"], ["--join-max-overlap", "4097"], ["--join-kmer", "7"], ["--join-kmer", "129"], ["--join-min-count", "0"],
                ["--join-min-overlap", "50", "--join-max-overlap", "40"]):
        r = subprocess.run(base + ["--scaffold", f["j.fa"], "--join-overlaps"] + opt + [prefix + ".fa"], capture_output=True)
        assert r.returncode == 1, opt
    r = subprocess.run([host.CLI_PATH, "unitig"], capture_output=True)  # no READSFILE: the help text
    assert r.returncode == 0 and all(w in r.stdout for w in (b"--join-overlaps", b"--join-min-overlap", b"--join-max-overlap", b"--join-slack",
                                                              b"--join-kmer", b"--join-min-count", b"--joins=FILE", b"before any join"))
