"""Gap filling of `siga unitig --scaffold --gapfill` on the GPU (csrc/sigax_gapfill.hip) against the serial restatement of its rules
(tests/gapfill_cases.py::expected_gapfill): every case through the host form and through the device form over output buffers of
exactly their size with canaries behind them, on the forward-only and on the two-strand index; a subset in child processes
without the two-step tables and with 64-bit positions over small superblocks; once the unitig, pairs, scaffold and gapfill calls
enqueued on one stream with nothing in between; capacity; hostile tables; refusals."""
import ctypes as C
import functools
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch  # before the library loads: one HIP runtime per process

from oracle import pyoracle as po
from tests import gapfill_cases as gc
from tests import pair_cases as pp
from tests import scaffold_cases as sc
from tests import unitig_cases as uc
from tests.fixtures import CACHE, ROOT
from tests.golden import make_reads as mr

pytestmark = pytest.mark.gpu
CANARY = 64


def _open(reads, both):
    """the reads' index, oracle-built, from memory: the forward strand alone, or both strands"""
    import siga_amd
    from siga_amd import _lib
    seqs = [r.decode() for r in reads]
    f = po.Index.build(seqs)
    if both:
        r = po.Index.build(seqs, reverse=True)
        return siga_amd.FMIndexPair.from_memory(f.runs(), r.runs(), len(f), f.nstrings, resident=False)
    runs = np.ascontiguousarray(f.runs(), dtype=np.uint8)
    h = C.c_void_p()
    assert _lib.lib().sigax_index_open_mem(runs.ctypes.data, len(runs), None, 0, len(f), f.nstrings, None, None, 0, C.byref(h)) == 0, _lib.last_error()
    return siga_amd.FMIndexPair(h.value)


def _up(a):
    a = np.frombuffer(a, dtype=np.uint8) if isinstance(a, bytes) else np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return torch.from_numpy(a.copy()).to("cuda:0") if a.size else torch.zeros(16, dtype=torch.uint8, device="cuda:0")


def _out(nbytes):
    return torch.full((nbytes + CANARY,), 0xEE, dtype=torch.uint8, device="cuda:0")


def _gopts(o):
    from siga_amd import _lib
    return _lib.GapfillOpts(0, o["k"], o["min_count"], o["slack"], o["max_fill"], 0)


def _same(got, exp, what, seqs=True):
    st = [int(x) for x in got["status"]]
    print(what, "status", st, "expected", exp["status"])
    assert st[:19] + st[20:] == exp["status"][:19] + exp["status"][20:], what
    assert st[19] > 0 or st[17] == 0, what  # a step asks for sectors
    assert [int(x) for x in got["sc_offs"]] == exp["sc_offs"], what
    assert [tuple(int(x) for x in p) for p in got["layout"].tolist()] == exp["layout"], what
    assert [tuple(int(x) for x in g) for g in got["gaps"].tolist()] == exp["gaps"], what
    if seqs and exp["seqs"] is not None:
        assert got["seqs"] is not None and bytes(got["seqs"]) == exp["seqs"], what


def _padded(values, n, dtype):
    a = np.zeros(n, dtype=dtype)
    v = np.array(values, dtype=dtype)[:n]
    a[:len(v)] = v
    return a


def _enqueue(L, ix, mu, nu_ptr, so_ptr, us_ptr, us_bytes, ns_ptr, slo_ptr, lay_ptr, o, capacity, walk_bases, stream):
    """sigax_gapfill_device over output buffers of exactly their size plus CANARY bytes of 0xEE -> (buffers, sizes)"""
    from siga_amd import _lib
    wb = C.c_uint64()
    assert L.sigax_gapfill_workspace(mu, walk_bases, C.byref(wb)) == 0
    sizes = {"sc_offs": 8 * (mu + 1), "layout": 16 * mu, "gaps": 32 * mu, "status": 192, "work": wb.value}
    if capacity is not None:
        sizes["seqs"] = capacity
    d = {k: _out(v) for k, v in sizes.items()}
    torch.cuda.synchronize()
    opts = _gopts(o)
    rc = L.sigax_gapfill_device(ix.handle, nu_ptr, mu, so_ptr, us_ptr, us_bytes, ns_ptr, slo_ptr, lay_ptr, C.byref(opts), d["sc_offs"].data_ptr(),
                                d["layout"].data_ptr(), d["seqs"].data_ptr() if capacity is not None else None, capacity or 0, d["gaps"].data_ptr(),
                                d["status"].data_ptr(), d["work"].data_ptr(), wb.value, walk_bases, stream)
    assert rc == 0, _lib.last_error()
    return d, sizes


def _collect(d, sizes, what):
    """the results, and that nothing behind them was written: the canaries, the table entries beyond the scaffolds, the placements
    and the gaps, and all of the bases buffer when the status says they were not written"""
    from siga_amd import _lib
    h = {k: v.cpu().numpy() for k, v in d.items()}
    status = h["status"][:192].view(np.uint64)
    ng, total, s = int(status[0]), int(status[16]), int(status[22])
    got = {"status": status, "sc_offs": h["sc_offs"][:8 * (s + 1)].view(np.uint64), "gaps": h["gaps"][:32 * ng].view(_lib.GAP_DTYPE), "seqs": None}
    lay = h["layout"][:sizes["layout"]].view(_lib.PLACEMENT_DTYPE)
    placed = len(lay)
    while placed and h["layout"][16 * (placed - 1):16 * placed].tobytes() == b"\xee" * 16:
        placed -= 1
    got["layout"] = lay[:placed]
    used = {"sc_offs": 8 * (s + 1), "layout": 16 * placed, "gaps": 32 * ng, "status": 192}
    if "seqs" in sizes:
        written = int(status[20]) == 0
        assert written == (total <= sizes["seqs"])
        used["seqs"] = total if written else 0
        got["seqs"] = h["seqs"][:total].tobytes() if written else None
    for k in used:
        rest = h[k][used[k]:].tobytes()
        assert len(rest) >= CANARY and rest == b"\xee" * len(rest), "%s: bytes after %s were written" % (what, k)
    assert h["work"][sizes["work"]:].tobytes() == b"\xee" * CANARY, what
    return got


def _walk_bases(c):
    if c.get("short_scratch") is not None:
        return gc.scratch_needed(c) - c["short_scratch"]
    return gc.scratch_needed(c) if c.get("max_walk_bases") is None else c["max_walk_bases"]


def _device(ix, c, what, capacity="exact", nu_dev=None, ns_dev=None, walk_bases=None, useqs_bytes=None, compare=True):
    """the device form over the case's tables in buffers of exactly their size -> (expected_gapfill's dict, what came back)"""
    from siga_amd import _lib
    L = _lib.lib()
    res, scaf = c["res"], c["scaf"]
    mu = len(res["seq_offs"]) - 1
    s = len(scaf["sc_lay_offs"]) - 1
    walk_bases = _walk_bases(c) if walk_bases is None else walk_bases
    kw = dict(n_unitigs=nu_dev, n_scaffolds=ns_dev, max_walk_bases=walk_bases, useqs_bytes=useqs_bytes)
    exp, cap = None, capacity
    if compare:
        exp = gc.expected_gapfill(c["reads"], res, scaf, c["opts"], **kw)
        cap = exp["status"][16] if capacity == "exact" else capacity
        exp = gc.expected_gapfill(c["reads"], res, scaf, c["opts"], sseqs_capacity=cap or 0, **kw)
    counts = _up(np.array([mu if nu_dev is None else nu_dev, s if ns_dev is None else ns_dev], dtype=np.uint64))
    d_so, d_us = _up(np.array(res["seq_offs"], dtype=np.uint64)), _up(res["useqs"])
    d_slo = _up(_padded(scaf["sc_lay_offs"], mu + 1, np.uint64))
    lay = np.zeros(mu, dtype=_lib.PLACEMENT_DTYPE)
    for i, p in enumerate(scaf["layout"][:mu]):
        lay[i] = tuple(p)
    d_lay = _up(lay)
    d, sizes = _enqueue(L, ix, mu, counts.data_ptr(), d_so.data_ptr(), d_us.data_ptr(), len(res["useqs"]) if useqs_bytes is None else useqs_bytes,
                        counts.data_ptr() + 8, d_slo.data_ptr(), d_lay.data_ptr(), c["opts"], cap, walk_bases, None)
    torch.cuda.synchronize()
    got = _collect(d, sizes, what)
    if compare:
        _same(got, exp, what + ", device", seqs=exp["status"][20] == 0)
        if exp["status"][20]:
            assert got["seqs"] is None
    return exp, got


def _host(ix, c, what):
    import siga_amd
    exp = gc.case_expected(c)
    o = c["opts"]
    mw = None if c.get("short_scratch") is None and c.get("max_walk_bases") is None else _walk_bases(c)
    got = siga_amd.scaffolds_gapfill(ix, c["res"], c["scaf"], k=o["k"], min_count=o["min_count"], slack=o["slack"], max_fill=o["max_fill"],
                                     max_walk_bases=mw)
    _same(got, exp, what + ", host")
    assert got["sc_lay_offs"].tolist() == c["scaf"]["sc_lay_offs"] and got["sc_flags"].tolist() == c["scaf"]["sc_flags"]
    return exp


def _run_cases(cases):
    """every case through both forms on both kinds of index, one pair of indexes per read set"""
    by_reads = {}
    for c in cases:
        by_reads.setdefault(c["reads_key"], []).append(c)
    for key, group in by_reads.items():
        for both in (False, True):
            ix = _open(group[0]["reads"], both)
            try:
                for c in group:
                    what = "%s, %s index" % (c["name"], "two-strand" if both else "forward-only")
                    _host(ix, c, what)
                    _device(ix, c, what)
            finally:
                ix.close()


@pytest.mark.parametrize("k", gc.KS)
def test_hand_built(k):
    _run_cases(gc.hand_built(k))


@pytest.mark.parametrize("count,k", [(70, 15), (300, 15), (70, 31)])
def test_many_gaps_across_waves_and_workgroups(count, k):
    c = gc.many_gaps(count, k)
    _run_cases([c])
    assert gc.case_expected(c)["status"][0] == count + 1


@pytest.mark.parametrize("block", range(5))
def test_random_cases(block):
    _run_cases([gc.random_case(s) for s in range(20 * block, 20 * block + 20)])


@pytest.mark.parametrize("k", [31, 128])
def test_long_fill(k):
    """fills of 5000 bases, one by the forward and one by the reverse walk: every byte of them is compared (_same)"""
    c = gc.long_fill(k)
    _run_cases([c])
    assert [g[4:6] + g[8:9] for g in gc.case_expected(c)["gaps"]] == [(5000, gc.C["FILLED"], 0), (5000, gc.C["FILLED"], 1)]


# ---- other forms of the index, in child processes ----
def _child(env_extra, ids):
    env = dict(os.environ, **env_extra)
    what = [os.path.join(ROOT, "tests", "test_gpu_gapfill.py") + "::" + i for i in ids]
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q"] + what, cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


SUBSET = ["test_hand_built[15]", "test_hand_built[64]", "test_random_cases[0]"]


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
    c = next(x for x in gc.hand_built(31) if x["kind"] == "three_gaps")
    ix = _open(c["reads"], False)
    try:
        total = gc.case_expected(c)["status"][16]
        assert _device(ix, c, "one byte short", capacity=total - 1)[0]["status"][20] == 1
        assert _device(ix, c, "exact", capacity=total)[0]["status"][20] == 0
        assert _device(ix, c, "room to spare", capacity=total + 100)[0]["status"][20] == 0
        assert _device(ix, c, "no bases asked for", capacity=None)[0]["status"][20] == 1
        need = gc.scratch_needed(c)
        exp, _ = _device(ix, c, "no scratch at all", walk_bases=0)
        assert exp["status"][1 + gc.C["NO_ROOM"]] == 3 and exp["status"][21] == 1 and exp["status"][17] == 0
        exp, _ = _device(ix, c, "scratch for the first gap", walk_bases=need // 3)
        assert 0 < exp["status"][1 + gc.C["NO_ROOM"]] < 3
    finally:
        ix.close()


# ---- hostile tables ----
def test_hostile_tables():
    c = dict(next(x for x in gc.hand_built(15) if x["kind"] == "three_gaps"))
    ix = _open(c["reads"], False)
    try:
        mu = len(c["res"]["seq_offs"]) - 1
        # counts on the device above their capacities are taken as the capacities; below them, the rest of the tables is unread
        assert _device(ix, c, "unitigs beyond the capacity", nu_dev=1 << 40)[0]["status"][0] == 3
        exp, _ = _device(ix, c, "scaffolds beyond the capacity", ns_dev=1 << 33)  # (the table's last entry, a zero here, is the placements)
        assert exp["status"][22] == mu and exp["status"][0] == 0
        exp, _ = _device(ix, c, "fewer unitigs than the layout names", nu_dev=2)
        assert exp["status"][1 + gc.C["MALFORMED"]] >= 1
        assert _device(ix, c, "no scaffolds", ns_dev=0)[0]["status"][:1] == [0]
        # a layout that claims more bases than useqs has: the placements that reach beyond are bad
        exp, _ = _device(ix, c, "useqs cut short", useqs_bytes=len(c["res"]["useqs"]) - 5)
        assert exp["status"][1 + gc.C["MALFORMED"]] >= 1
        # unitig ids beyond the tables
        bad = dict(c, scaf=dict(c["scaf"], layout=[(p[0] if i != 1 else 0xFFFFFFF0, p[1], p[2]) for i, p in enumerate(c["scaf"]["layout"])]))
        exp, _ = _device(ix, bad, "a unitig id beyond the tables")
        assert exp["status"][1 + gc.C["MALFORMED"]] == 2
        # offsets and tables that do not ascend: the call ends, the status is the rules', nothing behind a buffer is written
        lay = c["scaf"]["layout"]
        for name, scaf, res in (
                ("descending offsets", dict(c["scaf"], layout=[(p[0], p[1], (1 << 40) - 7 * i * p[2]) for i, p in enumerate(lay)]), c["res"]),
                ("lay_offs that do not ascend", dict(c["scaf"], sc_lay_offs=[0, 3, 1, 4], sc_flags=[0, 0, 0]), c["res"]),
                ("lay_offs beyond the placements", dict(c["scaf"], sc_lay_offs=[2, 1 << 50]), c["res"]),
                ("descending seq_offs", c["scaf"], dict(c["res"], seq_offs=[0, 90, 40, 200, len(c["res"]["useqs"])]))):
            exp = gc.expected_gapfill(c["reads"], res, scaf, c["opts"], max_walk_bases=1 << 12, sseqs_capacity=0)
            for cap in (0, 64, 1 << 16):
                got = _device(ix, dict(c, scaf=scaf, res=res), name, capacity=cap, walk_bases=1 << 12, compare=False)[1]
                st = [int(x) for x in got["status"]]
                print(name, cap, st, exp["status"])
                assert st[:19] + st[21:] == exp["status"][:19] + exp["status"][21:] and st[20] == (1 if st[16] > cap else 0), (name, cap)
                assert [tuple(int(x) for x in g) for g in got["gaps"].tolist()] == exp["gaps"], (name, cap)
                assert [int(x) for x in got["sc_offs"]] == exp["sc_offs"], (name, cap)
    finally:
        ix.close()


def test_no_unitigs():
    import siga_amd
    from siga_amd import _lib
    c = next(x for x in gc.hand_built(15) if x["kind"] == "plain")
    ix = _open(c["reads"], False)
    try:
        got = siga_amd.scaffolds_gapfill(ix, {"seq_offs": [0], "useqs": b""}, {"sc_lay_offs": [0], "sc_flags": [], "layout": []}, k=15)
        assert got["status"].tolist() == [0] * 24 and got["sc_offs"].tolist() == [0] and len(got["gaps"]) == 0 and len(got["seqs"]) == 0
        st = _out(192)
        opts = _gopts(c["opts"])
        assert _lib.lib().sigax_gapfill_device(ix.handle, None, 0, None, None, 0, None, None, None, C.byref(opts), None, None, None, 0, None,
                                               st.data_ptr(), None, 0, 0, None) == 0
        torch.cuda.synchronize()
        assert st.cpu().numpy().tobytes() == b"\0" * 192 + b"\xee" * CANARY
    finally:
        ix.close()


# ---- the four calls on one stream ----
def test_four_calls_on_one_stream():
    """sigax_unitigs_chimeric_device, sigax_unitigs_pairs_device, sigax_scaffold_device and sigax_gapfill_device enqueued on one
    stream, nothing in between: the gapfill call reads both counts, the unitig tables and bases and the scaffold tables where the
    calls before it leave them"""
    import siga_amd
    from siga_amd import _lib
    from tests import test_gpu_scaffold as ts
    from tests import test_gpu_unitig_pairs as tp
    L = _lib.lib()
    seen = 0
    for seed in (3, 7, 18):
        case, res, pairs, o = ts._through_the_calls(seed)
        exp_sc = sc.expected_scaffolds(res, pairs["links"], pairs["status"], o)
        scaf = {"sc_lay_offs": exp_sc["sc_lay_offs"], "sc_flags": exp_sc["sc_flags"], "layout": exp_sc["layout"]}
        reads = tuple(bytes(r) if not isinstance(r, str) else r.encode() for r in case["reads"])
        go = dict(gc.DEFAULT_OPTS, k=15, min_count=1, slack=20)
        n = len(reads)
        # the tables as the calls leave them: n-entry buffers, so the restatement sees the same capacity
        res_n = {"seq_offs": _padded(res["seq_offs"], n + 1, np.uint64).tolist(), "useqs": bytes(res["useqs"])}
        nu = len(res["uflags"])
        exp = gc.expected_gapfill(reads, res_n, scaf, go, n_unitigs=nu, n_scaffolds=exp_sc["status"][0], max_walk_bases=1 << 16,
                                  useqs_bytes=len(bytes(res["useqs"])))
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
            d, sizes = _enqueue(L, ix, n, u["status"].data_ptr(), u["seq_offs"].data_ptr(), u["useqs"].data_ptr(), nb, s["status"].data_ptr(),
                                s["sc_lay_offs"].data_ptr(), s["layout"].data_ptr(), go, exp["status"][16], 1 << 16, st)
            torch.cuda.synchronize()
        finally:
            L.sigax_stream_destroy(0, st)
            ix.close()
        got = _collect(d, sizes, case["name"])
        # beyond the unitigs the unitig call's seq_offs hold canary bytes, which the rules never read
        _same(got, exp, case["name"] + ", chained")
        seen += exp["status"][0]
    assert seen > 0


# ---- refusals ----
def test_refusals():
    from siga_amd import _lib
    L = _lib.lib()
    E = _lib.SIGAX_E_ARG
    c = next(x for x in gc.hand_built(15) if x["kind"] == "plain")
    ix = _open(c["reads"], False)
    try:
        wb = C.c_uint64()
        assert L.sigax_gapfill_workspace(1 << 31, 10, C.byref(wb)) == E and "max_unitigs" in _lib.last_error()
        assert L.sigax_gapfill_workspace(10, 1 << 43, C.byref(wb)) == E and "max_walk_bases" in _lib.last_error()
        assert L.sigax_gapfill_workspace(10, 10, None) == E
        assert L.sigax_gapfill_workspace(0, 0, C.byref(wb)) == 0 and wb.value == 0
        mu, walk = 8, 256
        assert L.sigax_gapfill_workspace(mu, walk, C.byref(wb)) == 0
        b = [torch.zeros(4096, dtype=torch.uint8, device="cuda:0") for _ in range(11)]
        p = [t.data_ptr() for t in b]
        work = torch.zeros(wb.value, dtype=torch.uint8, device="cuda:0")
        z = None
        names = ("nu", "so", "us", "ns", "slo", "lay", "sco", "layo", "seqs", "gaps", "st")
        full = {"nu": "d_n_unitigs", "so": "d_seq_offs", "us": "d_useqs", "ns": "d_n_scaffolds", "slo": "d_sc_lay_offs", "lay": "d_sc_layout",
                "sco": "d_sc_offs", "layo": "d_sc_layout_out", "seqs": "d_sseqs", "gaps": "d_gaps", "st": "d_status24"}

        def opts(flags=0, k=15, mc=3, slack=10, max_fill=100, reserved=0):
            return C.byref(_lib.GapfillOpts(flags, k, mc, slack, max_fill, reserved))

        def dev(o="usual", handle=ix.handle, w=work.data_ptr(), nbytes=wb.value, nmu=mu, cap=64, wbases=walk, **over):
            a = dict(zip(names, p))
            a.update(over)
            return L.sigax_gapfill_device(handle, a["nu"], nmu, a["so"], a["us"], 4096, a["ns"], a["slo"], a["lay"], opts() if o == "usual" else o,
                                          a["sco"], a["layo"], a["seqs"], cap, a["gaps"], a["st"], w, nbytes, wbases, z)

        assert dev(o=None) == E and dev(handle=None) == E
        assert dev(o=opts(flags=1)) == E and "flags" in _lib.last_error()
        assert dev(o=opts(reserved=1)) == E
        for k in (0, 7, 129):
            assert dev(o=opts(k=k)) == E and "k " in _lib.last_error()
        assert dev(o=opts(mc=0)) == E and "min_count" in _lib.last_error()
        assert dev(o=opts(slack=1 << 31)) == E and "slack" in _lib.last_error()
        assert dev(o=opts(max_fill=1 << 31)) == E and "max_fill" in _lib.last_error()
        assert dev(nmu=1 << 31) == E and "max_unitigs" in _lib.last_error()
        assert dev(cap=1 << 43) == E and "sseqs_capacity" in _lib.last_error()
        assert dev(wbases=1 << 43) == E and "max_walk_bases" in _lib.last_error()
        assert dev(nbytes=wb.value - 1) == E and "workspace" in _lib.last_error()
        assert dev(wbases=walk + 16) == E and "workspace" in _lib.last_error()
        for k in names:
            if k != "seqs":
                assert dev(**{k: z}) == E and full[k] in _lib.last_error(), k
        assert dev(seqs=z) == E and "d_sseqs" in _lib.last_error()  # NULL with a capacity
        assert dev(seqs=z, cap=0) == 0
        assert dev(w=z) == E and "d_work" in _lib.last_error()
        assert dev(layo=p[names.index("lay")]) == E and "overlaps" in _lib.last_error()
        assert dev(layo=p[names.index("lay")] + 16 * (mu - 1)) == E and "overlaps" in _lib.last_error()
        for k, off in (("nu", 4), ("so", 4), ("ns", 4), ("slo", 4), ("sco", 4), ("st", 4), ("lay", 8), ("layo", 8), ("gaps", 8), ("us", 8), ("seqs", 8)):
            assert dev(**{k: p[0] + 2048 + off}) == E and "aligned" in _lib.last_error() and full[k] in _lib.last_error(), k
        assert dev(w=work.data_ptr() + 8) == E and "aligned" in _lib.last_error()
        assert dev(o=opts(k=8)) == 0 and dev(o=opts(k=128)) == 0, _lib.last_error()  # (everything zero: no scaffolds)
        torch.cuda.synchronize()
        assert b[names.index("st")].cpu().numpy()[:192].view(np.uint64).tolist() == [0] * 24
        # the host form
        ptrs = [C.c_void_p() for _ in range(4)]
        ng = C.c_uint64()
        s24 = (C.c_uint64 * 24)()
        so, slo = (C.c_uint64 * 3)(0, 20, 45), (C.c_uint64 * 2)(0, 2)
        lay = np.array([(0, 0, 0), (1, 0, 23)], dtype=_lib.PLACEMENT_DTYPE)
        us = C.create_string_buffer(c["genome"][:20] + c["genome"][23:48])

        def host(o, handle=ix.handle, nu=2, so_=so, us_=us, ns=1, slo_=slo, lay_=lay.ctypes.data, walk_=_lib.SIGAX_GAPFILL_AUTO, out=None, ng_=C.byref(ng),
                 s24_=s24):
            out = [C.byref(x) for x in ptrs] if out is None else out
            return L.sigax_gapfill_host(handle, nu, so_, us_, ns, slo_, lay_, o, walk_, out[0], out[1], out[2], out[3], ng_, s24_)

        def free():
            for x in ptrs:
                L.sigax_free(x)

        assert host(opts()) == 0 and ng.value == 1 and list(s24)[:2] == [1, 1] and s24[16] == 48 and s24[20] == 0, (_lib.last_error(), list(s24))
        free()
        assert host(None) == E and host(opts(k=7)) == E and host(opts(), handle=None) == E
        assert host(opts(), ng_=None) == E and host(opts(), s24_=None) == E
        assert host(opts(), out=[None] + [C.byref(x) for x in ptrs[1:]]) == E
        assert host(opts(), so_=z) == E and host(opts(), slo_=z) == E
        assert host(opts(), us_=z) == E and "useqs" in _lib.last_error()
        assert host(opts(), lay_=z) == E and "sc_layout" in _lib.last_error()
        assert host(opts(), ns=3) == E and "n_scaffolds" in _lib.last_error()
        assert host(opts(), slo_=(C.c_uint64 * 2)(0, 3)) == E and "sc_lay_offs" in _lib.last_error()
        assert host(opts(), nu=1 << 31) == E
        assert host(opts(), walk_=1 << 43) == E and "max_walk_bases" in _lib.last_error()
        assert host(opts(), out=[C.byref(ptrs[0]), C.byref(ptrs[1]), None, C.byref(ptrs[3])]) == 0  # the tables alone
        free()
        assert host(opts(), nu=0, so_=z, us_=z, ns=0, slo_=z, lay_=z) == 0 and ng.value == 0 and list(s24) == [0] * 24
        free()
    finally:
        ix.close()


# ---- the command line, once: a genome with two repeats of two copies each that are longer than the minimum overlap, so that they
# break the unitigs, and shorter than the walks' k, so that the walks pass them; the unitig between two neighbouring copies is too
# short for the scaffolds, which leaves a gap of some 170 bases where it lay ----
E2E_GENOME, E2E_LEN, E2E_INSERT, E2E_REPEAT, E2E_STEP, E2E_M, E2E_MIN_UNITIG, E2E_SEED = 6000, 60, 400, 28, 6, 25, 300, 33
E2E_COPIES = ((1500, 4000), (1700, 4200))


@functools.lru_cache(maxsize=None)
def _e2e(seed):
    """-> (genome, names, reads): a read pair every E2E_STEP bases, the mates in random order"""
    rng = random.Random(seed)
    while True:
        g = bytearray(rng.choice(b"ACGT") for _ in range(E2E_GENOME))
        for src, dst in E2E_COPIES:
            g[dst:dst + E2E_REPEAT] = g[src:src + E2E_REPEAT]
        g = bytes(g)
        masked = g
        for _, dst in sorted(E2E_COPIES, reverse=True):  # (without the second copies)
            masked = masked[:dst] + masked[dst + E2E_REPEAT:]
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
    d = os.path.join(CACHE, "unitig_gapfill_e2e_%d" % seed)
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


def test_cli(tmp_path):
    import siga_amd
    from siga_amd import host
    prefix = _e2e_files(E2E_SEED)
    genome, names, reads = _e2e(E2E_SEED)
    fa, lay, pj, sfa, slay, gfa, glay, gps = (str(tmp_path / f) for f in ("u.fa", "u.layout", "u.pairs.json", "s.fa", "s.layout", "g.fa", "g.layout", "g.gaps"))
    base = [host.CLI_PATH, "unitig", "-m", str(E2E_M), "-p", prefix, "-o", fa, "--layout", lay, "--pairs", pj, "--insert-size", str(E2E_INSERT),
            "--min-scaffold-unitig", str(E2E_MIN_UNITIG)]
    r = subprocess.run(base + ["--scaffold", sfa, "--scaffold-layout", slay, prefix + ".fa"], capture_output=True)
    assert r.returncode == 0 and b"filled" not in r.stderr, r.stderr.decode()
    # the unitigs as the layout and the FASTA give them; the scaffolds as the restatements of the pairs and scaffold calls give them
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
    exp_sc = sc.expected_scaffolds(res, pairs["links"], pairs["status"], {"insert_size": E2E_INSERT, "min_unitig_bases": E2E_MIN_UNITIG})
    # without --gapfill every byte is the scaffold call's
    efa, elay = sc.render(exp_sc)
    assert open(sfa).read() == efa and open(slay).read() == elay
    r = subprocess.run(base + ["--scaffold", gfa, "--scaffold-layout", glay, "--gapfill", "--gaps", gps, prefix + ".fa"], capture_output=True)
    assert r.returncode == 0 and b"gaps, " in r.stderr and b"filled with" in r.stderr, r.stderr.decode()
    scaf = {"sc_lay_offs": exp_sc["sc_lay_offs"], "sc_flags": exp_sc["sc_flags"], "layout": exp_sc["layout"]}
    exp = gc.expected_gapfill(tuple(reads), res, scaf)
    print("unitigs", [len(s) for s in useqs], "scaffold status", exp_sc["status"], "gapfill status", exp["status"], "gaps", exp["gaps"])
    gfa_t, glay_t, gps_t = gc.render(exp, res["seq_offs"])
    assert open(gfa).read() == gfa_t and open(glay).read() == glay_t and open(gps).read() == gps_t
    # the repeat is shorter than k: the walks pass it, and what they put in is the genome's
    assert exp["status"][0] >= 1 and exp["status"][1] >= 1 and exp["status"][15] < exp_sc["status"][12]
    both = genome + b"\n" + uc.revcomp(genome)
    for s in range(exp["status"][22]):
        filled = all(g[5] == gc.C["FILLED"] for g in exp["gaps"] if g[0] == s)
        if filled:
            assert exp["seqs"][exp["sc_offs"][s]:exp["sc_offs"][s + 1]] in both, s
    # refusals and the help text
    r = subprocess.run(base + ["--gapfill", prefix + ".fa"], capture_output=True)
    assert r.returncode == 1 and b"--scaffold" in r.stderr
    for opt in (["--gap-kmer", "21"], ["--gap-min-count", "2"], ["--gap-slack", "5"], ["--gap-max-fill", "50"], ["--gaps", gps]):
        r = subprocess.run(base + ["--scaffold", gfa] + opt + [prefix + ".fa"], capture_output=True)
        assert r.returncode == 1 and b"--gapfill" in r.stderr, opt
    for opt in (["--gap-kmer", "7"], ["--gap-kmer", "129"], ["--gap-min-count", "0"]):
        r = subprocess.run(base + ["--scaffold", gfa, "--gapfill"] + opt + [prefix + ".fa"], capture_output=True)
        assert r.returncode == 1, opt
    r = subprocess.run([host.CLI_PATH, "unitig"], capture_output=True)  # no READSFILE: the help text
    assert r.returncode == 0 and all(w in r.stdout for w in (b"--gapfill", b"--gap-kmer", b"--gap-min-count", b"--gap-slack", b"--gap-max-fill",
                                                              b"--gaps=FILE"))
