"""`siga unitig --scaffold --join-overlaps --join-mismatches` on the GPU (csrc/sigax_join.hip) against the serial restatement of its
rules (tests/join_approx_cases.py::expected_join_approx), exactly: tables, bases, records, mm and all 24 status entries.  Every case
goes through the host form and through the device form over output buffers of exactly their size with canaries behind them, on
the forward-only and on the two-strand index; a subset in child processes with 64-bit positions and without the two-step tables;
the exact call through the new entry points; the call behind a scaffold call on one stream; capacity; refusals; the command line."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch  # before the library loads: one HIP runtime per process

from tests import join_approx_cases as ja
from tests import join_cases as jc
from tests import scaffold_cases as sc
from tests.fixtures import ROOT

pytestmark = pytest.mark.gpu


def _tj():
    from tests import test_gpu_join as tj
    return tj


def _aopts(o):
    from siga_amd import _lib
    return _lib.JoinApproxOpts(0, o["min_overlap"], o["max_overlap"], o["slack"], o["k"], o["min_count"], o.get("max_mismatches", 0),
                               o.get("mismatch_permille", 50), 0)


def _same(got, exp, what, seqs=True):
    st = [int(x) for x in got["status"]]
    print(what, "status", st, "expected", exp["status"], "mm", [int(x) for x in got["mm"]])
    assert st == exp["status"], what
    assert [int(x) for x in got["sc_offs"]] == exp["sc_offs"], what
    assert [tuple(int(x) for x in p) for p in got["layout"].tolist()] == exp["layout"], what
    assert [tuple(int(x) for x in g) for g in got["joins"].tolist()] == exp["joins"], what
    assert [int(x) for x in got["mm"]] == exp["mm"], what
    if seqs and exp["seqs"] is not None:
        assert got["seqs"] is not None and bytes(got["seqs"]) == exp["seqs"], what


def _enqueue(L, ix, mu, nu_ptr, so_ptr, ns_ptr, sco_ptr, slo_ptr, lay_ptr, seqs_ptr, seqs_bytes, o, capacity, stream):
    """sigax_join_approx_device over output buffers of exactly their size plus CANARY bytes of 0xEE -> (buffers, sizes)"""
    from siga_amd import _lib
    tj = _tj()
    wb = C.c_uint64()
    assert L.sigax_join_approx_workspace(mu, C.byref(wb)) == 0
    sizes = {"sc_offs": 8 * (mu + 1), "layout": 16 * mu, "joins": 32 * mu, "mm": 4 * mu, "status": 192, "work": wb.value}
    if capacity is not None:
        sizes["seqs"] = capacity
    d = {k: tj._out(v) for k, v in sizes.items()}
    torch.cuda.synchronize()
    opts = _aopts(o)
    rc = L.sigax_join_approx_device(ix.handle, nu_ptr, mu, so_ptr, ns_ptr, sco_ptr, slo_ptr, lay_ptr, seqs_ptr, seqs_bytes, C.byref(opts),
                                    d["sc_offs"].data_ptr(), d["layout"].data_ptr(), d["seqs"].data_ptr() if capacity is not None else None, capacity or 0,
                                    d["joins"].data_ptr(), d["mm"].data_ptr(), d["status"].data_ptr(), d["work"].data_ptr(), wb.value, stream)
    assert rc == 0, _lib.last_error()
    return d, sizes


def _collect(d, sizes, what):
    """the results, and that nothing beyond S, P and the gaps was written: the canaries, the rest of every table, and all of the
    bases buffer -- patches included -- when the status says the bases were not written"""
    from siga_amd import _lib
    CANARY = _tj().CANARY
    h = {k: v.cpu().numpy() for k, v in d.items()}
    status = h["status"][:192].view(np.uint64)
    ng, total, s = int(status[0]), int(status[11]), int(status[15])
    got = {"status": status, "sc_offs": h["sc_offs"][:8 * (s + 1)].view(np.uint64), "joins": h["joins"][:32 * ng].view(_lib.JOIN_DTYPE),
           "mm": h["mm"][:4 * ng].view(np.uint32), "seqs": None}
    lay = h["layout"][:sizes["layout"]].view(_lib.PLACEMENT_DTYPE)
    placed = len(lay)
    while placed and h["layout"][16 * (placed - 1):16 * placed].tobytes() == b"\xee" * 16:
        placed -= 1
    got["layout"] = lay[:placed]
    used = {"sc_offs": 8 * (s + 1), "layout": 16 * placed, "joins": 32 * ng, "mm": 4 * ng, "status": 192}
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


def _device(ix, c, what, capacity="exact", opts=None):
    """the device form over the case's tables in buffers of exactly their size -> (the restatement's dict, what came back)"""
    from siga_amd import _lib
    tj = _tj()
    L = _lib.lib()
    res, scaf, o = c["res"], c["scaf"], opts or c["opts"]
    mu = len(res["seq_offs"]) - 1
    s = len(scaf["sc_lay_offs"]) - 1
    exp = ja.expected_join_approx(c["reads"], res, scaf, o)
    cap = exp["status"][11] if capacity == "exact" else capacity
    exp = ja.expected_join_approx(c["reads"], res, scaf, o, sseqs_capacity=cap or 0)
    counts = tj._up(np.array([mu, s], dtype=np.uint64))
    d_so = tj._up(np.array(res["seq_offs"], dtype=np.uint64))
    d_sco = tj._up(tj._padded(scaf["sc_offs"], mu + 1, np.uint64))
    d_slo = tj._up(tj._padded(scaf["sc_lay_offs"], mu + 1, np.uint64))
    lay = np.zeros(mu, dtype=_lib.PLACEMENT_DTYPE)
    for i, p in enumerate(scaf["layout"][:mu]):
        lay[i] = tuple(p)
    d_lay, d_seqs = tj._up(lay), tj._up(scaf["seqs"])
    d, sizes = _enqueue(L, ix, mu, counts.data_ptr(), d_so.data_ptr(), counts.data_ptr() + 8, d_sco.data_ptr(), d_slo.data_ptr(), d_lay.data_ptr(),
                        d_seqs.data_ptr(), len(scaf["seqs"]), o, cap, None)
    torch.cuda.synchronize()
    got = _collect(d, sizes, what)
    _same(got, exp, what + ", device", seqs=exp["status"][14] == 0)
    if exp["status"][14]:
        assert got["seqs"] is None
    return exp, got


def _host_call(ix, c, opts=None):
    import siga_amd
    o = opts or c["opts"]
    scaf = dict(c["scaf"], layout=np.array([tuple(p) for p in c["scaf"]["layout"]], dtype=siga_amd._lib.PLACEMENT_DTYPE))
    return siga_amd.scaffolds_join(ix, c["res"], scaf, min_overlap=o["min_overlap"], max_overlap=o["max_overlap"], slack=o["slack"], k=o["k"],
                                   min_count=o["min_count"], max_mismatches=o.get("max_mismatches", 0), mismatch_permille=o.get("mismatch_permille", 50))


def _run_cases(cases):
    """every case through both forms on both kinds of index, one pair of indexes per read set"""
    by_reads = {}
    for c in cases:
        by_reads.setdefault(c["reads_key"], []).append(c)
    for group in by_reads.values():
        for both in (False, True):
            ix = _tj()._open(group[0]["reads"], both)
            try:
                for c in group:
                    what = "%s, %s index" % (c["name"], "two-strand" if both else "forward-only")
                    _same(_host_call(ix, c), ja.case_expected(c), what + ", host")
                    _device(ix, c, what)
            finally:
                ix.close()


@pytest.mark.parametrize("k", ja.KS)
def test_planted(k):
    """choice, budget, word boundaries, the half rule, bytes outside ACGT, |J| < k, the minus strand, exact first, ambiguity, a
    unitig joined on both sides (tests/join_approx_cases.py::planted)"""
    cases = ja.planted(k)
    _run_cases(cases)
    for c in cases:
        exp = ja.case_expected(c)
        if c["genome_out"]:
            assert exp["seqs"] == c["genome"][c["span"][0]:c["span"][1]], c["name"]


def test_max_overlap_4096():
    """v = 4090 of max_overlap = 4096: every LDS word of both ends, lanes with 64 candidates each, 4120 support windows"""
    _run_cases([ja.long_overlap(31)])


@pytest.mark.parametrize("block", range(4))
def test_random_sweep(block):
    _run_cases([ja.random_case(s) for s in ja.RANDOM_SEEDS[12 * block:12 * block + 12]])


# ---- exact first ----
def test_zero_mismatches_is_the_exact_call():
    """max_mismatches = 0 through the new entry points against sigax_join_host byte for byte, over the exact join's own cases and
    over the planted ones; the gap with an exact v and an approximate v' is the exact call's, whatever max_mismatches"""
    tj = _tj()
    cases = jc.hand_built(31) + [jc.random_case(s) for s in range(10)] + ja.planted(31)
    by_reads = {}
    for c in cases:
        by_reads.setdefault(c["reads_key"], []).append(c)
    for group in by_reads.values():
        ix = tj._open(group[0]["reads"], False)
        try:
            for c in group:
                exact = {x: c["opts"][x] for x in jc.DEFAULT_OPTS}
                old = tj._host_call(ix, dict(c, opts=exact))
                zero = dict(exact, max_mismatches=0, mismatch_permille=250)
                exp, dev = _device(ix, c, c["name"] + ", no mismatches", opts=zero)
                # (scaffolds_join takes the old entry point for 0: the new one's host form directly)
                new = _approx_host(ix, c, zero)
                for got in (dev, new):
                    assert [int(x) for x in got["status"][:16]] == [int(x) for x in old["status"]] and [int(x) for x in got["status"][16:]] == [0] * 8
                    assert got["joins"].tobytes() == old["joins"].tobytes() and got["layout"].tobytes() == old["layout"].tobytes()
                    assert got["sc_offs"].tobytes() == old["sc_offs"].tobytes() and bytes(got["seqs"]) == bytes(old["seqs"])
                    assert [int(x) for x in got["mm"]] == [0] * len(old["joins"])
                if c["kind"] == "exact_and_approximate":
                    got = _host_call(ix, c)
                    assert got["joins"].tobytes() == old["joins"].tobytes() and bytes(got["seqs"]) == bytes(old["seqs"]) and got["mm"].tolist() == [0]
                    assert int(old["joins"][0]["overlap"]) == c["exact_v"]
        finally:
            ix.close()


def _approx_host(ix, c, o):
    """sigax_join_approx_host, whatever max_mismatches -> the dict of scaffolds_join"""
    from siga_amd import _lib
    from siga_amd.overlap import _copy_records
    L = _lib.lib()
    res, scaf = c["res"], c["scaf"]
    so = np.array(res["seq_offs"], dtype=np.uint64)
    sco, slo = np.array(scaf["sc_offs"], dtype=np.uint64), np.array(scaf["sc_lay_offs"], dtype=np.uint64)
    lay = np.array([tuple(p) for p in scaf["layout"]], dtype=_lib.PLACEMENT_DTYPE)
    sq = np.frombuffer(scaf["seqs"], dtype=np.uint8)
    po, play, ps, pj, pm = (C.c_void_p() for _ in range(5))
    nj = C.c_uint64()
    st = np.zeros(24, dtype=np.uint64)
    opts = _aopts(o)
    rc = L.sigax_join_approx_host(ix.handle, len(so) - 1, so.ctypes.data, len(slo) - 1, sco.ctypes.data, slo.ctypes.data, lay.ctypes.data, sq.ctypes.data,
                                  C.byref(opts), C.byref(po), C.byref(play), C.byref(ps), C.byref(pj), C.byref(nj), C.byref(pm), st.ctypes.data)
    assert rc == 0, _lib.last_error()
    try:
        return {"status": st, "sc_offs": _copy_records(po, len(slo), np.dtype(np.uint64)), "layout": _copy_records(play, int(slo[-1]), _lib.PLACEMENT_DTYPE),
                "joins": _copy_records(pj, nj.value, _lib.JOIN_DTYPE), "mm": _copy_records(pm, nj.value, np.dtype(np.uint32)),
                "seqs": _copy_records(ps, int(st[11]), np.dtype(np.uint8))}
    finally:
        for p in (po, play, ps, pj, pm):
            L.sigax_free(p)


# ---- other forms of the index, in child processes ----
def _child(env_extra, ids):
    env = dict(os.environ, **env_extra)
    what = [os.path.join(ROOT, "tests", "test_gpu_join_approx.py") + "::" + i for i in ids]
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q"] + what, cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


SUBSET = ["test_planted[15]", "test_planted[128]", "test_random_sweep[0]", "test_max_overlap_4096"]


def test_without_two_step_tables():
    _child({"SIGAX_TWO_STEP": "0"}, SUBSET[1:3])


def test_wide_positions_small_superblocks():
    lib = os.path.join(ROOT, "build", "libsigax_super12.so")
    assert os.path.exists(lib)
    _child({"SIGAX_FORCE_WIDE": "1", "SIGAX_LIB": lib}, SUBSET)


# ---- the device form ----
def test_behind_a_scaffold_call_on_one_stream():
    """sigax_scaffold_device and sigax_join_approx_device enqueued on one stream with nothing in between: the join reads the number
    of scaffolds, the tables and the bases where the scaffold call leaves them, in buffers with room for more unitigs than there are"""
    from siga_amd import _lib
    from tests import test_gpu_scaffold as ts
    from tests import test_gpu_unitig_pairs as tp
    tj = _tj()
    L = _lib.lib()
    cases = [c for c in ja.planted(31) if c["kind"] in ("one_in_each_far_apart", "middle_joined_on_both_sides")]
    ix = tj._open(cases[0]["reads"], False)
    try:
        for c in cases:
            # the unitigs as placed, cut from the case's scaffold bases (substitutions included) and numbered in that order, so that
            # the path begins at unitig 0 and every unitig lies forward; links whose estimate is negative, so that min_gap is laid
            lay, old_so = c["scaf"]["layout"], c["res"]["seq_offs"]
            nu, mu = len(lay), len(lay) + 4
            useqs = [c["scaf"]["seqs"][off:off + old_so[u + 1] - old_so[u]] for u, _, off in lay]
            so = [0]
            for b in useqs:
                so.append(so[-1] + len(b))
            res = {"seq_offs": so, "uflags": [0] * nu, "useqs": b"".join(useqs)}
            links = sorted(sc.path_links(list(range(nu)), [False] * nu, spans=[500] * nu))
            o = dict(sc.DEFAULT_OPTS, insert_size=100, min_gap=4)
            st24 = [0] * 24
            st24[22] = len(links)
            exp_sc = sc.expected_scaffolds(res, links, st24, o)
            assert exp_sc["status"][0] == 1 and exp_sc["status"][10] == nu - 1
            res_n = {"seq_offs": tj._padded(so, mu + 1, np.uint64).tolist()}
            scaf = {k: exp_sc[k] for k in ("sc_offs", "sc_lay_offs", "sc_flags", "layout", "seqs")}
            exp = ja.expected_join_approx(c["reads"], res_n, scaf, c["opts"], n_unitigs=nu, n_scaffolds=1)
            assert exp["status"][16] == nu - 1 and exp["seqs"] == c["genome"][c["span"][0]:c["span"][1]]
            d_nu, d_so = tj._up(np.array([nu], dtype=np.uint64)), tj._up(tj._padded(so, mu + 1, np.uint64))
            d_uf, d_us = tj._up(np.zeros(mu, dtype=np.uint32)), tj._up(res["useqs"])
            d_links, d_st24 = tj._up(ts._links_array(links)), tj._up(np.array(st24, dtype=np.uint64))
            st = tp._stream()
            torch.cuda.synchronize()
            try:
                s, _ = ts._enqueue(L, mu, len(links), d_nu.data_ptr(), d_so.data_ptr(), d_uf.data_ptr(), d_us.data_ptr(), len(res["useqs"]),
                                   d_links.data_ptr(), d_st24.data_ptr() + 22 * 8, d_st24.data_ptr(), o, exp_sc["status"][1], st)
                d, sizes = _enqueue(L, ix, mu, d_nu.data_ptr(), d_so.data_ptr(), s["status"].data_ptr(), s["sc_offs"].data_ptr(), s["sc_lay_offs"].data_ptr(),
                                    s["layout"].data_ptr(), s["seqs"].data_ptr(), exp_sc["status"][1], c["opts"], exp["status"][11], st)
                torch.cuda.synchronize()
            finally:
                L.sigax_stream_destroy(0, st)
            _same(_collect(d, sizes, c["name"]), exp, c["name"] + ", chained")
    finally:
        ix.close()


def test_capacity():
    """one byte short: status[14] = 1 and neither a base nor a patch is written (_collect: the whole buffer is as it was)"""
    c = next(x for x in ja.planted(31) if x["kind"] == "sixteen_columns")
    ix = _tj()._open(c["reads"], False)
    try:
        total = ja.case_expected(c)["status"][11]
        assert _device(ix, c, "one byte short", capacity=total - 1)[0]["status"][14] == 1
        exp, _ = _device(ix, c, "exact", capacity=total)
        assert exp["status"][14] == 0 and exp["status"][18] == 16
        assert _device(ix, c, "room to spare", capacity=total + 100)[0]["status"][14] == 0
        assert _device(ix, c, "no bases asked for", capacity=None)[0]["status"][14] == 1
    finally:
        ix.close()


def test_refusals():
    from siga_amd import _lib
    L = _lib.lib()
    E = _lib.SIGAX_E_ARG
    c = ja.planted(15)[0]
    ix = _tj()._open(c["reads"], False)
    try:
        wb, wb0 = C.c_uint64(), C.c_uint64()
        assert L.sigax_join_approx_workspace(1 << 31, C.byref(wb)) == E and L.sigax_join_approx_workspace(10, None) == E
        assert L.sigax_join_approx_workspace(0, C.byref(wb)) == 0 and wb.value == 0
        mu = 8
        assert L.sigax_join_approx_workspace(mu, C.byref(wb)) == 0 and L.sigax_join_workspace(mu, C.byref(wb0)) == 0 and wb.value > wb0.value
        names = ("nu", "so", "ns", "sco", "slo", "lay", "sq", "scoo", "layo", "sqo", "joins", "mm", "st")
        b = [torch.zeros(4096, dtype=torch.uint8, device="cuda:0") for _ in names]
        p = [t.data_ptr() for t in b]
        work = torch.zeros(wb.value, dtype=torch.uint8, device="cuda:0")

        def opts(flags=0, mm=2, pm=50, reserved=0):
            return C.byref(_lib.JoinApproxOpts(flags, 16, 100, 10, 15, 3, mm, pm, reserved))

        def dev(o="usual", nbytes=wb.value, **over):
            a = dict(zip(names, p))
            a.update(over)
            return L.sigax_join_approx_device(ix.handle, a["nu"], mu, a["so"], a["ns"], a["sco"], a["slo"], a["lay"], a["sq"], 1024,
                                              opts() if o == "usual" else o, a["scoo"], a["layo"], a["sqo"], 64, a["joins"], a["mm"], a["st"],
                                              work.data_ptr(), nbytes, None)

        assert dev() == 0 and dev(o=opts(mm=0)) == 0 and dev(o=opts(mm=16, pm=1)) == 0 and dev(o=opts(pm=250)) == 0, _lib.last_error()
        assert dev(o=None) == E
        assert dev(o=opts(mm=17)) == E and "max_mismatches" in _lib.last_error()
        assert dev(o=opts(pm=0)) == E and "mismatch_permille" in _lib.last_error()
        assert dev(o=opts(pm=251)) == E and "mismatch_permille" in _lib.last_error()
        assert dev(o=opts(reserved=1)) == E and "reserved" in _lib.last_error()
        assert dev(o=opts(flags=1)) == E and "flags" in _lib.last_error()
        assert dev(mm=None) == E and "d_mm" in _lib.last_error()
        assert dev(mm=p[0] + 2050) == E and "d_mm" in _lib.last_error() and "aligned" in _lib.last_error()
        assert dev(st=None) == E and "d_status24" in _lib.last_error()
        assert dev(nbytes=wb0.value) == E and "sigax_join_approx_workspace" in _lib.last_error()
        torch.cuda.synchronize()
        assert b[names.index("st")].cpu().numpy()[:192].view(np.uint64).tolist() == [0] * 24
        import siga_amd
        with pytest.raises(siga_amd.SigaxError):
            _host_call(ix, c, dict(c["opts"], max_mismatches=17))
        with pytest.raises(siga_amd.SigaxError):
            _host_call(ix, c, dict(c["opts"], mismatch_permille=0))
    finally:
        ix.close()


# ---- the command line, once, over the read set of tests/test_gpu_join.py::test_cli ----
def test_cli(tmp_path):
    """`siga unitig --scaffold --join-overlaps --join-mismatches 2 --joins`: the FASTA with joined= and corrected= in its headers and
    the JN lines with their two further columns against the restatement; without --join-mismatches every byte as before, which is
    the exact restatement's text; refusals and the help text"""
    import siga_amd
    from siga_amd import host
    from tests import gapfill_cases as gc
    from tests import pair_cases as pp
    from tests import test_gpu_gapfill as tg
    tj = _tj()
    prefix = tj._e2e_files(tj.E2E_SEED)
    genome, names, reads = tj._e2e(tj.E2E_SEED)
    f = {k: str(tmp_path / k) for k in ("u.fa", "u.layout", "u.pairs.json", "j.fa", "j.layout", "j.joins", "a.fa", "a.layout", "a.joins", "z.fa", "z.joins")}
    base = [host.CLI_PATH, "unitig", "-m", str(tg.E2E_M), "-p", prefix, "-o", f["u.fa"], "--layout", f["u.layout"], "--pairs", f["u.pairs.json"],
            "--insert-size", str(tg.E2E_INSERT), "--min-scaffold-unitig", "100"]
    r = subprocess.run(base + ["--scaffold", f["j.fa"], "--scaffold-layout", f["j.layout"], "--join-overlaps", "--joins", f["j.joins"], prefix + ".fa"],
                       capture_output=True)
    assert r.returncode == 0 and b"nearly agree" not in r.stderr, r.stderr.decode()
    res = tj._unitig_tables(f["u.fa"], f["u.layout"], names)
    pairs = pp.expected_pairs(res, [len(s) for s in reads], siga_amd.mates_by_name(names), {})
    exp_sc = sc.expected_scaffolds(res, pairs["links"], pairs["status"], {"insert_size": tg.E2E_INSERT, "min_unitig_bases": 100})
    scaf = {k: exp_sc[k] for k in ("sc_offs", "sc_lay_offs", "sc_flags", "layout", "seqs")}
    old = jc.expected_join(tuple(reads), res, scaf)
    jfa, jlay, jjn = jc.render(old, res["seq_offs"])
    assert open(f["j.fa"]).read() == jfa and open(f["j.layout"]).read() == jlay and open(f["j.joins"]).read() == jjn  # byte for byte as before
    assert "corrected=" not in jfa
    # with --join-mismatches
    opts = {"max_mismatches": 2, "mismatch_permille": 100}
    r = subprocess.run(base + ["--scaffold", f["a.fa"], "--scaffold-layout", f["a.layout"], "--join-overlaps", "--join-mismatches", "2",
                               "--join-mismatch-permille", "100", "--joins", f["a.joins"], prefix + ".fa"], capture_output=True)
    assert r.returncode == 0 and b"nearly agree" in r.stderr, r.stderr.decode()
    exp = ja.expected_join_approx(tuple(reads), res, scaf, opts)
    print("join status", exp["status"], exp["joins"], exp["mm"])
    afa, ajn = ja.render(exp, res["seq_offs"])
    assert open(f["a.fa"]).read() == afa and open(f["a.joins"]).read() == ajn
    assert " joined=" in afa and " corrected=" in afa and all(len(l.split("\t")) == 12 for l in ajn.splitlines()) and exp["status"][0] >= 1
    # --join-mismatches 0 is the command without it
    r = subprocess.run(base + ["--scaffold", f["z.fa"], "--join-overlaps", "--join-mismatches", "0", "--joins", f["z.joins"], prefix + ".fa"], capture_output=True)
    assert r.returncode == 0 and open(f["z.fa"]).read() == jfa and open(f["z.joins"]).read() == jjn, r.stderr.decode()
    # refusals and the help text
    for opt in (["--join-mismatches", "2"], ["--join-mismatch-permille", "50"]):
        r = subprocess.run(base + ["--scaffold", f["z.fa"]] + opt + [prefix + ".fa"], capture_output=True)
        assert r.returncode == 1 and b"--join-overlaps" in r.stderr, opt
    for opt in (["--join-mismatches", "17"], ["--join-mismatch-permille", "0"], ["--join-mismatch-permille", "251"]):
        r = subprocess.run(base + ["--scaffold", f["z.fa"], "--join-overlaps"] + opt + [prefix + ".fa"], capture_output=True)
        assert r.returncode == 1, opt
    r = subprocess.run([host.CLI_PATH, "unitig"], capture_output=True)
    assert r.returncode == 0 and b"--join-mismatches" in r.stdout and b"--join-mismatch-permille" in r.stdout and b"needs --join-overlaps" in r.stdout
