"""Tip trimming and the lifted records of `siga unitig` on the GPU (csrc/sigax_unitig.hip) against the serial restatement of
their rules (tests/trim_cases.py): every case through the host and the device entry point, exactly -- offsets, flags, layout,
bytes, removed, lifted records, all 12 counts; no rounds = siga_amd.unitigs; canaries and refusals; and end to end over the
records of a GPU overlap run on reads with errors, through the wrapper and the command line."""
import ctypes as C
import functools
import gzip
import os
import subprocess

import numpy as np
import pytest
import torch  # before the library loads: one HIP runtime per process

from oracle import pyoracle as po
from tests import trim_cases as tc
from tests import unitig_cases as uc
from tests.fixtures import CACHE
from tests.golden import make_reads as mr

pytestmark = pytest.mark.gpu
CASES = tc.hand_built()
IDS = [c["name"] for c in CASES]
UC_CASES = uc.hand_built()


def _same(res, exp, what, bases=True, graph=True):
    """res: the wrapper's dict (numpy arrays); exp: expected_trim()'s"""
    status = res["status"].tolist()
    if not graph:
        assert status[11] == 0 and res["uedges"] is None, what
        status[11] = exp["status"][11]
    print(what, "status", status, "expected", exp["status"])
    assert status == exp["status"], what
    assert res["seq_offs"].tolist() == exp["seq_offs"] and res["lay_offs"].tolist() == exp["lay_offs"], what
    assert res["uflags"].tolist() == exp["uflags"], what
    assert [tuple(int(x) for x in p) for p in res["layout"].tolist()] == exp["layout"], what
    assert res["removed"].tolist() == exp["removed"], what
    if graph:
        assert [tuple(int(x) for x in e) for e in res["uedges"].tolist()] == exp["uedges"], what
    if bases:
        assert res["useqs"].tobytes() == exp["useqs"], what
    else:
        assert res["useqs"] is None, what


def _host(case, max_rounds=None, **kw):
    import siga_amd
    edges, lengths, seqs, offs = uc.arrays(case)
    return siga_amd.unitigs_trim(edges, lengths, seqs, offs, case["m"], case["x"] if max_rounds is None else max_rounds, case["L"], case["C"], **kw)


@pytest.mark.parametrize("case", UC_CASES, ids=[c["name"] for c in UC_CASES])
def test_no_rounds_is_unitigs(case):
    import siga_amd
    edges, lengths, seqs, offs = uc.arrays(case)
    res = siga_amd.unitigs_trim(edges, lengths, seqs, offs, case["m"], 0, 150)
    want = siga_amd.unitigs(edges, lengths, seqs, offs, case["m"])
    for k in ("seq_offs", "lay_offs", "uflags", "layout", "useqs"):
        assert res[k].tobytes() == want[k].tobytes(), k
    assert res["status"][:6].tolist() == want["status"].tolist() and res["status"][6:11].tolist() == [0] * 5
    assert not res["removed"].any() and len(res["removed"]) == len(lengths)
    exp = tc.expected_trim(case["reads"], case["edges"], case["m"], 0, 150)
    assert [tuple(int(x) for x in e) for e in res["uedges"].tolist()] == exp["uedges"] and int(res["status"][11]) == len(exp["uedges"])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_host_form_equals_brute_force(case):
    _same(_host(case), tc.expected_of(case["name"]), case["name"])


def test_host_form_takes_a_window_of_a_longer_table():
    import siga_amd
    case = tc.case_named("graph")
    edges, lengths, seqs, offs = uc.arrays(case)
    res = siga_amd.unitigs_trim(edges, lengths, b"#" * 7 + seqs, offs + np.uint64(7), case["m"], case["x"], case["L"])
    _same(res, tc.expected_of("graph"), "offs[0] = 7")


CANARY = 64


def _device_call(case, max_rounds=None, layout_only=False, graph=True):
    """sigax_unitigs_trim_device over torch buffers, each output buffer of exactly its size plus CANARY bytes of 0xEE -> (dict
    like the wrapper's, what lies beyond the bytes the call had to write)"""
    from siga_amd import _lib
    L = _lib.lib()
    edges, lengths, seqs, offs = uc.arrays(case)
    n, ne, nb = len(lengths), len(edges), len(seqs)
    dev = torch.device("cuda:0")

    def up(a):
        a = np.frombuffer(a, dtype=np.uint8) if isinstance(a, bytes) else a.view(np.uint8).reshape(-1)
        return torch.from_numpy(a.copy()).to(dev) if a.size else torch.zeros(16, dtype=torch.uint8, device=dev)

    def out(nbytes):
        return torch.full((nbytes + CANARY,), 0xEE, dtype=torch.uint8, device=dev)

    wb = C.c_uint64()
    assert L.sigax_unitigs_trim_workspace(n, ne, int(graph), C.byref(wb)) == 0
    d_edges, d_len, d_seqs, d_offs = up(edges), up(lengths), up(seqs), up(offs)
    sizes = {"seq_offs": 8 * (n + 1), "lay_offs": 8 * (n + 1), "uflags": 4 * n, "layout": 16 * n, "useqs": nb, "removed": 4 * n,
             "uedges": 16 * ne, "status": 96, "work": wb.value}
    d = {k: out(v) for k, v in sizes.items()}
    opts = _lib.TrimOpts(case["x"] if max_rounds is None else max_rounds, case["L"],
                         _lib.SIGAX_TRIM_NO_COVERAGE if case["C"] is None else case["C"], 0)
    torch.cuda.synchronize()
    rc = L.sigax_unitigs_trim_device(0, d_edges.data_ptr(), ne, d_len.data_ptr(), d_seqs.data_ptr(), d_offs.data_ptr(), n, case["m"],
                                     C.byref(opts), d["seq_offs"].data_ptr(), d["lay_offs"].data_ptr(), d["uflags"].data_ptr(),
                                     d["layout"].data_ptr(), None if layout_only else d["useqs"].data_ptr(), d["removed"].data_ptr(),
                                     d["uedges"].data_ptr() if graph else None, d["status"].data_ptr(), d["work"].data_ptr(), wb.value, None)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    h = {k: v.cpu().numpy() for k, v in d.items()}
    status = h["status"][:96].view(np.uint64)
    u, placed, lifted = int(status[0]), n - int(status[9]), int(status[11])
    assert u <= n and lifted <= ne and int(status[1]) <= nb
    res = {"status": status, "seq_offs": h["seq_offs"][:8 * (u + 1)].view(np.uint64), "lay_offs": h["lay_offs"][:8 * (u + 1)].view(np.uint64),
           "uflags": h["uflags"][:4 * u].view(np.uint32), "layout": h["layout"][:16 * placed].view(_lib.PLACEMENT_DTYPE),
           "useqs": None if layout_only else h["useqs"][:int(status[1])], "removed": h["removed"][:4 * n].view(np.uint32),
           "uedges": h["uedges"][:16 * lifted].view(_lib.EDGE_DTYPE) if graph else None}
    tails = {k: h[k][sizes[k]:].tobytes() for k in sizes}
    # what lies beyond the entries the call wrote, inside the buffers, is the caller's too
    tails["seq_offs_rest"] = h["seq_offs"][8 * (u + 1):sizes["seq_offs"]].tobytes()
    tails["lay_offs_rest"] = h["lay_offs"][8 * (u + 1):sizes["lay_offs"]].tobytes()
    tails["uflags_rest"] = h["uflags"][4 * u:sizes["uflags"]].tobytes()
    tails["layout_rest"] = h["layout"][16 * placed:sizes["layout"]].tobytes()
    tails["useqs_rest"] = h["useqs"][0 if layout_only else int(status[1]):nb].tobytes()
    tails["uedges_rest"] = h["uedges"][16 * lifted if graph else 0:sizes["uedges"]].tobytes()
    return res, tails


def _untouched(tails, what):
    for k, t in tails.items():
        assert t == b"\xee" * len(t), "%s: bytes after %s were written" % (what, k)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_device_form_equals_brute_force(case):
    res, tails = _device_call(case)
    _same(res, tc.expected_of(case["name"]), case["name"])
    _untouched(tails, case["name"])


@pytest.mark.parametrize("rounds", [1, 2, 3, 10])
def test_cascade_round_by_round(rounds):
    case = tc.case_named("cascade")
    exp = tc.expected_of("cascade", rounds)
    assert exp["status"][6] == min(rounds, 3)
    _same(_host(case, rounds), exp, "cascade, host, %d rounds" % rounds)
    res, tails = _device_call(case, rounds)
    _same(res, exp, "cascade, device, %d rounds" % rounds)
    _untouched(tails, "cascade")


@pytest.mark.parametrize("name", ["graph", "ring_tip", "all_removed"])
def test_graph_off_and_layout_only(name):
    case, exp = tc.case_named(name), tc.expected_of(name)
    _same(_host(case, graph=False), exp, name + ", host, no graph", graph=False)
    _same(_host(case, bases=False), exp, name + ", host, layout only", bases=False)
    res, tails = _device_call(case, graph=False)
    _same(res, exp, name + ", device, no graph", graph=False)
    _untouched(tails, name)
    res, tails = _device_call(case, layout_only=True)
    _same(res, exp, name + ", device, layout only", bases=False)
    _untouched(tails, name)


def test_refusals():
    from siga_amd import _lib
    L = _lib.lib()
    E = _lib.SIGAX_E_ARG
    wb = C.c_uint64()
    assert L.sigax_unitigs_trim_workspace(1 << 31, 0, 1, C.byref(wb)) == E
    assert L.sigax_unitigs_trim_workspace(10, (1 << 32) + 1, 1, C.byref(wb)) == E
    assert L.sigax_unitigs_trim_workspace(10, 1 << 32, 1, None) == E
    assert L.sigax_unitigs_trim_workspace(10, 1 << 32, 1, C.byref(wb)) == 0 and wb.value > 12 * (1 << 32)
    with_graph = wb.value
    assert L.sigax_unitigs_trim_workspace(10, 1 << 32, 0, C.byref(wb)) == 0 and 0 < wb.value < with_graph
    z = None
    ok = _lib.TrimOpts(10, 150, _lib.SIGAX_TRIM_NO_COVERAGE, 0)
    dev = lambda n, ne, o, *b: L.sigax_unitigs_trim_device(0, b[0], ne, b[1], b[2], b[3], n, 20, o, *b[4:])  # noqa: E731
    nothing = [z] * 13 + [0, z]
    assert dev(0, 0, C.byref(ok), *nothing) == 0  # n_reads == 0
    assert dev(1 << 31, 0, C.byref(ok), *nothing) == E
    assert dev(0, (1 << 32) + 1, C.byref(ok), *nothing) == E
    assert dev(4, 0, C.byref(ok), *nothing) == E  # NULL buffers
    assert dev(0, 0, None, *nothing) == E  # no options
    assert dev(0, 0, C.byref(_lib.TrimOpts(10, 150, 0, 1)), *nothing) == E and "reserved" in _lib.last_error()
    assert dev(0, 0, C.byref(_lib.TrimOpts(65, 150, 0, 0)), *nothing) == E and "max_rounds" in _lib.last_error()
    assert dev(0, 0, C.byref(_lib.TrimOpts(64, 150, 0, 0)), *nothing) == 0
    n = 4
    assert L.sigax_unitigs_trim_workspace(n, 0, 1, C.byref(wb)) == 0
    b = [torch.zeros(4096, dtype=torch.uint8, device="cuda:0") for _ in range(12)]
    p = [t.data_ptr() for t in b]
    work = torch.zeros(wb.value, dtype=torch.uint8, device="cuda:0")

    def args(w, nbytes, **over):
        a = {"edges": z, "len": p[0], "seqs": p[1], "offs": p[2], "so": p[3], "lo": p[4], "uf": p[5], "lay": p[6], "us": p[7], "rm": p[8],
             "ue": p[9], "st": p[10]}
        a.update(over)
        return (n, 0, C.byref(ok), a["edges"], a["len"], a["seqs"], a["offs"], a["so"], a["lo"], a["uf"], a["lay"], a["us"], a["rm"], a["ue"],
                a["st"], w, nbytes, z)

    assert dev(*args(work.data_ptr(), wb.value - 1)) == E and "workspace" in _lib.last_error()
    assert dev(*args(z, wb.value)) == E
    assert dev(*args(work.data_ptr(), wb.value, rm=z)) == E
    assert dev(*args(work.data_ptr(), wb.value, st=z)) == E
    assert dev(*args(work.data_ptr(), wb.value, ue=p[9] + 8)) == E and "aligned" in _lib.last_error()
    assert dev(*args(work.data_ptr(), wb.value, lay=p[6] + 4)) == E
    assert dev(*args(work.data_ptr(), wb.value, st=p[10] + 4)) == E
    assert dev(*args(work.data_ptr(), wb.value, rm=p[8] + 2)) == E
    assert dev(*args(work.data_ptr(), wb.value)) == 0, _lib.last_error()  # (lengths and offsets all zero)
    assert dev(*args(work.data_ptr(), wb.value, ue=z, us=z)) == 0, _lib.last_error()
    torch.cuda.synchronize()
    nu = C.c_uint64()
    v = [C.c_void_p() for _ in range(7)]
    st = (C.c_uint64 * 12)()
    host = lambda nr, o, pn, ps: L.sigax_unitigs_trim_host(0, z, 0, z, z, z, nr, 20, o, pn, *[C.byref(x) for x in v], ps)  # noqa: E731
    assert host(0, C.byref(ok), C.byref(nu), st) == 0 and nu.value == 0 and list(st) == [0] * 12
    for x in v:
        L.sigax_free(x)
    assert host(0, C.byref(ok), None, st) == E
    assert host(0, C.byref(ok), C.byref(nu), None) == E
    assert host(0, None, C.byref(nu), st) == E
    assert host(0, C.byref(_lib.TrimOpts(65, 150, 0, 0)), C.byref(nu), st) == E
    assert host(0, C.byref(_lib.TrimOpts(1, 150, 0, 7)), C.byref(nu), st) == E
    assert host(3, C.byref(ok), C.byref(nu), st) == E


# ---- end to end: the edge records of a GPU overlap run over reads with errors ----
def _e2e_files():
    d = os.path.join(CACHE, "unitig_trim_e2e")
    os.makedirs(d, exist_ok=True)
    prefix = os.path.join(d, "reads")
    case = tc.end_to_end()
    if not all(os.path.exists(prefix + e) for e in (".bwt", ".rbwt", ".sai", ".rsai", ".fa")):
        seqs = [s.decode() for _, s in case["reads"]]
        po.Index.build(seqs).save(prefix + ".bwt", prefix + ".sai")
        po.Index.build(seqs, reverse=True).save(prefix + ".rbwt", prefix + ".rsai")
        with open(prefix + ".fa", "w") as f:
            f.write(mr.fasta_text([(n, s.decode()) for n, s in case["reads"]]))
    return prefix


@functools.lru_cache(maxsize=None)
def _e2e_run():
    """-> (edges of the GPU overlap run, the wrapper's result on them, expected_trim() on them, expected_trim() without rounds)"""
    import siga_amd
    case = tc.end_to_end()
    prefix = _e2e_files()
    names = [n for n, _ in case["reads"]]
    reads = [s for _, s in case["reads"]]
    pair = siga_amd.FMIndexPair.load(prefix, device=0, with_sai=True, resident=False)
    try:
        lengths = np.array([len(s) for s in reads], dtype=np.uint32)
        pair.set_reads(lengths, siga_amd.overlap.name_ranks(names))
        edges = siga_amd.OverlapBuilder(pair, prefix).overlap(reads, case["m"], edges=True)["edges"]
    finally:
        pair.close()
    offs = np.zeros(len(reads) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(lengths, dtype=np.uint64)
    res = siga_amd.unitigs_trim(edges, lengths, b"".join(reads), offs, case["m"], case["x"], case["L"])
    recs = [tuple(int(x) for x in e) for e in edges.tolist()]
    return edges, res, tc.expected_trim(reads, recs, case["m"], case["x"], case["L"]), tc.expected_trim(reads, recs, case["m"], 0, case["L"])


def test_end_to_end():
    edges, res, exp, untrimmed = _e2e_run()
    assert len(edges) > 300
    _same(res, exp, "end to end")
    print("unitigs without trimming", untrimmed["status"][0], "with", exp["status"][0], "rounds", exp["status"][6], "reads removed", exp["status"][9])
    assert exp["status"][6] >= 2, "built so that at least two rounds remove something"
    assert exp["status"][0] < untrimmed["status"][0]
    assert exp["status"][2] == 0 and exp["status"][3] == 0 and exp["status"][9] > 0 and exp["status"][11] > 0


def _want_texts(names, res, m):
    from siga_amd.overlap import format_asqg
    plain = {"uflags": res["uflags"], "lay_offs": res["lay_offs"], "seq_offs": res["seq_offs"], "useqs": res["useqs"].tobytes(),
             "layout": res["layout"].tolist()}
    fa, lay = uc.render(names, plain)
    verts = tc.render_graph(plain)
    graph = format_asqg([(v[0], v[1], v[2].decode()) for v in verts], {"substring": [0] * len(verts), "edges": res["uedges"]}, m)
    return fa, lay, graph, tc.render_removed(names, res["removed"])


def test_cli(tmp_path):
    from siga_amd import host
    case = tc.end_to_end()
    prefix = _e2e_files()
    _, res, _, _ = _e2e_run()
    names = [n for n, _ in case["reads"]]
    want_fa, want_lay, want_graph, want_removed = _want_texts(names, res, case["m"])
    assert "\nED\tunitig-" in want_graph and "\tCR:i:" in want_graph and want_removed.count("\n") == int(res["status"][9])
    fa, lay, gr, gz, rm = (str(tmp_path / f) for f in ("u.fa", "u.layout", "u.asqg", "u.asqg.gz", "u.removed"))
    base = [host.CLI_PATH, "unitig", "-m", str(case["m"]), "-p", prefix]
    trim = ["-x", str(case["x"]), "-n", str(case["L"])]
    r = subprocess.run(base + trim + ["-o", fa, "--layout", lay, "--graph", gr, "--removed", rm, prefix + ".fa"], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    assert open(fa).read() == want_fa and open(lay).read() == want_lay and open(gr).read() == want_graph and open(rm).read() == want_removed
    r = subprocess.run(base + ["--cut-terminal=%d" % case["x"], "--min-branch-length=%d" % case["L"], "-o", fa, "--graph=" + gz, prefix + ".fa"],
                       capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    assert open(fa).read() == want_fa and gzip.open(gz, "rb").read().decode() == want_graph
    # -x 0 is the run without the option, byte for byte
    plain, zero = str(tmp_path / "p.fa"), str(tmp_path / "z.fa")
    play, zlay = str(tmp_path / "p.layout"), str(tmp_path / "z.layout")
    assert subprocess.run(base + ["-o", plain, "--layout", play, prefix + ".fa"], capture_output=True).returncode == 0
    assert subprocess.run(base + ["-x", "0", "-o", zero, "--layout", zlay, prefix + ".fa"], capture_output=True).returncode == 0
    assert open(plain, "rb").read() == open(zero, "rb").read() and open(play, "rb").read() == open(zlay, "rb").read()
    assert open(plain).read() != want_fa
    # the host class through its C entry point, in overlap calls of 97 reads
    host.unitig_file(prefix + ".fa", prefix, case["m"], out=fa, layout=lay, piece_reads=97, cut_terminal=case["x"], min_branch_length=case["L"],
                     graph=gr, removed=rm)
    assert open(fa).read() == want_fa and open(lay).read() == want_lay and open(gr).read() == want_graph and open(rm).read() == want_removed
    for bad in (["-x", prefix + ".fa"], ["-x", "65", prefix + ".fa"], ["-n", "12x", prefix + ".fa"], ["-C", "-1", prefix + ".fa"]):
        r = subprocess.run(base + ["-o", fa] + bad, capture_output=True)  # (-x was --exhaustive's short form once: no file name as N)
        assert r.returncode != 0 and b"needs a number" in r.stderr, bad
    r = subprocess.run(base, capture_output=True)  # no READSFILE: the help text
    assert r.returncode == 0 and all(w in r.stdout for w in (b"--cut-terminal", b"--min-branch-length", b"--min-branch-coverage", b"--graph", b"--removed"))
