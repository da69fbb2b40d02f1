"""Non-maximal overlap cutting in the rounds of `siga unitig` on the GPU (csrc/sigax_unitig.hip) against the serial restatement of
its rules (tests/prune_cases.py): every case through the host and the device entry point, exactly -- offsets, flags, layout,
bytes, removed, cut, lifted records, all 16 counts; delta = 0 = siga_amd.unitigs_trim; no rounds = siga_amd.unitigs; canaries and
refusals; and end to end over the records of a GPU overlap run on reads with substitutions, through the wrapper and the command
line."""
import ctypes as C
import functools
import os
import random
import subprocess

import numpy as np
import pytest
import torch  # before the library loads: one HIP runtime per process

from oracle import pyoracle as po
from tests import prune_cases as pc
from tests import trim_cases as tc
from tests import unitig_cases as uc
from tests.fixtures import CACHE
from tests.golden import make_reads as mr

pytestmark = pytest.mark.gpu
CASES = pc.hand_built()
IDS = [c["name"] for c in CASES]
TC_CASES = tc.hand_built()
UC_CASES = uc.hand_built()


def _same(res, exp, what, bases=True, graph=True):
    """res: the wrapper's dict (numpy arrays); exp: expected_prune()'s"""
    status = res["status"].tolist()
    if not graph:
        assert status[11] == 0 and res["uedges"] is None, what
        status[11] = exp["status"][11]
    print(what, "status", status, "expected", exp["status"])
    assert status == exp["status"], what
    assert res["cut"].tolist() == exp["cut"], what
    assert res["removed"].tolist() == exp["removed"], what
    assert res["seq_offs"].tolist() == exp["seq_offs"] and res["lay_offs"].tolist() == exp["lay_offs"], what
    assert res["uflags"].tolist() == exp["uflags"], what
    assert [tuple(int(x) for x in p) for p in res["layout"].tolist()] == exp["layout"], what
    if graph:
        assert [tuple(int(x) for x in e) for e in res["uedges"].tolist()] == exp["uedges"], what
    if bases:
        assert res["useqs"].tobytes() == exp["useqs"], what
    else:
        assert res["useqs"] is None, what


def _host(case, max_rounds=None, **kw):
    import siga_amd
    edges, lengths, seqs, offs = uc.arrays(case)
    return siga_amd.unitigs_prune(edges, lengths, seqs, offs, case["m"], case["x"] if max_rounds is None else max_rounds, case["L"], case["C"],
                                  delta=case["delta"], careful=case["careful"], num_reads=case["N"], genome_size=case["G"],
                                  uniq_threshold=case["T"], **kw)


CANARY = 64


def _device_call(case, max_rounds=None, layout_only=False, graph=True):
    """sigax_unitigs_prune_device over torch buffers, each output buffer of exactly its size plus CANARY bytes of 0xEE -> (dict
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
    assert L.sigax_unitigs_prune_workspace(n, ne, int(graph), int(case["careful"]), C.byref(wb)) == 0
    d_edges, d_len, d_seqs, d_offs = up(edges), up(lengths), up(seqs), up(offs)
    sizes = {"seq_offs": 8 * (n + 1), "lay_offs": 8 * (n + 1), "uflags": 4 * n, "layout": 16 * n, "useqs": nb, "removed": 4 * n, "cut": 4 * ne,
             "uedges": 16 * ne, "status": 128, "work": wb.value}
    d = {k: out(v) for k, v in sizes.items()}
    opts = _lib.PruneOpts(case["x"] if max_rounds is None else max_rounds, case["L"],
                          _lib.SIGAX_TRIM_NO_COVERAGE if case["C"] is None else case["C"], case["delta"], int(case["careful"]), 0, case["N"],
                          case["G"], case["T"])
    torch.cuda.synchronize()
    rc = L.sigax_unitigs_prune_device(0, d_edges.data_ptr(), ne, d_len.data_ptr(), d_seqs.data_ptr(), d_offs.data_ptr(), n, case["m"],
                                      C.byref(opts), d["seq_offs"].data_ptr(), d["lay_offs"].data_ptr(), d["uflags"].data_ptr(),
                                      d["layout"].data_ptr(), None if layout_only else d["useqs"].data_ptr(), d["removed"].data_ptr(),
                                      d["cut"].data_ptr(), d["uedges"].data_ptr() if graph else None, d["status"].data_ptr(),
                                      d["work"].data_ptr(), wb.value, None)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    h = {k: v.cpu().numpy() for k, v in d.items()}
    status = h["status"][:128].view(np.uint64)
    u, placed, lifted = int(status[0]), n - int(status[9]), int(status[11])
    assert u <= n and lifted <= ne and int(status[1]) <= nb
    res = {"status": status, "seq_offs": h["seq_offs"][:8 * (u + 1)].view(np.uint64), "lay_offs": h["lay_offs"][:8 * (u + 1)].view(np.uint64),
           "uflags": h["uflags"][:4 * u].view(np.uint32), "layout": h["layout"][:16 * placed].view(_lib.PLACEMENT_DTYPE),
           "useqs": None if layout_only else h["useqs"][:int(status[1])], "removed": h["removed"][:4 * n].view(np.uint32),
           "cut": h["cut"][:4 * ne].view(np.uint32), "uedges": h["uedges"][:16 * lifted].view(_lib.EDGE_DTYPE) if graph else None}
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
def test_host_form_equals_brute_force(case):
    _same(_host(case), pc.expected_of(case["name"]), case["name"])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_device_form_equals_brute_force(case):
    res, tails = _device_call(case)
    _same(res, pc.expected_of(case["name"]), case["name"])
    _untouched(tails, case["name"])


@pytest.mark.parametrize("rounds", [1, 2, 3])
def test_cascade_round_by_round(rounds):
    case = pc.case_named("cascade")
    exp = pc.expected_of("cascade", rounds)
    assert exp["status"][6] == min(rounds, 2) and exp["status"][12] == (rounds >= 2)
    _same(_host(case, rounds), exp, "cascade, host, %d rounds" % rounds)
    res, tails = _device_call(case, rounds)
    _same(res, exp, "cascade, device, %d rounds" % rounds)
    _untouched(tails, "cascade")


def test_random_graphs():
    for seed in range(20):
        case = pc.random_case(seed)
        exp = pc.run(pc.expected_prune, case)
        _same(_host(case), exp, case["name"] + ", host")
        res, tails = _device_call(case)
        _same(res, exp, case["name"] + ", device")
        _untouched(tails, case["name"])


def test_large_graph():
    case = pc.large_case()
    exp = pc.run(pc.expected_prune, case)
    assert exp["status"][12] > 100 and exp["status"][13] >= 2 and exp["status"][9] > 100, exp["status"]
    res, tails = _device_call(case)
    _same(res, exp, "large, device")
    _untouched(tails, "large")
    careful = dict(case, careful=True)
    res, tails = _device_call(careful)
    _same(res, pc.run(pc.expected_prune, careful), "large, device, careful")
    _untouched(tails, "large, careful")


@pytest.mark.parametrize("case", TC_CASES, ids=[c["name"] for c in TC_CASES])
def test_delta_0_is_unitigs_trim(case):
    import siga_amd
    edges, lengths, seqs, offs = uc.arrays(case)
    want = siga_amd.unitigs_trim(edges, lengths, seqs, offs, case["m"], case["x"], case["L"], case["C"])
    for careful in (False, True):
        res = siga_amd.unitigs_prune(edges, lengths, seqs, offs, case["m"], case["x"], case["L"], case["C"], delta=0, careful=careful,
                                     genome_size=5000)
        for k in ("seq_offs", "lay_offs", "uflags", "layout", "useqs", "removed", "uedges"):
            assert res[k].tobytes() == want[k].tobytes(), k
        assert res["status"][:12].tolist() == want["status"].tolist() and res["status"][12:].tolist() == [0] * 4
        assert not res["cut"].any() and len(res["cut"]) == len(edges)
    d = dict(case, delta=0, careful=False, N=len(lengths), G=0, T=13.0)
    res, tails = _device_call(d)
    for k in ("seq_offs", "lay_offs", "uflags", "layout", "useqs", "removed", "uedges"):
        assert res[k].tobytes() == want[k].tobytes(), k
    assert res["status"][:12].tolist() == want["status"].tolist() and res["status"][12:].tolist() == [0] * 4 and not res["cut"].any()
    _untouched(tails, case["name"])


@pytest.mark.parametrize("case", UC_CASES, ids=[c["name"] for c in UC_CASES])
def test_no_rounds_is_unitigs(case):
    import siga_amd
    edges, lengths, seqs, offs = uc.arrays(case)
    res = siga_amd.unitigs_prune(edges, lengths, seqs, offs, case["m"], 0, 150, delta=10, careful=True, genome_size=100000)
    want = siga_amd.unitigs(edges, lengths, seqs, offs, case["m"])
    for k in ("seq_offs", "lay_offs", "uflags", "layout", "useqs"):
        assert res[k].tobytes() == want[k].tobytes(), k
    assert res["status"][:6].tolist() == want["status"].tolist() and res["status"][6:11].tolist() == [0] * 5
    assert res["status"][12:].tolist() == [0] * 4
    assert not res["removed"].any() and not res["cut"].any() and len(res["cut"]) == len(edges)
    exp = tc.expected_trim(case["reads"], case["edges"], case["m"], 0, 150)
    assert [tuple(int(x) for x in e) for e in res["uedges"].tolist()] == exp["uedges"] and int(res["status"][11]) == len(exp["uedges"])


@pytest.mark.parametrize("name", ["fork", "parallel_careful", "cascade", "self_tip"])
def test_graph_off_and_layout_only(name):
    case, exp = pc.case_named(name), pc.expected_of(name)
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
    assert L.sigax_unitigs_prune_workspace(1 << 31, 0, 1, 0, C.byref(wb)) == E
    assert L.sigax_unitigs_prune_workspace(10, (1 << 32) + 1, 1, 0, C.byref(wb)) == E
    assert L.sigax_unitigs_prune_workspace(10, 100, 1, 0, None) == E
    assert L.sigax_unitigs_prune_workspace(10, 100, 1, 0, C.byref(wb)) == 0
    plain = wb.value
    assert L.sigax_unitigs_prune_workspace(10, 100, 1, 1, C.byref(wb)) == 0 and wb.value >= plain + 8 * 400  # the table only with careful
    assert L.sigax_unitigs_trim_workspace(10, 100, 1, C.byref(wb)) == 0 and wb.value < plain
    z = None

    def opts(**over):
        o = dict(max_rounds=10, min_branch_length=150, min_branch_coverage=_lib.SIGAX_TRIM_NO_COVERAGE, delta=10, careful=0, reserved=0,
                 num_reads=4, genome_size=5000, uniq_threshold=13.0)
        o.update(over)
        return C.byref(_lib.PruneOpts(*[o[k] for k, _ in _lib.PruneOpts._fields_]))

    dev = lambda n, ne, o, *b: L.sigax_unitigs_prune_device(0, b[0], ne, b[1], b[2], b[3], n, 20, o, *b[4:])  # noqa: E731
    nothing = [z] * 14 + [0, z]
    assert dev(0, 0, opts(), *nothing) == 0  # n_reads == 0
    assert dev(0, 0, None, *nothing) == E
    assert dev(0, 0, opts(careful=2), *nothing) == E and "careful" in _lib.last_error()
    assert dev(0, 0, opts(reserved=1), *nothing) == E and "reserved" in _lib.last_error()
    assert dev(0, 0, opts(genome_size=0), *nothing) == E and "genome_size" in _lib.last_error()
    assert dev(0, 0, opts(genome_size=0, delta=0), *nothing) == 0
    assert dev(0, 0, opts(max_rounds=65), *nothing) == E and "max_rounds" in _lib.last_error()
    assert dev(4, 0, opts(num_reads=3), *nothing) == E and "num_reads" in _lib.last_error()
    assert dev(4, 0, opts(), *nothing) == E  # NULL buffers
    assert dev(1 << 31, 0, opts(num_reads=1 << 31), *nothing) == E
    n, ne = 4, 2
    assert L.sigax_unitigs_prune_workspace(n, ne, 1, 1, C.byref(wb)) == 0
    b = [torch.zeros(4096, dtype=torch.uint8, device="cuda:0") for _ in range(14)]
    p = [t.data_ptr() for t in b]
    work = torch.zeros(wb.value, dtype=torch.uint8, device="cuda:0")

    def args(w, nbytes, o=None, **over):
        a = {"edges": p[11], "len": p[0], "seqs": p[1], "offs": p[2], "so": p[3], "lo": p[4], "uf": p[5], "lay": p[6], "us": p[7], "rm": p[8],
             "ct": p[12], "ue": p[9], "st": p[10]}
        a.update(over)
        return (n, ne, o or opts(careful=1), a["edges"], a["len"], a["seqs"], a["offs"], a["so"], a["lo"], a["uf"], a["lay"], a["us"], a["rm"],
                a["ct"], a["ue"], a["st"], w, nbytes, z)

    assert dev(*args(work.data_ptr(), wb.value - 1)) == E and "workspace" in _lib.last_error()
    assert dev(*args(z, wb.value)) == E
    assert dev(*args(work.data_ptr(), wb.value, ct=z)) == E
    assert dev(*args(work.data_ptr(), wb.value, ct=p[12] + 2)) == E and "d_cut" in _lib.last_error()
    assert dev(*args(work.data_ptr(), wb.value, ct=p[12] + 2, o=opts(delta=0))) == E and "d_cut" in _lib.last_error()
    assert dev(*args(work.data_ptr(), wb.value, rm=z)) == E
    assert dev(*args(work.data_ptr(), wb.value, st=z)) == E
    assert dev(*args(work.data_ptr(), wb.value, st=p[10] + 4)) == E
    assert dev(*args(work.data_ptr(), wb.value, ue=p[9] + 8)) == E and "aligned" in _lib.last_error()
    assert dev(*args(work.data_ptr(), wb.value)) == 0, _lib.last_error()  # (lengths, offsets and records all zero: every record malformed)
    assert dev(*args(work.data_ptr(), wb.value, ue=z, us=z)) == 0, _lib.last_error()
    torch.cuda.synchronize()
    nu = C.c_uint64()
    v = [C.c_void_p() for _ in range(8)]
    st = (C.c_uint64 * 16)()
    host = lambda nr, o, pn, ps: L.sigax_unitigs_prune_host(0, z, 0, z, z, z, nr, 20, o, pn, *[C.byref(x) for x in v], ps)  # noqa: E731
    assert host(0, opts(), C.byref(nu), st) == 0 and nu.value == 0 and list(st) == [0] * 16
    for x in v:
        L.sigax_free(x)
    assert host(0, opts(), None, st) == E
    assert host(0, opts(), C.byref(nu), None) == E
    assert host(0, None, C.byref(nu), st) == E
    assert host(0, opts(careful=2), C.byref(nu), st) == E
    assert host(0, opts(reserved=7), C.byref(nu), st) == E
    assert host(0, opts(genome_size=0), C.byref(nu), st) == E
    assert host(3, opts(num_reads=2), C.byref(nu), st) == E
    assert host(3, opts(), C.byref(nu), st) == E  # NULL buffers


def test_no_reads():
    import siga_amd
    none = np.zeros(0, dtype=np.uint32)
    res = siga_amd.unitigs_prune(np.zeros(0, dtype=uc.EDGE_DTYPE), none, b"", np.zeros(1, dtype=np.uint64), 20, 10, 150, delta=10, genome_size=5000)
    assert res["status"].tolist() == [0] * 16 and len(res["cut"]) == 0 and len(res["removed"]) == 0 and len(res["layout"]) == 0


# ---- end to end: the edge records of a GPU overlap run over reads with substitutions ----
E2E_READS, E2E_GENOME, E2E_LEN, E2E_M, E2E_SEED = 2400, 12000, 60, 25, 11
E2E_X, E2E_L, E2E_DELTA, E2E_G, E2E_T = 10, 60, 10, 12000, 13.0


@functools.lru_cache(maxsize=None)
def _e2e_case():
    """2 400 reads of 60 from a 12 000-base random genome, both strands, one read in four with one substitution"""
    rng = random.Random(E2E_SEED)
    g = bytes(rng.choice(b"ACGT") for _ in range(E2E_GENOME))
    reads = []
    for i in range(E2E_READS):
        at = rng.randrange(E2E_GENOME - E2E_LEN + 1)
        w = bytearray(g[at:at + E2E_LEN])
        if i % 4 == 0:
            k = rng.randrange(E2E_LEN)
            w[k] = rng.choice([b for b in b"ACGT" if b != w[k]])
        w = bytes(w)
        reads.append(("r%d" % i, uc.revcomp(w) if rng.random() < 0.5 else w))
    return reads


def _e2e_files():
    d = os.path.join(CACHE, "unitig_prune_e2e")
    os.makedirs(d, exist_ok=True)
    prefix = os.path.join(d, "reads")
    reads = _e2e_case()
    if not all(os.path.exists(prefix + e) for e in (".bwt", ".rbwt", ".sai", ".rsai", ".fa")):
        seqs = [s.decode() for _, s in reads]
        po.Index.build(seqs).save(prefix + ".bwt", prefix + ".sai")
        po.Index.build(seqs, reverse=True).save(prefix + ".rbwt", prefix + ".rsai")
        with open(prefix + ".fa", "w") as f:
            f.write(mr.fasta_text([(n, s.decode()) for n, s in reads]))
    return prefix


@functools.lru_cache(maxsize=None)
def _e2e_run():
    """-> (edges of the GPU overlap run, the wrapper's result on them, expected_prune() on them, expected_trim() on them)"""
    import siga_amd
    named = _e2e_case()
    prefix = _e2e_files()
    names = [n for n, _ in named]
    reads = [s for _, s in named]
    pair = siga_amd.FMIndexPair.load(prefix, device=0, with_sai=True, resident=False)
    try:
        lengths = np.array([len(s) for s in reads], dtype=np.uint32)
        pair.set_reads(lengths, siga_amd.overlap.name_ranks(names))
        edges = siga_amd.OverlapBuilder(pair, prefix).overlap(reads, E2E_M, edges=True)["edges"]
    finally:
        pair.close()
    offs = np.zeros(len(reads) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(lengths, dtype=np.uint64)
    res = siga_amd.unitigs_prune(edges, lengths, b"".join(reads), offs, E2E_M, E2E_X, E2E_L, delta=E2E_DELTA, genome_size=E2E_G,
                                 uniq_threshold=E2E_T)
    recs = [tuple(int(x) for x in e) for e in edges.tolist()]
    exp = pc.expected_prune(reads, recs, E2E_M, E2E_X, E2E_L, None, E2E_DELTA, False, None, E2E_G, E2E_T)
    return edges, res, exp, tc.expected_trim(reads, recs, E2E_M, E2E_X, E2E_L)


def test_end_to_end():
    edges, res, exp, trimmed = _e2e_run()
    assert len(edges) > 2000  # (about one irreducible record per read at this coverage)
    _same(res, exp, "end to end")
    print("unitigs with trimming only", trimmed["status"][0], "with cutting", exp["status"][0], "records cut", exp["status"][12], "in rounds",
          exp["status"][13], "reads removed", trimmed["status"][9], "->", exp["status"][9])
    assert exp["status"][12] > 0 and exp["status"][14] > 0 and exp["status"][2] == 0 and exp["status"][3] == 0
    assert exp["status"][9] >= trimmed["status"][9] > 0  # (a cut only ever frees ends: what trimming alone removes goes here too)


def _want_texts(names, res, edges, m):
    from siga_amd.overlap import format_asqg
    plain = {"uflags": res["uflags"], "lay_offs": res["lay_offs"], "seq_offs": res["seq_offs"], "useqs": res["useqs"].tobytes(),
             "layout": res["layout"].tolist()}
    fa, lay = uc.render(names, plain)
    verts = tc.render_graph(plain)
    graph = format_asqg([(v[0], v[1], v[2].decode()) for v in verts], {"substring": [0] * len(verts), "edges": res["uedges"]}, m)
    cut = "".join("%s\t%s\t%d\t%d\n" % (names[int(e["query"])], names[int(e["target"])], int(e["length"]), int(r))
                  for e, r in zip(edges, res["cut"]) if int(r))
    return fa, lay, graph, tc.render_removed(names, res["removed"]), cut


def test_cli(tmp_path):
    from siga_amd import host
    prefix = _e2e_files()
    edges, res, _, _ = _e2e_run()
    names = [n for n, _ in _e2e_case()]
    want_fa, want_lay, want_graph, want_removed, want_cut = _want_texts(names, res, edges, E2E_M)
    assert want_cut.count("\n") == int(res["status"][12]) > 0
    fa, lay, gr, rm, ct = (str(tmp_path / f) for f in ("u.fa", "u.layout", "u.asqg", "u.removed", "u.cut"))
    base = [host.CLI_PATH, "unitig", "-m", str(E2E_M), "-p", prefix]
    r = subprocess.run(base + ["-x", str(E2E_X), "-n", str(E2E_L), "-d", str(E2E_DELTA), "-G", str(E2E_G), "-o", fa, "--layout", lay, "--graph", gr,
                               "--removed", rm, "--cut-edges", ct, prefix + ".fa"], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    assert open(fa).read() == want_fa and open(lay).read() == want_lay and open(gr).read() == want_graph
    assert open(rm).read() == want_removed and open(ct).read() == want_cut
    assert b"records cut" in r.stderr
    r = subprocess.run(base + ["--cut-terminal=%d" % E2E_X, "--min-branch-length=%d" % E2E_L, "--max-overlap-delta=%d" % E2E_DELTA,
                               "--genome-size=%d" % E2E_G, "--num-reads=%d" % len(names), "--uniq-threshold=%s" % E2E_T, "-o", fa,
                               "--cut-edges=" + ct, prefix + ".fa"], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    assert open(fa).read() == want_fa and open(ct).read() == want_cut
    # careful mode: the wrapper on the same records equals the rules, and the command line equals the wrapper, file for file
    cres, cexp = _careful_run()
    _same(cres, cexp, "end to end, careful")
    want_fa, want_lay, want_graph, want_removed, want_cut = _want_texts(names, cres, edges, E2E_M)
    r = subprocess.run(base + ["-x", str(E2E_X), "-n", str(E2E_L), "-d", str(E2E_DELTA), "-G", str(E2E_G), "--max-overlap-carefully", "-o", fa,
                               "--layout", lay, "--graph", gr, "--removed", rm, "--cut-edges", ct, prefix + ".fa"], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    assert open(fa).read() == want_fa and open(lay).read() == want_lay and open(gr).read() == want_graph
    assert open(rm).read() == want_removed and open(ct).read() == want_cut
    r = subprocess.run(base, capture_output=True)  # no READSFILE: the help text
    assert r.returncode == 0 and all(w in r.stdout for w in (b"--max-overlap-delta", b"--max-overlap-carefully", b"--num-reads", b"--genome-size",
                                                              b"--uniq-threshold", b"--cut-edges"))


def _careful_run():
    """-> (the wrapper's result with careful=True on the end-to-end records, expected_prune() for it)"""
    import siga_amd
    edges, _, _, _ = _e2e_run()
    reads = [s for _, s in _e2e_case()]
    lengths = np.array([len(s) for s in reads], dtype=np.uint32)
    offs = np.zeros(len(reads) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(lengths, dtype=np.uint64)
    res = siga_amd.unitigs_prune(edges, lengths, b"".join(reads), offs, E2E_M, E2E_X, E2E_L, delta=E2E_DELTA, careful=True, genome_size=E2E_G,
                                 uniq_threshold=E2E_T)
    recs = [tuple(int(x) for x in e) for e in edges.tolist()]
    return res, pc.expected_prune(reads, recs, E2E_M, E2E_X, E2E_L, None, E2E_DELTA, True, None, E2E_G, E2E_T)


def test_cli_refuses_delta_without_genome_size_or_rounds(tmp_path):
    from siga_amd import host
    prefix = _e2e_files()
    fa = str(tmp_path / "u.fa")
    base = [host.CLI_PATH, "unitig", "-m", str(E2E_M), "-p", prefix, "-o", fa]
    r = subprocess.run(base + ["-x", "10", "-d", "10", prefix + ".fa"], capture_output=True)
    assert r.returncode == 1 and b"--genome-size" in r.stderr
    r = subprocess.run(base + ["-d", "10", "-G", "12000", prefix + ".fa"], capture_output=True)
    assert r.returncode == 1 and b"--cut-terminal" in r.stderr
