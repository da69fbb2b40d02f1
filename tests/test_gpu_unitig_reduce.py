"""The transitive reduction in the rounds of `siga unitig` on the GPU (csrc/sigax_unitig.hip) against the serial restatement of its rules
(tests/reduce_cases.py): every case through the host entry point and some through the device one with every round enqueued, exactly --
offsets, flags, layout, bytes, removed, cut with bit 31, lifted records, all 40 counts; on five read sets the records left unflagged are
the CPU oracle's irreducible overlap run and the unitigs those of that run; reduce = 0 is the indel call; refusals; the command line."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch  # before the library loads: one HIP runtime per process

from oracle import pyoracle as po
from tests import indel_cases as ic
from tests import reduce_cases as rc
from tests import unitig_cases as uc
from tests.fixtures import CACHE
from tests.golden import make_reads as mr

pytestmark = pytest.mark.gpu
CASES = rc.hand_built()
IDS = [c["name"] for c in CASES]
CANARY = 64


def _same(res, exp, what):
    """res: the wrapper's dict (numpy arrays); exp: expected_reduce()'s"""
    status = res["status"].tolist()
    print(what, "status", status, "expected", exp["status"])
    assert status == exp["status"], what
    assert res["cut"].tolist() == exp["cut"], what
    assert res["removed"].tolist() == exp["removed"], what
    assert res["seq_offs"].tolist() == exp["seq_offs"] and res["lay_offs"].tolist() == exp["lay_offs"], what
    assert res["uflags"].tolist() == exp["uflags"], what
    assert [tuple(int(x) for x in p) for p in res["layout"].tolist()] == exp["layout"], what
    assert [tuple(int(x) for x in e) for e in res["uedges"].tolist()] == exp["uedges"], what
    assert res["useqs"].tobytes() == exp["useqs"], what


def _kw(case):
    return dict(delta=case["delta"], careful=case["careful"], num_reads=case["N"], genome_size=case["G"], uniq_threshold=case["T"],
                min_chimeric_length=case["Lc"], min_chimeric_coverage=case["Ac"], chimeric_delta=case["delta_c"], chimeric_threshold=case["Tc"],
                max_bubble_span=case["Lb"], bubble_divergence=case["D"], max_edits=case["Ed"], edit_permille=case["De"])


def _host(case, max_rounds=None, reduce=None):
    import siga_amd
    edges, lengths, seqs, offs = uc.arrays(case)
    return siga_amd.unitigs_reduce(edges, lengths, seqs, offs, case["m"], case["x"] if max_rounds is None else max_rounds, case["L"], case["C"],
                                   reduce=case.get("reduce", True) if reduce is None else reduce, **_kw(case))


def _opts(case, max_rounds=None, reduce=None, reserved=(0, 0, 0)):
    from siga_amd import _lib
    n = len(case["reads"])
    x, none = case["x"] if max_rounds is None else max_rounds, _lib.SIGAX_TRIM_NO_COVERAGE
    prune = _lib.PruneOpts(x, case["L"], none if case["C"] is None else case["C"], case["delta"], int(case["careful"]), 0,
                           n if case["N"] is None else case["N"], case["G"] or 0, case["T"])
    chim = _lib.ChimericOpts(prune, case["Lc"], none if case["Ac"] is None else case["Ac"], case["delta_c"], 0, case["Tc"])
    bub = _lib.BubbleOpts(chim, case["Lb"], _lib.SIGAX_BUBBLE_NO_BASES if case["D"] is None else case["D"], (C.c_uint32 * 2)(0, 0))
    ind = _lib.IndelOpts(bub, case["Ed"], case["De"], (C.c_uint32 * 2)(0, 0))
    return _lib.ReduceOpts(ind, int(case.get("reduce", True)) if reduce is None else reduce, (C.c_uint32 * 3)(*reserved))


def _device_call(case, max_rounds=None):
    """sigax_unitigs_reduce_device over torch buffers, each output buffer of exactly its size plus CANARY bytes of 0xEE; it enqueues
    every round (paced = false), so the rounds behind one that changed nothing run idle -> (dict like the wrapper's, the bytes beyond)"""
    from siga_amd import _lib
    L = _lib.lib()
    edges, lengths, seqs, offs = uc.arrays(case)
    n, ne, nb = len(lengths), len(edges), len(seqs)
    dev = torch.device("cuda:0")

    def up(a):
        a = np.frombuffer(a, dtype=np.uint8) if isinstance(a, bytes) else a.view(np.uint8).reshape(-1)
        return torch.from_numpy(a.copy()).to(dev) if a.size else torch.zeros(16, dtype=torch.uint8, device=dev)

    wb = C.c_uint64()
    assert L.sigax_unitigs_reduce_workspace(n, ne, 1, int(case["careful"]), C.byref(wb)) == 0
    d_edges, d_len, d_seqs, d_offs = up(edges), up(lengths), up(seqs), up(offs)
    sizes = {"seq_offs": 8 * (n + 1), "lay_offs": 8 * (n + 1), "uflags": 4 * n, "layout": 16 * n, "useqs": nb, "removed": 4 * n, "cut": 4 * ne,
             "uedges": 16 * ne, "status": 8 * 40, "work": wb.value}
    d = {k: torch.full((v + CANARY,), 0xEE, dtype=torch.uint8, device=dev) for k, v in sizes.items()}
    opts = _opts(case, max_rounds)
    torch.cuda.synchronize()
    rcode = L.sigax_unitigs_reduce_device(
        0, d_edges.data_ptr(), ne, d_len.data_ptr(), d_seqs.data_ptr(), d_offs.data_ptr(), n, case["m"], C.byref(opts), d["seq_offs"].data_ptr(),
        d["lay_offs"].data_ptr(), d["uflags"].data_ptr(), d["layout"].data_ptr(), d["useqs"].data_ptr(), d["removed"].data_ptr(),
        d["cut"].data_ptr(), d["uedges"].data_ptr(), d["status"].data_ptr(), d["work"].data_ptr(), wb.value, None)
    assert rcode == 0, _lib.last_error()
    torch.cuda.synchronize()
    h = {k: v.cpu().numpy() for k, v in d.items()}
    status = h["status"][:8 * 40].view(np.uint64)
    u, placed, lifted = int(status[0]), n - int(status[9]), int(status[11])
    assert u <= n and lifted <= ne and int(status[1]) <= nb and 0 <= placed
    res = {"status": status, "seq_offs": h["seq_offs"][:8 * (u + 1)].view(np.uint64), "lay_offs": h["lay_offs"][:8 * (u + 1)].view(np.uint64),
           "uflags": h["uflags"][:4 * u].view(np.uint32), "layout": h["layout"][:16 * placed].view(_lib.PLACEMENT_DTYPE),
           "useqs": h["useqs"][:int(status[1])], "removed": h["removed"][:4 * n].view(np.uint32), "cut": h["cut"][:4 * ne].view(np.uint32),
           "uedges": h["uedges"][:16 * lifted].view(_lib.EDGE_DTYPE)}
    tails = {k: h[k][sizes[k]:].tobytes() for k in sizes}
    return res, tails


def _untouched(tails, what):
    for k, t in tails.items():
        assert t == b"\xee" * len(t), "%s: bytes after %s were written" % (what, k)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_host_form_equals_the_restatement(case):
    _same(_host(case), rc.expected_of(case["name"]), case["name"])


@pytest.mark.parametrize("name", ["revive", "dead_witness_cut", "chain5", "wide_end", "participants_257", "participants_0"])
def test_device_form_with_every_round_enqueued(name):
    """ten rounds enqueued where one or two change anything: the passes of the rounds behind them are idle and the flags hold"""
    case = dict(rc.case_named(name), x=10)
    res, tails = _device_call(case)
    _same(res, rc.expected_of(name, 10), name)
    _untouched(tails, name)


@pytest.mark.parametrize("rounds", [0, 1, 2, 64])
def test_revive_round_by_round(rounds):
    case, exp = rc.case_named("revive"), rc.expected_of("revive", rounds)
    ac = case["claims"]["ac"]
    assert exp["cut"][ac] == (rc.TRANSITIVE if rounds == 0 else 0)
    _same(_host(case, rounds), exp, "revive, host, %d rounds" % rounds)
    res, tails = _device_call(case, rounds)
    _same(res, exp, "revive, device, %d rounds" % rounds)
    _untouched(tails, "revive")


def test_every_step_removes_something_in_one_call():
    """reduce, cut, trim, bubble, indel and chimeric all on, and each with something to take (reduce_cases.every_step asserts that on
    the restatement): a mark or a counter wired to another step's block shows in removed[]'s flag bits or in a status word"""
    case, exp = rc.every_step()
    res, tails = _device_call(case)
    _same(res, exp, "every_step")
    _untouched(tails, "every_step")


def test_revive_through_the_indel_call_without_the_record_stays_broken():
    import siga_amd
    case, irr = rc.case_named("revive"), rc.case_named("revive_irreducible")
    a, b, c = case["claims"]["abc"]
    where = rc.unit_of(_host(case))
    assert where[a] == where[c]
    edges, lengths, seqs, offs = uc.arrays(irr)
    plain = siga_amd.unitigs_indel(edges, lengths, seqs, offs, irr["m"], irr["x"], irr["L"], irr["C"], **_kw(irr))
    where = rc.unit_of(plain)
    assert where[a] != where[c] and int(plain["removed"][b]) == 1 | ic.CHIMERIC


def test_random_graphs_through_the_rounds():
    for seed in range(12):
        case = dict(rc.random_case(seed), x=3, L=60)  # (reads of up to 60 bases: ends of the line are trimmed, round by round)
        exp = rc.run(rc.expected_reduce, case)
        _same(_host(case), exp, case["name"] + ", host")
        if seed % 3 == 0:
            res, tails = _device_call(case)
            _same(res, exp, case["name"] + ", device")
            _untouched(tails, case["name"])


# ---- the yardstick from the reference: the CPU oracle's irreducible overlap run ----
@pytest.mark.parametrize("k", range(len(rc.ORACLE_SETS)), ids=[s[0] for s in rc.ORACLE_SETS])
def test_exhaustive_reduced_is_the_oracles_irreducible_run(k):
    import siga_amd
    s = rc.oracle_sets()[k]
    reads, m = s["reads"], s["m"]
    exh = uc.arrays({"reads": reads, "edges": s["exhaustive"]})
    irr = uc.arrays({"reads": reads, "edges": s["irreducible"]})
    res = siga_amd.unitigs_reduce(exh[0], exh[1], exh[2], exh[3], m, 0, 0)
    left = {e for e, x in zip(s["exhaustive"], res["cut"].tolist()) if not x & rc.TRANSITIVE}
    print(s["name"], "exhaustive", len(s["exhaustive"]), "irreducible", len(s["irreducible"]), "status", res["status"][32:36].tolist())
    assert left == set(s["irreducible"])
    assert res["status"][32:36].tolist() == [len(s["exhaustive"]) - len(s["irreducible"])] * 2 + [1, len(s["exhaustive"])]
    want = siga_amd.unitigs(irr[0], irr[1], irr[2], irr[3], m)
    for key in ("seq_offs", "lay_offs", "uflags", "layout", "useqs"):
        assert res[key].tobytes() == want[key].tobytes(), key


# ---- reduce = 0 is the indel call ----
@pytest.mark.parametrize("case", [c for c in ic.hand_built() if len(c["reads"]) <= 200][:12], ids=lambda c: c["name"])
def test_reduce_0_is_the_indel_call(case):
    import siga_amd
    edges, lengths, seqs, offs = uc.arrays(case)
    want = siga_amd.unitigs_indel(edges, lengths, seqs, offs, case["m"], case["x"], case["L"], case["C"], **_kw(case))
    got = _host(case, reduce=False)
    for k in ("seq_offs", "lay_offs", "uflags", "layout", "useqs", "removed", "uedges", "cut"):
        assert got[k].tobytes() == want[k].tobytes(), k
    assert got["status"][:32].tolist() == want["status"].tolist() and got["status"][32:].tolist() == [0] * 8
    assert not (got["cut"] & rc.TRANSITIVE).any()
    dres, tails = _device_call(dict(case, reduce=False))
    _untouched(tails, case["name"])
    assert dres["status"].tolist() == got["status"].tolist() and dres["cut"].tobytes() == got["cut"].tobytes()


def test_refusals_and_workspace():
    from siga_amd import _lib
    L = _lib.lib()
    E = _lib.SIGAX_E_ARG
    case = rc.case_named("triple")
    z = None
    nothing = [z] * 14 + [0, z]
    dev = lambda n, ne, o, *b: L.sigax_unitigs_reduce_device(0, b[0], ne, b[1], b[2], b[3], n, 20, o, *b[4:])  # noqa: E731
    assert dev(0, 0, C.byref(_opts(case)), *nothing) == 0
    assert dev(0, 0, C.byref(_opts(case, reduce=0)), *nothing) == 0
    assert dev(0, 0, None, *nothing) != 0 and "reduce options" in _lib.last_error()
    rcode = dev(0, 0, C.byref(_opts(case, reduce=2)), *nothing)
    assert rcode == E != 0 and "reduce 2" in _lib.last_error()
    for k in range(3):
        assert dev(0, 0, C.byref(_opts(case, reserved=[int(j == k) for j in range(3)])), *nothing) == E and "reserved5" in _lib.last_error()
    # a workspace one byte short
    n, ne = 4, 2
    wb = C.c_uint64()
    assert L.sigax_unitigs_reduce_workspace(n, ne, 1, 0, C.byref(wb)) == 0
    b = [torch.zeros(4096, dtype=torch.uint8, device="cuda:0") for _ in range(14)]
    p = [t.data_ptr() for t in b]
    work = torch.zeros(wb.value, dtype=torch.uint8, device="cuda:0")
    o = _opts(dict(case, N=4))
    args = lambda nbytes: (n, ne, C.byref(o), p[11], p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[12], p[9], p[10],  # noqa: E731
                           work.data_ptr(), nbytes, z)
    assert dev(*args(wb.value - 1)) == E and "sigax_unitigs_reduce_workspace" in _lib.last_error()
    assert dev(*args(wb.value)) == 0, _lib.last_error()  # (lengths, offsets and records all zero: every record malformed)
    torch.cuda.synchronize()
    # the grid of tests/test_unitig_workspace.py: never below the indel call's, and a multiple of 16
    for nr in (0, 1, 7, 4096, 1000000, (1 << 31) - 1):
        for nedges in (0, 5, 1 << 20, 1 << 32):
            for graph in (0, 1):
                for careful in (0, 1):
                    wi = C.c_uint64()
                    assert L.sigax_unitigs_indel_workspace(nr, nedges, graph, careful, C.byref(wi)) == 0
                    assert L.sigax_unitigs_reduce_workspace(nr, nedges, graph, careful, C.byref(wb)) == 0
                    assert wb.value > wi.value and wb.value % 16 == 0


def test_no_reads():
    import siga_amd
    none = np.zeros(0, dtype=np.uint32)
    res = siga_amd.unitigs_reduce(np.zeros(0, dtype=uc.EDGE_DTYPE), none, b"", np.zeros(1, dtype=np.uint64), 20, 10, 150)
    assert res["status"].tolist() == [0] * 40 and len(res["cut"]) == 0 and len(res["removed"]) == 0 and len(res["layout"]) == 0
    with pytest.raises(siga_amd.SigaxError, match="reduce"):
        siga_amd.unitigs_reduce(np.zeros(0, dtype=uc.EDGE_DTYPE), none, b"", np.zeros(1, dtype=np.uint64), 20, 10, 150, reduce=2)


# ---- the command line, on unitig_cases.end_to_end()'s 600 reads ----
def _e2e_prefix():
    d = os.path.join(CACHE, "unitig_e2e")
    os.makedirs(d, exist_ok=True)
    prefix = os.path.join(d, "reads")
    case = uc.end_to_end()
    if not all(os.path.exists(prefix + e) for e in (".bwt", ".rbwt", ".sai", ".rsai", ".fa")):
        seqs = [s.decode() for _, s in case["reads"]]
        po.Index.build(seqs).save(prefix + ".bwt", prefix + ".sai")
        po.Index.build(seqs, reverse=True).save(prefix + ".rbwt", prefix + ".rsai")
        with open(prefix + ".fa", "w") as f:
            f.write(mr.fasta_text([(n, s.decode()) for n, s in case["reads"]]))
    return prefix


@functools.lru_cache(maxsize=None)
def _e2e_records():
    """-> (names, exhaustive records, irreducible records) of the CPU oracle over the 600 reads, as (query name, target name, length)"""
    from siga_amd.overlap import name_ranks
    from tests.bigcheck import expected_edges
    case = uc.end_to_end()
    names = [n for n, _ in case["reads"]]
    seqs = [s.decode() for _, s in case["reads"]]
    fwd, rev = po.Index.build(seqs), po.Index.build(seqs, reverse=True)
    lengths = np.array([len(s) for s in seqs], dtype=np.uint32)
    out = []
    for irreducible in (False, True):
        got = po.overlap_batch(fwd, rev, seqs, uc.E2E_M, irreducible=irreducible)
        e = expected_edges(got["blocks"], got["block_offs"], fwd.sai(), rev.sai(), lengths, np.asarray(name_ranks(names)))
        out.append([tuple(int(x) for x in r) for r in e.tolist()])
    return names, out[0], out[1]


def test_cli(tmp_path):
    import subprocess

    from siga_amd import host
    prefix = _e2e_prefix()
    names, exh, irr = _e2e_records()
    fa, lay, fa2, lay2, fa3, red, cut = (str(tmp_path / f) for f in ("a.fa", "a.layout", "b.fa", "b.layout", "c.fa", "a.reduced", "a.cut"))
    base = [host.CLI_PATH, "unitig", "-m", str(uc.E2E_M), "-p", prefix]
    r = subprocess.run(base + ["-o", fa2, "--layout", lay2, prefix + ".fa"], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    r = subprocess.run(base + ["--exhaustive", "--reduce", "-o", fa, "--layout", lay, "--reduced-edges", red, prefix + ".fa"], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    assert open(fa).read() == open(fa2).read() and open(lay).read() == open(lay2).read()
    # (the set holds 11 duplicate reads and so 23 containment records; both runs of the oracle keep those, and the rest reduces exactly)
    got = sorted(tuple(line.split("\t")) for line in open(red).read().splitlines())
    want = sorted((names[q], names[t], str(ln)) for q, t, ln, _ in set(exh) - set(irr))
    assert got == want and len(got) > 0
    assert (b"%d records transitive" % len(got)) in r.stderr
    # --exhaustive alone: strictly more unitigs, so a --reduce that is silently ignored fails here
    r = subprocess.run(base + ["--exhaustive", "-o", fa3, prefix + ".fa"], capture_output=True)
    assert r.returncode == 0
    assert open(fa3).read().count(">") > open(fa).read().count(">")
    # --cut-edges lists the rounds of the -d cuts: no round of 2^31 or more, although cut[] carries bit 31
    r = subprocess.run(base + ["--exhaustive", "--reduce", "-x", "10", "-d", "10", "-G", str(uc.E2E_GENOME), "-o", fa3, "--cut-edges", cut,
                               "--reduced-edges", red, prefix + ".fa"], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    assert all(int(line.split("\t")[-1]) < (1 << 31) for line in open(cut).read().splitlines())
    assert len(open(red).read().splitlines()) > 0
    # --reduced-edges needs --reduce; the help text names both options
    r = subprocess.run(base + ["--reduced-edges", red, "-o", fa3, prefix + ".fa"], capture_output=True)
    assert r.returncode == 1 and b"--reduce" in r.stderr
    r = subprocess.run(base, capture_output=True)
    assert r.returncode == 0 and all(w in r.stdout for w in (b"--reduce ", b"--reduced-edges=FILE", b"see --reduce"))
