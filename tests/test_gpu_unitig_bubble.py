"""Bubble popping in the rounds of `siga unitig` on the GPU (csrc/sigax_unitig.hip) against the serial restatement of its rules
(tests/bubble_cases.py): every case through the host and the device entry point, exactly -- offsets, flags, layout, bytes, removed
with its flag bits, cut, lifted records, all 24 counts; Lb = 0 = siga_amd.unitigs_chimeric, unitigs_prune and unitigs_trim; canaries
and refusals; and end to end over the records of a GPU overlap run on reads that tile two haplotypes of a genome."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch  # before the library loads: one HIP runtime per process

from oracle import pyoracle as po
from tests import bubble_cases as bc
from tests import chimeric_cases as cc
from tests import prune_cases as pc
from tests import trim_cases as tc
from tests import unitig_cases as uc
from tests.fixtures import CACHE
from tests.golden import make_reads as mr

pytestmark = pytest.mark.gpu
CASES = bc.hand_built()
IDS = [c["name"] for c in CASES]
CC_CASES = cc.hand_built()
PC_CASES = [c for c in pc.hand_built() if len(c["reads"]) <= 40]
TC_CASES = tc.hand_built()


def _same(res, exp, what, bases=True, graph=True):
    """res: the wrapper's dict (numpy arrays); exp: expected_bubble()'s"""
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
    return siga_amd.unitigs_bubble(edges, lengths, seqs, offs, case["m"], case["x"] if max_rounds is None else max_rounds, case["L"], case["C"],
                                   delta=case["delta"], careful=case["careful"], num_reads=case["N"], genome_size=case["G"],
                                   uniq_threshold=case["T"], min_chimeric_length=case["Lc"], min_chimeric_coverage=case["Ac"],
                                   chimeric_delta=case["delta_c"], chimeric_threshold=case["Tc"], max_bubble_span=case["Lb"],
                                   bubble_divergence=case["D"], **kw)


CANARY = 64


N_STATUS = {"trim": 12, "prune": 16, "chimeric": 20, "bubble": 24}


def _opts(case, max_rounds=None, level="bubble"):
    from siga_amd import _lib
    n = len(case["reads"])
    x, cov = case["x"] if max_rounds is None else max_rounds, _lib.SIGAX_TRIM_NO_COVERAGE if case["C"] is None else case["C"]
    if level == "trim":
        return _lib.TrimOpts(x, case["L"], cov, 0)
    prune = _lib.PruneOpts(x, case["L"], cov, case["delta"], int(case["careful"]), 0, n if case["N"] is None else case["N"], case["G"] or 0, case["T"])
    if level == "prune":
        return prune
    chim = _lib.ChimericOpts(prune, case["Lc"], _lib.SIGAX_TRIM_NO_COVERAGE if case["Ac"] is None else case["Ac"], case["delta_c"], 0, case["Tc"])
    if level == "chimeric":
        return chim
    return _lib.BubbleOpts(chim, case["Lb"], _lib.SIGAX_BUBBLE_NO_BASES if case["D"] is None else case["D"], (C.c_uint32 * 2)(0, 0))


def _device_call(case, max_rounds=None, layout_only=False, graph=True, level="bubble"):
    """sigax_unitigs_bubble_device (or the device form of a lower `level`, over that call's scratch and status block) over torch buffers,
    each output buffer of exactly its size plus CANARY bytes of 0xEE -> (dict like the wrapper's, what lies beyond the bytes the call had
    to write)"""
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
    ns = N_STATUS[level]
    assert getattr(L, "sigax_unitigs_%s_workspace" % level)(n, ne, int(graph), *([] if level == "trim" else [int(case["careful"])]), C.byref(wb)) == 0
    d_edges, d_len, d_seqs, d_offs = up(edges), up(lengths), up(seqs), up(offs)
    sizes = {"seq_offs": 8 * (n + 1), "lay_offs": 8 * (n + 1), "uflags": 4 * n, "layout": 16 * n, "useqs": nb, "removed": 4 * n, "cut": 4 * ne,
             "uedges": 16 * ne, "status": 8 * ns, "work": wb.value}
    d = {k: out(v) for k, v in sizes.items()}
    opts = _opts(case, max_rounds, level)
    torch.cuda.synchronize()
    rc = getattr(L, "sigax_unitigs_%s_device" % level)(
        0, d_edges.data_ptr(), ne, d_len.data_ptr(), d_seqs.data_ptr(), d_offs.data_ptr(), n, case["m"], C.byref(opts), d["seq_offs"].data_ptr(),
        d["lay_offs"].data_ptr(), d["uflags"].data_ptr(), d["layout"].data_ptr(), None if layout_only else d["useqs"].data_ptr(),
        d["removed"].data_ptr(), *([] if level == "trim" else [d["cut"].data_ptr()]), d["uedges"].data_ptr() if graph else None,
        d["status"].data_ptr(), d["work"].data_ptr(), wb.value, None)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    h = {k: v.cpu().numpy() for k, v in d.items()}
    status = h["status"][:8 * ns].view(np.uint64)
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
    _same(_host(case), bc.expected_of(case["name"]), case["name"])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_device_form_equals_brute_force(case):
    res, tails = _device_call(case)
    _same(res, bc.expected_of(case["name"]), case["name"])
    _untouched(tails, case["name"])
    if len(case["reads"]) <= 200:  # the cut step and the chimeric step around it
        with_d = dict(case, delta=10, careful=True, Lc=case["Lc"] or 90)
        res, tails = _device_call(with_d)
        _same(res, bc.run(bc.expected_bubble, with_d), case["name"] + ", -d 10 carefully, -l")
        _untouched(tails, case["name"])


@pytest.mark.parametrize("rounds", [0, 1, 2, 3])
def test_second_round_round_by_round(rounds):
    case = bc.case_named("second_round")
    exp = bc.expected_of("second_round", rounds)
    assert exp["status"][6] == min(rounds, 2) and exp["status"][20] == (rounds >= 2)
    _same(_host(case, rounds), exp, "second_round, host, %d rounds" % rounds)
    res, tails = _device_call(case, rounds)
    _same(res, exp, "second_round, device, %d rounds" % rounds)
    _untouched(tails, "second_round")


def test_random_graphs():
    popped = kept = 0
    for seed in range(300):
        case = bc.random_case(seed)
        exp = bc.run(bc.expected_bubble, case)
        popped += exp["status"][20] > 0
        kept += exp["status"][23] > 0
        if seed % 3 == 0:
            _same(_host(case), exp, case["name"] + ", host")
        res, tails = _device_call(case)
        _same(res, exp, case["name"] + ", device")
        _untouched(tails, case["name"])
    assert popped >= 150 and kept >= 75


def test_large_graph():
    case = bc.large_case()
    exp = bc.run(bc.expected_bubble, case)
    # many workgroups, 200 groups, arms of two reads, and rounds after the last change
    assert 80 <= exp["status"][20] <= 120 and exp["status"][23] >= 80 and 1 <= exp["status"][22] <= exp["status"][6] < case["x"], exp["status"]
    res, tails = _device_call(case)
    _same(res, exp, "large, device")
    _untouched(tails, "large")


def _identical(got, want, n_status):
    for k in ("seq_offs", "lay_offs", "uflags", "layout", "useqs", "removed", "uedges"):
        assert got[k].tobytes() == want[k].tobytes(), k
    assert got["status"][:n_status].tolist() == want["status"].tolist() and got["status"][n_status:].tolist() == [0] * (24 - n_status)
    assert not (got["removed"] & bc.BUBBLE).any()


@pytest.mark.parametrize("case", CC_CASES, ids=[c["name"] for c in CC_CASES])
def test_lb_0_is_unitigs_chimeric(case):
    import siga_amd
    edges, lengths, seqs, offs = uc.arrays(case)
    want = siga_amd.unitigs_chimeric(edges, lengths, seqs, offs, case["m"], case["x"], case["L"], case["C"], delta=case["delta"],
                                     careful=case["careful"], num_reads=case["N"], genome_size=case["G"], uniq_threshold=case["T"],
                                     min_chimeric_length=case["Lc"], min_chimeric_coverage=case["Ac"], chimeric_delta=case["delta_c"],
                                     chimeric_threshold=case["Tc"])
    d = bc.with_bubble_keys(case, Lb=0, D=7)
    dres, tails = _device_call(d)
    _untouched(tails, case["name"])
    for got in (_host(d), dres):
        _identical(got, want, 20)
        assert got["cut"].tobytes() == want["cut"].tobytes()


@pytest.mark.parametrize("case", PC_CASES, ids=[c["name"] for c in PC_CASES])
def test_lb_0_and_lc_0_is_unitigs_prune(case):
    import siga_amd
    edges, lengths, seqs, offs = uc.arrays(case)
    want = siga_amd.unitigs_prune(edges, lengths, seqs, offs, case["m"], case["x"], case["L"], case["C"], delta=case["delta"],
                                  careful=case["careful"], num_reads=case["N"], genome_size=case["G"], uniq_threshold=case["T"])
    got = _host(bc.with_bubble_keys(case, Lb=0))
    _identical(got, want, 16)
    assert got["cut"].tobytes() == want["cut"].tobytes()


@pytest.mark.parametrize("case", TC_CASES, ids=[c["name"] for c in TC_CASES])
def test_lb_0_lc_0_and_delta_0_is_unitigs_trim(case):
    import siga_amd
    edges, lengths, seqs, offs = uc.arrays(case)
    want = siga_amd.unitigs_trim(edges, lengths, seqs, offs, case["m"], case["x"], case["L"], case["C"])
    got = _host(bc.with_bubble_keys(case, Lb=0))
    _identical(got, want, 12)
    assert not got["cut"].any() and len(got["cut"]) == len(edges)


# ---- a call whose upper steps are off runs as the lower call: the ladder through the device forms ----
def _ladder(case, upper, lower):
    """the device form `upper` with its own steps off (the keys of `case` say which) against the device form `lower`: every output byte,
    the counts beyond the lower call's zero, cut all zero where the lower call has none, every canary"""
    got, gtails = _device_call(case, level=upper)
    want, wtails = _device_call(case, level=lower)
    _untouched(gtails, "%s as %s" % (upper, lower))
    _untouched(wtails, lower)
    k = N_STATUS[lower]
    print(upper, "as", lower, "status", got["status"].tolist(), "expected", want["status"].tolist())
    assert got["status"][:k].tolist() == want["status"].tolist() and got["status"][k:].tolist() == [0] * (N_STATUS[upper] - k)
    for key in ("removed", "layout", "seq_offs", "lay_offs", "uflags", "useqs", "uedges"):
        assert got[key].tobytes() == want[key].tobytes(), key
    if lower == "trim":
        assert len(got["cut"]) == len(case["edges"]) and not got["cut"].any()
    else:
        assert got["cut"].tobytes() == want["cut"].tobytes()
    return want


@pytest.mark.parametrize("upper", ["bubble", "chimeric", "prune"])
def test_device_ladder_down_to_trim(upper):
    case = bc.with_bubble_keys(tc.case_named("cascade"), Lb=0)
    assert case["Lb"] == 0 and case["Lc"] == 0 and case["delta"] == 0 and len(case["reads"]) <= 60
    want = _ladder(case, upper, "trim")
    assert want["status"].tolist() == tc.expected_of("cascade")["status"] and want["status"][6] == 3  # (the rounds did run)


def test_device_ladder_bubble_to_chimeric():
    case = bc.with_bubble_keys(cc.case_named("second_round"), Lb=0)
    assert case["Lc"] > 0
    want = _ladder(case, "bubble", "chimeric")
    assert want["status"].tolist() == cc.expected_of("second_round")["status"] and want["status"][16] > 0


def test_device_ladder_chimeric_to_prune():
    case = bc.with_bubble_keys(pc.case_named("cascade"), Lb=0)
    assert case["Lc"] == 0 and case["delta"] > 0 and len(case["reads"]) <= 40
    want = _ladder(case, "chimeric", "prune")
    assert want["status"].tolist() == pc.expected_of("cascade")["status"] and want["status"][12] > 0


def test_last_round_slot():
    """max_rounds = 64, the most there are: the host form stops after the first idle round, the device form enqueues all 64"""
    case, exp = bc.case_named("second_round"), bc.expected_of("second_round", 64)
    assert exp["status"][6] == 2 and exp["status"][20] == 1
    _same(_host(case, 64), exp, "second_round, host, 64 rounds")
    res, tails = _device_call(case, 64)
    _same(res, exp, "second_round, device, 64 rounds")
    _untouched(tails, "second_round, 64 rounds")


@pytest.mark.parametrize("name", ["two_arms", "chains_flipped", "second_round", "three_arms"])
def test_graph_off_and_layout_only(name):
    case, exp = bc.case_named(name), bc.expected_of(name)
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
    assert L.sigax_unitigs_bubble_workspace(1 << 31, 0, 1, 0, C.byref(wb)) == E
    assert L.sigax_unitigs_bubble_workspace(10, (1 << 32) + 1, 1, 0, C.byref(wb)) == E
    assert L.sigax_unitigs_bubble_workspace(10, 100, 1, 0, None) == E
    assert L.sigax_unitigs_bubble_workspace(10, 100, 1, 0, C.byref(wb)) == 0
    mine = wb.value
    # the chimeric call's scratch, 60 bytes per read, 12 per slot of a table of 32, and the counters
    assert L.sigax_unitigs_chimeric_workspace(10, 100, 1, 0, C.byref(wb)) == 0 and wb.value + 60 * 10 + 12 * 32 + 25216 <= mine <= wb.value + 26400
    z = None

    def opts(**over):
        o = dict(max_rounds=10, min_branch_length=150, min_branch_coverage=_lib.SIGAX_TRIM_NO_COVERAGE, delta=0, careful=0, reserved=0,
                 num_reads=4, genome_size=0, uniq_threshold=13.0, min_chimeric_length=0, min_chimeric_coverage=_lib.SIGAX_TRIM_NO_COVERAGE,
                 chimeric_delta=0, reserved2=0, chimeric_threshold=0.0, max_bubble_span=40, max_divergence_permille=50, r0=0, r1=0)
        o.update(over)
        prune = _lib.PruneOpts(*[o[k] for k, _ in _lib.PruneOpts._fields_])
        chim = _lib.ChimericOpts(prune, *[o[k] for k, _ in _lib.ChimericOpts._fields_[1:]])
        return C.byref(_lib.BubbleOpts(chim, o["max_bubble_span"], o["max_divergence_permille"], (C.c_uint32 * 2)(o["r0"], o["r1"])))

    dev = lambda n, ne, o, *b: L.sigax_unitigs_bubble_device(0, b[0], ne, b[1], b[2], b[3], n, 20, o, *b[4:])  # noqa: E731
    nothing = [z] * 14 + [0, z]
    assert dev(0, 0, opts(), *nothing) == 0  # n_reads == 0; the bubble step needs neither G nor N
    assert dev(0, 0, None, *nothing) == E
    assert dev(0, 0, opts(r0=1), *nothing) == E and "reserved3" in _lib.last_error()
    assert dev(0, 0, opts(r1=1), *nothing) == E and "reserved3" in _lib.last_error()
    assert dev(0, 0, opts(reserved2=1), *nothing) == E and "reserved2" in _lib.last_error()
    assert dev(0, 0, opts(reserved=1), *nothing) == E and "reserved" in _lib.last_error()
    assert dev(0, 0, opts(careful=2), *nothing) == E
    assert dev(0, 0, opts(min_chimeric_length=100), *nothing) == E and "genome_size" in _lib.last_error()
    assert dev(0, 0, opts(delta=10), *nothing) == E and "genome_size" in _lib.last_error()
    assert dev(0, 0, opts(max_rounds=65), *nothing) == E and "max_rounds" in _lib.last_error()
    assert dev(4, 0, opts(num_reads=3), *nothing) == E and "num_reads" in _lib.last_error()
    assert dev(4, 0, opts(), *nothing) == E  # NULL buffers
    n, ne = 4, 2
    assert L.sigax_unitigs_bubble_workspace(n, ne, 1, 1, C.byref(wb)) == 0
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
    assert dev(*args(work.data_ptr(), wb.value, seqs=z)) == E  # a bases test without the bases
    assert dev(*args(work.data_ptr(), wb.value, seqs=z, o=opts(max_divergence_permille=_lib.SIGAX_BUBBLE_NO_BASES))) == E
    assert dev(*args(work.data_ptr(), wb.value, ct=z)) == E
    assert dev(*args(work.data_ptr(), wb.value, ct=p[12] + 2)) == E and "d_cut" in _lib.last_error()
    assert dev(*args(work.data_ptr(), wb.value, rm=z)) == E
    assert dev(*args(work.data_ptr(), wb.value, st=z)) == E
    assert dev(*args(work.data_ptr(), wb.value, st=p[10] + 4)) == E
    assert dev(*args(work.data_ptr(), wb.value, ue=p[9] + 8)) == E and "aligned" in _lib.last_error()
    assert dev(*args(work.data_ptr(), wb.value)) == 0, _lib.last_error()  # (lengths, offsets and records all zero: every record malformed)
    assert dev(*args(work.data_ptr(), wb.value, ue=z, us=z, o=opts(max_bubble_span=0))) == 0, _lib.last_error()
    torch.cuda.synchronize()
    nu = C.c_uint64()
    v = [C.c_void_p() for _ in range(8)]
    st = (C.c_uint64 * 24)()
    host = lambda nr, o, pn, ps: L.sigax_unitigs_bubble_host(0, z, 0, z, z, z, nr, 20, o, pn, *[C.byref(x) for x in v], ps)  # noqa: E731
    assert host(0, opts(), C.byref(nu), st) == 0 and nu.value == 0 and list(st) == [0] * 24
    for x in v:
        L.sigax_free(x)
    assert host(0, opts(), None, st) == E
    assert host(0, opts(), C.byref(nu), None) == E
    assert host(0, None, C.byref(nu), st) == E
    assert host(0, opts(r0=7), C.byref(nu), st) == E
    assert host(0, opts(min_chimeric_length=50), C.byref(nu), st) == E
    assert host(3, opts(num_reads=2), C.byref(nu), st) == E
    assert host(3, opts(), C.byref(nu), st) == E  # NULL buffers


def test_no_reads():
    import siga_amd
    none = np.zeros(0, dtype=np.uint32)
    res = siga_amd.unitigs_bubble(np.zeros(0, dtype=uc.EDGE_DTYPE), none, b"", np.zeros(1, dtype=np.uint64), 20, 10, 150, max_bubble_span=40)
    assert res["status"].tolist() == [0] * 24 and len(res["cut"]) == 0 and len(res["removed"]) == 0 and len(res["layout"]) == 0


# ---- end to end: the edge records of a GPU overlap run over reads of two haplotypes ----
def _e2e_files():
    d = os.path.join(CACHE, "unitig_bubble_e2e")
    os.makedirs(d, exist_ok=True)
    prefix = os.path.join(d, "reads")
    names, reads = bc.end_to_end()
    if not all(os.path.exists(prefix + e) for e in (".bwt", ".rbwt", ".sai", ".rsai", ".fa")):
        seqs = [s.decode() for s in reads]
        po.Index.build(seqs).save(prefix + ".bwt", prefix + ".sai")
        po.Index.build(seqs, reverse=True).save(prefix + ".rbwt", prefix + ".rsai")
        with open(prefix + ".fa", "w") as f:
            f.write(mr.fasta_text(list(zip(names, seqs))))
    return prefix


@functools.lru_cache(maxsize=None)
def _e2e_run():
    """-> (edges of the GPU overlap run, the wrapper's result on them, expected_bubble() on them, the result without -b)"""
    import siga_amd
    names, reads = bc.end_to_end()
    prefix = _e2e_files()
    pair = siga_amd.FMIndexPair.load(prefix, device=0, with_sai=True, resident=False)
    try:
        lengths = np.array([len(s) for s in reads], dtype=np.uint32)
        pair.set_reads(lengths, siga_amd.overlap.name_ranks(names))
        edges = siga_amd.OverlapBuilder(pair, prefix).overlap(reads, bc.E2E_M, edges=True)["edges"]
    finally:
        pair.close()
    offs = np.zeros(len(reads) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(lengths, dtype=np.uint64)
    res = siga_amd.unitigs_bubble(edges, lengths, b"".join(reads), offs, bc.E2E_M, bc.E2E_X, bc.E2E_L, max_bubble_span=bc.E2E_LB,
                                  bubble_divergence=bc.E2E_D)
    plain = siga_amd.unitigs_bubble(edges, lengths, b"".join(reads), offs, bc.E2E_M, bc.E2E_X, bc.E2E_L)
    recs = [tuple(int(x) for x in e) for e in edges.tolist()]
    exp = bc.expected_bubble(reads, recs, bc.E2E_M, bc.E2E_X, bc.E2E_L, None, Lb=bc.E2E_LB, D=bc.E2E_D)
    return edges, res, exp, plain


def test_end_to_end():
    edges, res, exp, plain = _e2e_run()
    _, reads = bc.end_to_end()
    assert len(edges) > len(reads) // 2
    _same(res, exp, "end to end")
    print("arms popped", exp["status"][20], "unitigs with -b", exp["status"][0], "without", int(plain["status"][0]))
    # six variant sites: arms go, and fewer unitigs are left than without the step
    assert exp["status"][20] >= 1 and exp["status"][0] < int(plain["status"][0])


def test_cli(tmp_path):
    import subprocess

    from siga_amd import host
    prefix = _e2e_files()
    edges, res, _, _ = _e2e_run()
    names, _ = bc.end_to_end()
    plain = {"uflags": res["uflags"], "lay_offs": res["lay_offs"], "seq_offs": res["seq_offs"], "useqs": res["useqs"].tobytes(),
             "layout": res["layout"].tolist()}
    want_fa, _ = uc.render(names, plain)
    want_removed = tc.render_removed(names, res["removed"] & ~np.uint32(bc.BUBBLE))
    want_bubbles = "".join("%s\t%d\n" % (names[r], int(x) & ~bc.BUBBLE) for r, x in enumerate(res["removed"]) if int(x) & bc.BUBBLE)
    assert want_bubbles.count("\n") == int(res["status"][21]) > 0
    fa, rm, bu = (str(tmp_path / f) for f in ("u.fa", "u.removed", "u.bubbles"))
    base = [host.CLI_PATH, "unitig", "-m", str(bc.E2E_M), "-p", prefix]
    r = subprocess.run(base + ["-x", str(bc.E2E_X), "-n", str(bc.E2E_L), "-b", str(bc.E2E_LB), "--bubble-divergence", str(bc.E2E_D), "-o", fa,
                               "--removed", rm, "--bubbles", bu, prefix + ".fa"], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    assert open(fa).read() == want_fa and open(rm).read() == want_removed and open(bu).read() == want_bubbles
    assert b"bubble arms popped" in r.stderr
    # the wrapper of the host library, with the default divergence: the counts of the library call
    st = host.unitig_file(prefix + ".fa", prefix, bc.E2E_M, out=fa, cut_terminal=bc.E2E_X, min_branch_length=bc.E2E_L, max_bubble_span=bc.E2E_LB,
                          bubble_divergence=bc.E2E_D, bubbles=bu)
    assert open(fa).read() == want_fa and open(bu).read() == want_bubbles
    assert (st["bubbles_popped"], st["bubble_reads"], st["bubbles_kept"]) == tuple(int(x) for x in res["status"][[20, 21, 23]])
    # --no-bubble-bases pops at least as many arms
    r = subprocess.run(base + ["--cut-terminal=%d" % bc.E2E_X, "--min-branch-length=%d" % bc.E2E_L, "--max-bubble-span=%d" % bc.E2E_LB,
                               "--no-bubble-bases", "-o", fa, "--bubbles=" + bu, prefix + ".fa"], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    assert open(bu).read().count("\n") >= want_bubbles.count("\n")
    # the refusals: -b needs -x; the other three need -b
    r = subprocess.run(base + ["-b", "40", "-o", fa, prefix + ".fa"], capture_output=True)
    assert r.returncode == 1 and b"--cut-terminal" in r.stderr
    r = subprocess.run(base + ["-x", "10", "--bubbles", bu, "-o", fa, prefix + ".fa"], capture_output=True)
    assert r.returncode == 1 and b"--max-bubble-span" in r.stderr
    r = subprocess.run(base + ["-x", "10", "--no-bubble-bases", "-o", fa, prefix + ".fa"], capture_output=True)
    assert r.returncode == 1 and b"--max-bubble-span" in r.stderr
    r = subprocess.run(base, capture_output=True)  # no READSFILE: the help text
    assert r.returncode == 0 and all(w in r.stdout for w in (b"--max-bubble-span", b"--bubble-divergence", b"--no-bubble-bases", b"--bubbles=FILE"))
