"""Indel bubble popping in the rounds of `siga unitig` on the GPU (csrc/sigax_unitig.hip) against the serial restatement of its rules
(tests/indel_cases.py): every case through the host and the device entry point, exactly -- offsets, flags, layout, bytes, removed with
its flag bits, cut, lifted records, all 32 counts; E = 0 = the bubble call bit for bit; canaries, hostile tables and refusals; the
calls of one pipeline on one stream; and end to end over the records of a GPU overlap run on reads that tile two haplotypes apart by
substitutions and short indels, through the library, the wrapper and the command line."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch  # before the library loads: one HIP runtime per process

from oracle import pyoracle as po
from tests import bubble_cases as bc
from tests import indel_cases as ic
from tests import trim_cases as tc
from tests import unitig_cases as uc
from tests.fixtures import CACHE
from tests.golden import make_reads as mr

pytestmark = pytest.mark.gpu
CASES = ic.hand_built()
IDS = [c["name"] for c in CASES]
CANARY = 64
N_STATUS = {"bubble": 24, "indel": 32}


def _same(res, exp, what, bases=True, graph=True):
    """res: the wrapper's dict (numpy arrays); exp: expected_indel()'s"""
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


def _kw(case):
    return dict(delta=case["delta"], careful=case["careful"], num_reads=case["N"], genome_size=case["G"], uniq_threshold=case["T"],
                min_chimeric_length=case["Lc"], min_chimeric_coverage=case["Ac"], chimeric_delta=case["delta_c"], chimeric_threshold=case["Tc"],
                max_bubble_span=case["Lb"], bubble_divergence=case["D"])


def _host(case, max_rounds=None, **kw):
    import siga_amd
    edges, lengths, seqs, offs = uc.arrays(case)
    return siga_amd.unitigs_indel(edges, lengths, seqs, offs, case["m"], case["x"] if max_rounds is None else max_rounds, case["L"], case["C"],
                                  max_edits=case["Ed"], edit_permille=case["De"], **_kw(case), **kw)


def _opts(case, max_rounds=None, level="indel"):
    from siga_amd import _lib
    n = len(case["reads"])
    x, none = case["x"] if max_rounds is None else max_rounds, _lib.SIGAX_TRIM_NO_COVERAGE
    prune = _lib.PruneOpts(x, case["L"], none if case["C"] is None else case["C"], case["delta"], int(case["careful"]), 0,
                           n if case["N"] is None else case["N"], case["G"] or 0, case["T"])
    chim = _lib.ChimericOpts(prune, case["Lc"], none if case["Ac"] is None else case["Ac"], case["delta_c"], 0, case["Tc"])
    bub = _lib.BubbleOpts(chim, case["Lb"], _lib.SIGAX_BUBBLE_NO_BASES if case["D"] is None else case["D"], (C.c_uint32 * 2)(0, 0))
    return bub if level == "bubble" else _lib.IndelOpts(bub, case["Ed"], case["De"], (C.c_uint32 * 2)(0, 0))


def _device_call(case, max_rounds=None, layout_only=False, graph=True, level="indel", stream=None, arrays=None):
    """sigax_unitigs_indel_device (or the bubble call's device form, over that call's scratch and status block) over torch buffers, each
    output buffer of exactly its size plus CANARY bytes of 0xEE -> (dict like the wrapper's, what lies beyond the bytes the call had to
    write).  arrays: (edges, lengths, seqs, offs) in place of the case's own: tables that hold anything."""
    from siga_amd import _lib
    L = _lib.lib()
    edges, lengths, seqs, offs = arrays or uc.arrays(case)
    n, ne, nb = len(lengths), len(edges), len(seqs)
    dev = torch.device("cuda:0")

    def up(a):
        a = np.frombuffer(a, dtype=np.uint8) if isinstance(a, bytes) else a.view(np.uint8).reshape(-1)
        return torch.from_numpy(a.copy()).to(dev) if a.size else torch.zeros(16, dtype=torch.uint8, device=dev)

    def out(nbytes):
        return torch.full((nbytes + CANARY,), 0xEE, dtype=torch.uint8, device=dev)

    wb = C.c_uint64()
    ns = N_STATUS[level]
    assert getattr(L, "sigax_unitigs_%s_workspace" % level)(n, ne, int(graph), int(case["careful"]), C.byref(wb)) == 0
    d_edges, d_len, d_seqs, d_offs = up(edges), up(lengths), up(seqs), up(offs)
    sizes = {"seq_offs": 8 * (n + 1), "lay_offs": 8 * (n + 1), "uflags": 4 * n, "layout": 16 * n, "useqs": nb, "removed": 4 * n, "cut": 4 * ne,
             "uedges": 16 * ne, "status": 8 * ns, "work": wb.value}
    d = {k: out(v) for k, v in sizes.items()}
    opts = _opts(case, max_rounds, level)
    torch.cuda.synchronize()
    rc = getattr(L, "sigax_unitigs_%s_device" % level)(
        0, d_edges.data_ptr(), ne, d_len.data_ptr(), d_seqs.data_ptr(), d_offs.data_ptr(), n, case["m"], C.byref(opts), d["seq_offs"].data_ptr(),
        d["lay_offs"].data_ptr(), d["uflags"].data_ptr(), d["layout"].data_ptr(), None if layout_only else d["useqs"].data_ptr(),
        d["removed"].data_ptr(), d["cut"].data_ptr(), d["uedges"].data_ptr() if graph else None, d["status"].data_ptr(), d["work"].data_ptr(),
        wb.value, stream)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    h = {k: v.cpu().numpy() for k, v in d.items()}
    status = h["status"][:8 * ns].view(np.uint64)
    u, placed, lifted = int(status[0]), n - int(status[9]), int(status[11])
    assert u <= n and lifted <= ne and int(status[1]) <= nb and 0 <= placed
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
    _same(_host(case), ic.expected_of(case["name"]), case["name"])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_device_form_equals_brute_force(case):
    res, tails = _device_call(case)
    _same(res, ic.expected_of(case["name"]), case["name"])
    _untouched(tails, case["name"])
    if len(case["reads"]) <= 40:  # the cut step and the chimeric step around it
        with_d = dict(case, delta=10, careful=True, Lc=case["Lc"] or 90)
        res, tails = _device_call(with_d)
        _same(res, ic.run(ic.expected_indel, with_d), case["name"] + ", -d 10 carefully, -l")
        _untouched(tails, case["name"])


@pytest.mark.parametrize("rounds", [0, 1, 2, 3, 10, 64])
def test_second_round_round_by_round(rounds):
    """the bubble that appears in round 2; ten and sixty-four rounds, all but two of them idle: the host form stops, the device form enqueues all"""
    case = ic.case_named("second_round")
    exp = ic.expected_of("second_round", rounds)
    assert exp["status"][6] == min(rounds, 2) and exp["status"][24] == (rounds >= 2) and exp["status"][26] == (rounds >= 2)
    _same(_host(case, rounds), exp, "second_round, host, %d rounds" % rounds)
    res, tails = _device_call(case, rounds)
    _same(res, exp, "second_round, device, %d rounds" % rounds)
    _untouched(tails, "second_round")


def test_counter_slots_wrap_with_both_block_shapes():
    """indel_cases.many_bubbles (44 indel bubbles, 40 plain ones and 105 tips among 2289 reads, asserted there): the compare kernel runs more than 32 one-wave workgroups and the
    256-lane kernels more than 32 waves, so every counter is the sum of slots that were added to more than once"""
    case, exp = ic.many_bubbles()
    res, tails = _device_call(case)
    _same(res, exp, "many_bubbles")
    _untouched(tails, "many_bubbles")


def test_random_graphs():
    seen = {}
    for seed in range(0, 300, 3):
        case = ic.random_case(seed)
        exp = ic.run(ic.expected_indel, case)
        for e in exp["indel_log"]:
            seen[e["cls"]] = seen.get(e["cls"], 0) + 1
        if seed % 9 == 0:
            _same(_host(case), exp, case["name"] + ", host")
        res, tails = _device_call(case)
        _same(res, exp, case["name"] + ", device")
        _untouched(tails, case["name"])
    print(seen)
    assert all(seen.get(k, 0) >= 3 for k in ("POPPED", "KEPT_EDITS", "KEPT_PERMILLE", "SAME_SPAN", "FAR")), seen


@pytest.mark.parametrize("name", ["three_bubble_keeps", "arms130", "entered_111", "span_4096_loser"])
def test_order_does_not_matter(name):
    case, exp = ic.case_named(name), ic.expected_of(name)
    other, new = ic.shuffled(case, 11, 6)
    res, tails = _device_call(other)
    _untouched(tails, name)
    assert res["status"].tolist() == exp["status"]
    assert [int(res["removed"][new[r]]) for r in range(len(new))] == exp["removed"]


# ---- E = 0 is the bubble call, bit for bit ----
@pytest.mark.parametrize("case", [c for c in bc.hand_built() if len(c["reads"]) <= 200], ids=lambda c: c["name"])
def test_e_0_is_the_bubble_call(case):
    import siga_amd
    edges, lengths, seqs, offs = uc.arrays(case)
    want = siga_amd.unitigs_bubble(edges, lengths, seqs, offs, case["m"], case["x"], case["L"], case["C"], **_kw(case))
    d = ic.with_indel_keys(case, Ed=0, De=7)
    dres, tails = _device_call(d)
    _untouched(tails, case["name"])
    bres, btails = _device_call(d, level="bubble")
    _untouched(btails, case["name"])
    for got in (_host(d), dres):
        for k in ("seq_offs", "lay_offs", "uflags", "layout", "useqs", "removed", "uedges", "cut"):
            assert got[k].tobytes() == want[k].tobytes() == bres[k].tobytes(), k
        assert got["status"][:24].tolist() == want["status"].tolist() == bres["status"].tolist() and got["status"][24:].tolist() == [0] * 8
        assert not (got["removed"] & ic.INDEL).any()


def test_indel_cases_without_the_step_keep_both_arms():
    """the same cases through the bubble call: the arms this step pops stay, so the tests above fail without it"""
    import siga_amd
    case = ic.case_named("deleted_middle")
    edges, lengths, seqs, offs = uc.arrays(case)
    plain = siga_amd.unitigs_bubble(edges, lengths, seqs, offs, case["m"], case["x"], case["L"], case["C"], **_kw(case))
    assert int(plain["status"][0]) == 4 and not plain["removed"].any() and int(_host(case)["status"][0]) == 1


@pytest.mark.parametrize("name", ["deleted_middle", "span_4096_winner", "second_round", "three_bubble_keeps"])
def test_graph_off_and_layout_only(name):
    case, exp = ic.case_named(name), ic.expected_of(name)
    _same(_host(case, graph=False), exp, name + ", host, no graph", graph=False)
    _same(_host(case, bases=False), exp, name + ", host, layout only", bases=False)
    res, tails = _device_call(case, graph=False)
    _same(res, exp, name + ", device, no graph", graph=False)
    _untouched(tails, name)
    res, tails = _device_call(case, layout_only=True)
    _same(res, exp, name + ", device, layout only", bases=False)
    _untouched(tails, name)


def test_calls_on_one_stream():
    """unitigs, then the indel call over the same reads, enqueued on one non-default stream without a wait between them"""
    from siga_amd import _lib
    L = _lib.lib()
    case = ic.case_named("three_bubble_pops")
    edges, lengths, seqs, offs = uc.arrays(case)
    n, ne, nb = len(lengths), len(edges), len(seqs)
    st = torch.cuda.Stream()
    dev = torch.device("cuda:0")
    up = lambda a: torch.from_numpy((np.frombuffer(a, dtype=np.uint8) if isinstance(a, bytes) else a.view(np.uint8).reshape(-1)).copy()).to(dev)  # noqa: E731
    d_edges, d_len, d_seqs, d_offs = up(edges), up(lengths), up(seqs), up(offs)
    z = lambda k: torch.zeros(k + 16, dtype=torch.uint8, device=dev)  # noqa: E731
    wb, wb0 = C.c_uint64(), C.c_uint64()
    assert L.sigax_unitigs_workspace(n, ne, C.byref(wb0)) == 0 and L.sigax_unitigs_indel_workspace(n, ne, 1, 0, C.byref(wb)) == 0
    plain = {k: z(v) for k, v in (("so", 8 * (n + 1)), ("lo", 8 * (n + 1)), ("uf", 4 * n), ("lay", 16 * n), ("us", nb), ("st", 48), ("w", wb0.value))}
    full = {k: z(v) for k, v in (("so", 8 * (n + 1)), ("lo", 8 * (n + 1)), ("uf", 4 * n), ("lay", 16 * n), ("us", nb), ("rm", 4 * n), ("ct", 4 * ne),
                                 ("ue", 16 * ne), ("st", 256), ("w", wb.value))}
    opts = _opts(case)
    torch.cuda.synchronize()
    s = C.c_void_p(st.cuda_stream)
    assert L.sigax_unitigs_device(0, d_edges.data_ptr(), ne, d_len.data_ptr(), d_seqs.data_ptr(), d_offs.data_ptr(), n, case["m"],
                                  plain["so"].data_ptr(), plain["lo"].data_ptr(), plain["uf"].data_ptr(), plain["lay"].data_ptr(),
                                  plain["us"].data_ptr(), plain["st"].data_ptr(), plain["w"].data_ptr(), wb0.value, s) == 0, _lib.last_error()
    assert L.sigax_unitigs_indel_device(0, d_edges.data_ptr(), ne, d_len.data_ptr(), d_seqs.data_ptr(), d_offs.data_ptr(), n, case["m"],
                                        C.byref(opts), full["so"].data_ptr(), full["lo"].data_ptr(), full["uf"].data_ptr(), full["lay"].data_ptr(),
                                        full["us"].data_ptr(), full["rm"].data_ptr(), full["ct"].data_ptr(), full["ue"].data_ptr(),
                                        full["st"].data_ptr(), full["w"].data_ptr(), wb.value, s) == 0, _lib.last_error()
    st.synchronize()
    exp = ic.expected_of("three_bubble_pops")
    assert full["st"].cpu().numpy()[:256].view(np.uint64).tolist() == exp["status"]
    assert full["rm"].cpu().numpy()[:4 * n].view(np.uint32).tolist() == exp["removed"]
    assert int(plain["st"].cpu().numpy()[:8].view(np.uint64)[0]) == uc.expected(case["reads"], case["edges"], case["m"])["status"][0]


def test_hostile_tables():
    """records and offsets that hold anything: the call returns, and nothing outside the buffers is written"""
    case = ic.case_named("three_bubble_keeps")
    edges, lengths, seqs, offs = uc.arrays(case)
    rng = np.random.default_rng(3)
    n = len(lengths)
    for kind in range(3):
        e, of = edges.copy(), offs.copy()
        raw = e.view(np.uint32).reshape(-1, 4)
        if kind == 0:  # read ids out of range, lengths beyond the reads, flags that are none
            raw[::3, 0] = rng.integers(n, 2 ** 32, size=len(raw[::3]), dtype=np.uint64).astype(np.uint32)
            raw[1::3, 2] = 0xFFFFFFF0
            raw[2::3, 3] = 9
        elif kind == 1:  # every record between two random read ends, with the overlap it had
            raw[:, 0] = rng.integers(0, n, size=len(raw))
            raw[:, 1] = rng.integers(0, n, size=len(raw))
        else:  # offsets far beyond the bases, and not ascending (the last one still names the end of the bases)
            of[1:-1] = rng.integers(0, 2 ** 40, size=n - 1, dtype=np.uint64)
        res, tails = _device_call(case, arrays=(e, lengths, seqs, of))
        _untouched(tails, "hostile %d" % kind)
        assert int(res["status"][0]) <= n and int(res["status"][9]) <= n


def test_refusals():
    from siga_amd import _lib
    L = _lib.lib()
    E = _lib.SIGAX_E_ARG
    wb = C.c_uint64()
    assert L.sigax_unitigs_indel_workspace(1 << 31, 0, 1, 0, C.byref(wb)) == E
    assert L.sigax_unitigs_indel_workspace(10, (1 << 32) + 1, 1, 0, C.byref(wb)) == E
    assert L.sigax_unitigs_indel_workspace(10, 100, 1, 0, None) == E
    assert L.sigax_unitigs_indel_workspace(10, 100, 1, 0, C.byref(wb)) == 0
    mine = wb.value
    # the bubble call's scratch, the counters and 4 bytes per read, each piece rounded up to 16 bytes
    assert L.sigax_unitigs_bubble_workspace(10, 100, 1, 0, C.byref(wb)) == 0 and mine == wb.value + 33408 + 48
    z = None

    def opts(**over):
        o = dict(max_rounds=10, min_branch_length=150, min_branch_coverage=_lib.SIGAX_TRIM_NO_COVERAGE, delta=0, careful=0, reserved=0,
                 num_reads=4, genome_size=0, uniq_threshold=13.0, min_chimeric_length=0, min_chimeric_coverage=_lib.SIGAX_TRIM_NO_COVERAGE,
                 chimeric_delta=0, reserved2=0, chimeric_threshold=0.0, max_bubble_span=40, max_divergence_permille=50, r0=0, r1=0, max_edits=2,
                 max_edit_permille=50, r2=0, r3=0)
        o.update(over)
        prune = _lib.PruneOpts(*[o[k] for k, _ in _lib.PruneOpts._fields_])
        chim = _lib.ChimericOpts(prune, *[o[k] for k, _ in _lib.ChimericOpts._fields_[1:]])
        bub = _lib.BubbleOpts(chim, o["max_bubble_span"], o["max_divergence_permille"], (C.c_uint32 * 2)(o["r0"], o["r1"]))
        return C.byref(_lib.IndelOpts(bub, o["max_edits"], o["max_edit_permille"], (C.c_uint32 * 2)(o["r2"], o["r3"])))

    dev = lambda n, ne, o, *b: L.sigax_unitigs_indel_device(0, b[0], ne, b[1], b[2], b[3], n, 20, o, *b[4:])  # noqa: E731
    nothing = [z] * 14 + [0, z]
    assert dev(0, 0, opts(), *nothing) == 0  # n_reads == 0; the step needs neither G nor N
    assert dev(0, 0, None, *nothing) == E and "indel options" in _lib.last_error()
    assert dev(0, 0, opts(r2=1), *nothing) == E and "reserved4" in _lib.last_error()
    assert dev(0, 0, opts(r3=1), *nothing) == E and "reserved4" in _lib.last_error()
    assert dev(0, 0, opts(r0=1), *nothing) == E and "reserved3" in _lib.last_error()
    assert dev(0, 0, opts(reserved2=1), *nothing) == E and "reserved2" in _lib.last_error()
    assert dev(0, 0, opts(reserved=1), *nothing) == E and "reserved" in _lib.last_error()
    assert dev(0, 0, opts(max_edits=32), *nothing) == E and "max_edits" in _lib.last_error()
    assert dev(0, 0, opts(max_edits=31), *nothing) == 0
    assert dev(0, 0, opts(max_bubble_span=0), *nothing) == E and "max_bubble_span" in _lib.last_error()
    assert dev(0, 0, opts(max_bubble_span=4097), *nothing) == E and "max_bubble_span" in _lib.last_error()
    assert dev(0, 0, opts(max_bubble_span=4096), *nothing) == 0
    assert dev(0, 0, opts(max_bubble_span=4097, max_edits=0), *nothing) == 0  # (without the step the bubble call's limits hold)
    assert dev(0, 0, opts(max_bubble_span=0, max_edits=0), *nothing) == 0
    assert dev(0, 0, opts(careful=2), *nothing) == E
    assert dev(0, 0, opts(min_chimeric_length=100), *nothing) == E and "genome_size" in _lib.last_error()
    assert dev(0, 0, opts(delta=10), *nothing) == E and "genome_size" in _lib.last_error()
    assert dev(0, 0, opts(max_rounds=65), *nothing) == E and "max_rounds" in _lib.last_error()
    assert dev(4, 0, opts(num_reads=3), *nothing) == E and "num_reads" in _lib.last_error()
    assert dev(4, 0, opts(), *nothing) == E  # NULL buffers
    n, ne = 4, 2
    assert L.sigax_unitigs_indel_workspace(n, ne, 1, 1, C.byref(wb)) == 0
    b = [torch.zeros(4096, dtype=torch.uint8, device="cuda:0") for _ in range(14)]
    p = [t.data_ptr() for t in b]
    work = torch.zeros(wb.value, dtype=torch.uint8, device="cuda:0")

    def args(w, nbytes, o=None, **over):
        a = {"edges": p[11], "len": p[0], "seqs": p[1], "offs": p[2], "so": p[3], "lo": p[4], "uf": p[5], "lay": p[6], "us": p[7], "rm": p[8],
             "ct": p[12], "ue": p[9], "st": p[10]}
        a.update(over)
        return (n, ne, o or opts(careful=1), a["edges"], a["len"], a["seqs"], a["offs"], a["so"], a["lo"], a["uf"], a["lay"], a["us"], a["rm"],
                a["ct"], a["ue"], a["st"], w, nbytes, z)

    assert dev(*args(work.data_ptr(), wb.value - 1)) == E and "workspace" in _lib.last_error() and "sigax_unitigs_indel_workspace" in _lib.last_error()
    assert dev(*args(z, wb.value)) == E
    assert dev(*args(work.data_ptr(), wb.value, seqs=z)) == E
    assert dev(*args(work.data_ptr(), wb.value, ct=z)) == E
    assert dev(*args(work.data_ptr(), wb.value, ct=p[12] + 2)) == E and "d_cut" in _lib.last_error()
    assert dev(*args(work.data_ptr(), wb.value, rm=z)) == E
    assert dev(*args(work.data_ptr(), wb.value, st=z)) == E
    assert dev(*args(work.data_ptr(), wb.value, st=p[10] + 4)) == E
    assert dev(*args(work.data_ptr(), wb.value, ue=p[9] + 8)) == E and "aligned" in _lib.last_error()
    assert dev(*args(work.data_ptr(), wb.value)) == 0, _lib.last_error()  # (lengths, offsets and records all zero: every record malformed)
    assert dev(*args(work.data_ptr(), wb.value, ue=z, us=z, o=opts(max_edits=0, max_bubble_span=0))) == 0, _lib.last_error()
    torch.cuda.synchronize()
    nu = C.c_uint64()
    v = [C.c_void_p() for _ in range(8)]
    st = (C.c_uint64 * 32)()
    host = lambda nr, o, pn, ps: L.sigax_unitigs_indel_host(0, z, 0, z, z, z, nr, 20, o, pn, *[C.byref(x) for x in v], ps)  # noqa: E731
    assert host(0, opts(), C.byref(nu), st) == 0 and nu.value == 0 and list(st) == [0] * 32
    for x in v:
        L.sigax_free(x)
    assert host(0, opts(), None, st) == E
    assert host(0, opts(), C.byref(nu), None) == E
    assert host(0, None, C.byref(nu), st) == E
    assert host(0, opts(r2=7), C.byref(nu), st) == E
    assert host(0, opts(max_edits=40), C.byref(nu), st) == E
    assert host(0, opts(max_bubble_span=5000), C.byref(nu), st) == E
    assert host(3, opts(num_reads=2), C.byref(nu), st) == E
    assert host(3, opts(), C.byref(nu), st) == E  # NULL buffers


def test_no_reads_and_wrapper_refusals():
    import siga_amd
    none = np.zeros(0, dtype=np.uint32)
    res = siga_amd.unitigs_indel(np.zeros(0, dtype=uc.EDGE_DTYPE), none, b"", np.zeros(1, dtype=np.uint64), 20, 10, 150, max_bubble_span=40, max_edits=3)
    assert res["status"].tolist() == [0] * 32 and len(res["cut"]) == 0 and len(res["removed"]) == 0 and len(res["layout"]) == 0
    with pytest.raises(siga_amd.SigaxError, match="max_bubble_span"):
        siga_amd.unitigs_indel(np.zeros(0, dtype=uc.EDGE_DTYPE), none, b"", np.zeros(1, dtype=np.uint64), 20, 10, 150, max_edits=3)
    with pytest.raises(siga_amd.SigaxError, match="max_edits"):
        siga_amd.unitigs_indel(np.zeros(0, dtype=uc.EDGE_DTYPE), none, b"", np.zeros(1, dtype=np.uint64), 20, 10, 150, max_bubble_span=40, max_edits=32)


# ---- end to end: the edge records of a GPU overlap run over reads of two haplotypes ----
def _e2e_files():
    d = os.path.join(CACHE, "unitig_indel_e2e")
    os.makedirs(d, exist_ok=True)
    prefix = os.path.join(d, "reads")
    names, reads = ic.end_to_end()
    if not all(os.path.exists(prefix + e) for e in (".bwt", ".rbwt", ".sai", ".rsai", ".fa")):
        seqs = [s.decode() for s in reads]
        po.Index.build(seqs).save(prefix + ".bwt", prefix + ".sai")
        po.Index.build(seqs, reverse=True).save(prefix + ".rbwt", prefix + ".rsai")
        with open(prefix + ".fa", "w") as f:
            f.write(mr.fasta_text(list(zip(names, seqs))))
    return prefix


@functools.lru_cache(maxsize=None)
def _e2e_run():
    """-> (edges of the GPU overlap run, the wrapper's result on them, expected_indel() on them, the result without --bubble-edits)"""
    import siga_amd
    names, reads = ic.end_to_end()
    prefix = _e2e_files()
    pair = siga_amd.FMIndexPair.load(prefix, device=0, with_sai=True, resident=False)
    try:
        lengths = np.array([len(s) for s in reads], dtype=np.uint32)
        pair.set_reads(lengths, siga_amd.overlap.name_ranks(names))
        edges = siga_amd.OverlapBuilder(pair, prefix).overlap(reads, ic.E2E_M, edges=True)["edges"]
    finally:
        pair.close()
    offs = np.zeros(len(reads) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum(lengths, dtype=np.uint64)
    kw = dict(max_bubble_span=ic.E2E_LB, bubble_divergence=ic.E2E_D)
    res = siga_amd.unitigs_indel(edges, lengths, b"".join(reads), offs, ic.E2E_M, ic.E2E_X, ic.E2E_L, max_edits=ic.E2E_ED, edit_permille=ic.E2E_DE, **kw)
    plain = siga_amd.unitigs_bubble(edges, lengths, b"".join(reads), offs, ic.E2E_M, ic.E2E_X, ic.E2E_L, **kw)
    recs = [tuple(int(x) for x in e) for e in edges.tolist()]
    exp = ic.expected_indel(reads, recs, ic.E2E_M, ic.E2E_X, ic.E2E_L, None, Lb=ic.E2E_LB, D=ic.E2E_D, Ed=ic.E2E_ED, De=ic.E2E_DE)
    return edges, res, exp, plain


def test_end_to_end():
    edges, res, exp, plain = _e2e_run()
    _, reads = ic.end_to_end()
    assert len(edges) > len(reads) // 2
    _same(res, exp, "end to end")
    print("indel arms popped", exp["status"][24], "unitigs with --bubble-edits", exp["status"][0], "without", int(plain["status"][0]))
    # four indel sites: arms go, and fewer unitigs are left than with the bubble step alone
    assert exp["status"][24] >= 1 and exp["status"][0] < int(plain["status"][0])


def test_cli(tmp_path):
    import subprocess

    from siga_amd import host
    prefix = _e2e_files()
    edges, res, _, _ = _e2e_run()
    names, _ = ic.end_to_end()
    plain = {"uflags": res["uflags"], "lay_offs": res["lay_offs"], "seq_offs": res["seq_offs"], "useqs": res["useqs"].tobytes(),
             "layout": res["layout"].tolist()}
    want_fa, _ = uc.render(names, plain)
    flags = np.uint32(bc.BUBBLE | ic.INDEL)
    want_removed = tc.render_removed(names, res["removed"] & ~flags)
    want_bubbles = "".join("%s\t%d\n" % (names[r], int(x) & ~bc.BUBBLE) for r, x in enumerate(res["removed"]) if int(x) & bc.BUBBLE)
    want_bubbles += "".join("%s\t%d\tindel\n" % (names[r], int(x) & ~ic.INDEL) for r, x in enumerate(res["removed"]) if int(x) & ic.INDEL)
    assert want_bubbles.count("\tindel\n") == int(res["status"][25]) > 0
    fa, rm, bu = (str(tmp_path / f) for f in ("u.fa", "u.removed", "u.bubbles"))
    base = [host.CLI_PATH, "unitig", "-m", str(ic.E2E_M), "-p", prefix]
    tail = ["-x", str(ic.E2E_X), "-n", str(ic.E2E_L), "-b", str(ic.E2E_LB), "--bubble-divergence", str(ic.E2E_D)]
    r = subprocess.run(base + tail + ["--bubble-edits", str(ic.E2E_ED), "--bubble-edit-permille", str(ic.E2E_DE), "-o", fa, "--removed", rm,
                                      "--bubbles", bu, prefix + ".fa"], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    assert open(fa).read() == want_fa and open(rm).read() == want_removed and open(bu).read() == want_bubbles
    assert ("%d indel arms popped, %d reads, %d kept on edits, %d not compared" % tuple(int(x) for x in res["status"][[24, 25, 27, 28]])).encode() in r.stderr
    assert b"bubble arms popped" in r.stderr
    # the wrapper of the host library: the counts of the library call
    st = host.unitig_file(prefix + ".fa", prefix, ic.E2E_M, out=fa, cut_terminal=ic.E2E_X, min_branch_length=ic.E2E_L, max_bubble_span=ic.E2E_LB,
                          bubble_divergence=ic.E2E_D, bubbles=bu, bubble_edits=ic.E2E_ED, bubble_edit_permille=ic.E2E_DE)
    assert open(fa).read() == want_fa and open(bu).read() == want_bubbles
    assert (st["indels_popped"], st["indel_reads"], st["indels_kept"], st["indels_not_compared"]) == tuple(int(x) for x in res["status"][[24, 25, 27, 28]])
    assert (st["bubbles_popped"], st["bubble_reads"]) == tuple(int(x) for x in res["status"][[20, 21]])
    # the default of --bubble-edit-permille is 50
    r = subprocess.run(base + tail + ["--bubble-edits=%d" % ic.E2E_ED, "-o", fa, "--bubbles=" + bu, prefix + ".fa"], capture_output=True)
    assert r.returncode == 0 and b"indel arms popped" in r.stderr
    # without --bubble-edits no line of the new kind and no new summary line
    r = subprocess.run(base + tail + ["-o", fa, "--bubbles", bu, prefix + ".fa"], capture_output=True)
    assert r.returncode == 0 and b"indel" not in r.stderr and "indel" not in open(bu).read()
    # the refusals
    r = subprocess.run(base + ["-x", "10", "--bubble-edits", "2", "-o", fa, prefix + ".fa"], capture_output=True)
    assert r.returncode == 1 and b"--max-bubble-span" in r.stderr
    r = subprocess.run(base + ["-x", "10", "-b", "4097", "--bubble-edits", "2", "-o", fa, prefix + ".fa"], capture_output=True)
    assert r.returncode == 1 and b"4096" in r.stderr
    r = subprocess.run(base + ["-x", "10", "-b", "40", "--bubble-edits", "32", "-o", fa, prefix + ".fa"], capture_output=True)
    assert r.returncode == 1 and b"--bubble-edits needs a number from 0 to 31" in r.stderr
    r = subprocess.run(base + ["-x", "10", "-b", "40", "--bubble-edit-permille", "5", "-o", fa, prefix + ".fa"], capture_output=True)
    assert r.returncode == 1 and b"--bubble-edits" in r.stderr
    r = subprocess.run(base, capture_output=True)  # no READSFILE: the help text
    assert r.returncode == 0 and all(w in r.stdout for w in (b"--bubble-edits=E", b"--bubble-edit-permille=M"))
