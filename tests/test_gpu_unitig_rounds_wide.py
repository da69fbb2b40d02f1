"""The later steps of the unitig rounds -- cut, chimeric, bubble, indel, reduce -- with more than 2^32 bases and at the limits of their
u32 options (csrc/sigax_unitig.hip), against the serial restatements in their tables-only mode (tests/giant_cases.py; its claims are
held on the CPU by tests/test_giant_cases.py).  All comparisons are exact.

(a) a hand-built case of the step behind ballast reads on the device, through the step's own device entry with the graph on: every
    table against the restatement's, the ballast unitigs' bytes against their reads where they lie, the case's unitigs against the
    small case's bytes, everything behind against the 0xEE the buffers were filled with.
(b) unitigs of 2^32 + 101 bases that take part in a decision, layout only: the reads buffer has its full size and only the small
    reads' bytes are written into it.
(c) option values near 2^32 on small graphs, host form and device form.
The device plumbing is tests/test_gpu_unitig_wide.py's; at most one ballast is on the device at a time."""
import ctypes as C

import numpy as np
import pytest
import torch  # before the library loads: one HIP runtime per process

from tests import giant_cases as gc
from tests import test_gpu_unitig_wide as tw
from tests import unitig_cases as uc

pytestmark = pytest.mark.gpu
CANARY = tw.CANARY
G31, G32 = gc.G31, gc.G32
ENTRY = {"cut": "prune", "chimeric": "chimeric", "bubble": "bubble", "indel": "indel", "reduce": "reduce"}
assert all(tw.SHAPES[k] == v for k, v in gc.SHAPES.items()) and tw.SHAPES["d"] == [gc.GIANT]


@pytest.fixture(scope="module", autouse=True)
def _free_at_the_end():
    yield
    tw._release()


def _opts(step, case):
    from siga_amd import _lib
    none = _lib.SIGAX_TRIM_NO_COVERAGE
    prune = _lib.PruneOpts(case["x"], case["L"], none if case["C"] is None else case["C"], case["delta"], int(case["careful"]), 0, case["N"],
                           case["G"] or 0, case["T"])
    chim = _lib.ChimericOpts(prune, case["Lc"], none if case["Ac"] is None else case["Ac"], case["delta_c"], 0, case["Tc"])
    bub = _lib.BubbleOpts(chim, case["Lb"], _lib.SIGAX_BUBBLE_NO_BASES if case["D"] is None else case["D"], (C.c_uint32 * 2)(0, 0))
    ind = _lib.IndelOpts(bub, case["Ed"], case["De"], (C.c_uint32 * 2)(0, 0))
    red = _lib.ReduceOpts(ind, int(case["reduce"]), (C.c_uint32 * 3)(0, 0, 0))
    return {"cut": prune, "chimeric": chim, "bubble": bub, "indel": ind, "reduce": red}[step]


def _call(step, case, d_seqs, layout_only=False):
    """the step's device entry over reads already on the device (case["reads"]: bytes or bare lengths), the graph on.  Every output
    buffer has exactly its size plus CANARY bytes of 0xEE; the tables come to the host, the bases stay
    -> dict(status, seq_offs, lay_offs, uflags, layout, removed, cut, uedges, useqs (device, to status[1]; None layout only))"""
    from siga_amd import _lib
    L = _lib.lib()
    lengths = [uc.nbases(r) for r in case["reads"]]
    offs = [0]
    for x in lengths:
        offs.append(offs[-1] + x)
    n, ne, nb, words = len(lengths), len(case["edges"]), offs[-1], gc.STEPS[step][2]
    assert nb <= d_seqs.numel()  # no byte at or beyond offs[n] is read, and every byte below it lies in the buffer
    e = np.ascontiguousarray(np.array(case["edges"], dtype=np.uint64).astype(np.uint32).reshape(-1, 4)).view(_lib.EDGE_DTYPE).reshape(-1)
    d_edges, d_len, d_offs = tw._up(e), tw._up(np.array(lengths, dtype=np.uint32)), tw._up(np.array(offs, dtype=np.uint64))
    wb = C.c_uint64()
    assert getattr(L, "sigax_unitigs_%s_workspace" % ENTRY[step])(n, ne, 1, int(case["careful"]), C.byref(wb)) == 0
    sizes = {"seq_offs": 8 * (n + 1), "lay_offs": 8 * (n + 1), "uflags": 4 * n, "layout": 16 * n, "removed": 4 * n, "cut": 4 * ne,
             "uedges": 16 * ne, "status": 8 * words, "work": wb.value}
    if not layout_only:
        sizes["useqs"] = nb
    d = {k: tw._out(v) for k, v in sizes.items()}
    opts = _opts(step, case)
    torch.cuda.synchronize()
    p = {k: v.data_ptr() for k, v in d.items()}
    rc = getattr(L, "sigax_unitigs_%s_device" % ENTRY[step])(
        0, d_edges.data_ptr(), ne, d_len.data_ptr(), d_seqs.data_ptr(), d_offs.data_ptr(), n, case["m"], C.byref(opts), p["seq_offs"],
        p["lay_offs"], p["uflags"], p["layout"], None if layout_only else p["useqs"], p["removed"], p["cut"], p["uedges"], p["status"],
        p["work"], wb.value, None)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    h = {k: v.cpu().numpy() for k, v in d.items() if k not in ("useqs", "work")}
    status = h["status"][:8 * words].view(np.uint64).tolist()
    u, total, placed, lifted = status[0], status[1], n - status[9], status[11]
    assert u <= n and total <= nb and lifted <= ne and 0 <= placed
    used = {"seq_offs": 8 * (u + 1), "lay_offs": 8 * (u + 1), "uflags": 4 * u, "layout": 16 * placed, "removed": 4 * n, "cut": 4 * ne,
            "uedges": 16 * lifted, "status": 8 * words}
    for k, v in used.items():  # the canaries, and inside the buffers what lies beyond the entries the call had to write
        rest = h[k][v:].tobytes()
        assert len(rest) >= CANARY and rest == b"\xee" * len(rest), "bytes after %s were written" % k
    assert tw._all_ee(d["work"][sizes["work"]:]), "bytes after the workspace were written"
    if not layout_only:
        assert tw._all_ee(d["useqs"][total:]), "bytes after the unitigs' bases were written"
    return {"status": status, "seq_offs": h["seq_offs"][:used["seq_offs"]].view(np.uint64).tolist(),
            "lay_offs": h["lay_offs"][:used["lay_offs"]].view(np.uint64).tolist(), "uflags": h["uflags"][:used["uflags"]].view(np.uint32).tolist(),
            "layout": [tuple(int(x) for x in q) for q in h["layout"][:used["layout"]].view(_lib.PLACEMENT_DTYPE).tolist()],
            "removed": h["removed"][:4 * n].view(np.uint32).tolist(), "cut": h["cut"][:4 * ne].view(np.uint32).tolist(),
            "uedges": [tuple(int(x) for x in q) for q in h["uedges"][:16 * lifted].view(_lib.EDGE_DTYPE).tolist()],
            "useqs": None if layout_only else d["useqs"][:total]}


def _same_tables(res, exp, what):
    print(what, "status", res["status"], "expected", exp["status"])
    for k in gc.TABLES:
        assert res[k] == exp[k], "%s: %s" % (what, k)


# ---- (a) behind ballast: shape a first, then shape c, so that each is made once ----
BEHIND = sorted(gc.BEHIND, key=lambda b: b[2])


@pytest.mark.parametrize("step,name,shape", BEHIND, ids=["%s-%s-%s" % (s, b, n) for b, n, s in BEHIND])
def test_rounds_behind_ballast(step, name, shape):
    big, bal, exp, small = gc.behind(step, name, shape)
    held, seqs = tw._shape(shape)
    assert held.lens == bal.lens
    mine = b"".join(big["reads"][bal.k:])
    assert len(mine) <= tw.ROOM
    seqs[bal.read_bases:bal.read_bases + len(mine)] = tw._up(mine)[:len(mine)]
    res = _call(step, big, seqs)
    _same_tables(res, exp, big["name"])
    useqs, at = res["useqs"], 0
    for bases, lay in bal.units:
        tw._ballast_unit_on_device(useqs, at, lay, bal, seqs, big["name"])
        at += bases
    assert at == exp["seq_offs"][len(bal.units)] and useqs.numel() == at + len(small["useqs"])
    assert torch.equal(useqs[at:], tw._up(small["useqs"])[:len(small["useqs"])]), "%s: the case's unitigs" % big["name"]
    # what the shape is for
    if shape == "a":
        assert bal.read_offs[bal.k] < G32 < bal.read_offs[bal.k] + len(big["reads"][bal.k])  # offs of the case's first two reads
    else:
        assert exp["seq_offs"][len(bal.units)] == G32 + G31 + 1


# ---- (b) giant unitigs that take part, layout only ----
def _giant_reads(case):
    """the reads buffer at its full size, unfilled but for the small reads' bytes"""
    tw._release()
    lengths = [uc.nbases(r) for r in case["reads"]]
    tw._require(sum(lengths) + (1 << 28))
    seqs = torch.empty(sum(lengths), dtype=torch.uint8, device=tw._dev())
    k = 3 * case["giants"]
    mine = b"".join(case["reads"][k:])
    seqs[sum(lengths[:k]):] = tw._up(mine)[:len(mine)]
    return seqs


GIANT_RUNS = [(c["name"], r) for c in gc.giants() for r in ((0, 1) if c["step"] == "reduce" else (None,))]


@pytest.mark.parametrize("name,reduce", GIANT_RUNS, ids=["%s-%s" % (n, "step" if r is None else "reduce%d" % r) for n, r in GIANT_RUNS])
def test_giant_unitigs_take_part(name, reduce):
    case = gc.giant_named(name)
    exp = gc.giant_expected(name, reduce)
    if reduce is not None:
        case = dict(case, reduce=bool(reduce))
    res = _call(case["step"], case, _giant_reads(case), layout_only=True)
    _same_tables(res, exp, "%s, reduce %s" % (name, reduce))
    assert res["status"][1] > G32 and case["third"] in res["layout"]
    assert gc.decision(case, res) == case["want"]
    if reduce:
        assert res["status"][32:34] == [0, 0] and not any(x >> 31 for x in res["cut"])


# ---- (c) option values near 2^32 on small graphs ----
@pytest.mark.parametrize("name", [c["name"] for c in gc.no_wrap()])
def test_option_values_near_2_32(name):
    from tests import test_gpu_unitig_chimeric as tch
    from tests import test_gpu_unitig_trim as ttr
    case, exp = gc.no_wrap_named(name), gc.no_wrap_expected(name)
    t = ttr if case["step"] == "trim" else tch
    host = t._host(case)
    t._same(host, exp, name + ", host")
    assert bool(host["removed"][case["watch"][1]]) == case["want"]
    res, tails = t._device_call(case)
    t._same(res, exp, name + ", device")
    t._untouched(tails, name)
