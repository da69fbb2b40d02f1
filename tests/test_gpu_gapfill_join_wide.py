"""`siga unitig --scaffold --gapfill` and `--join-overlaps` with more than 2^32 bases (csrc/sigax_gapfill.hip, csrc/sigax_join.hip):
the device forms only.

A small case runs behind ballast of random bases made on the device (tests/lift_cases.py: ballast scaffolds in front, a joined
pair and a reverse-placed unitig among them, or the case's first unitig grown beyond 2^32 bases), so that its offsets, its
sources and its status carry a high word.  The index holds the small case's reads only.  The expected tables, records and status
are the small case's, shifted by the rule tests/test_lift_cases.py holds against the restatements; the bases are compared where
they lie, on the device: ballast stretches against the input slice they come from, N runs against N, the case's scaffolds
against the restatement's bytes, and everything behind them against the 0xEE the buffers were filled with.  All comparisons are
exact."""
import numpy as np
import pytest
import torch  # before the library loads: one HIP runtime per process

from tests import gapfill_cases as gc
from tests import join_cases as jc
from tests import lift_cases as lc
from tests.test_gpu_unitig_wide import CANARY, CHUNK, _all_ee, _equal_revcomp, _fill_acgt, _release, _require, _up

pytestmark = pytest.mark.gpu
G31, G32 = 1 << 31, 1 << 32
STEP = 1 << 30  # bytes per comparison

# The ballast shapes.  The lengths follow from what each must straddle:
#  a   one unitig of 2^32 - 37 bases in front: the case's first scaffold begins below 2^32 and ends above it
#  a_cut  join: 2^32 - 110 bases in front of three_joins_in_a_row: the 28 bytes its first join deletes lie at 2^32 - 8 .. 2^32 + 20,
#      so the 16-byte pieces whose sources jump by 28 to addresses that are not aligned lie on either side of 2^32
#  b   2^32 + 2^31 + 17 bases in three unitigs: everything of the case beyond 2^32, odd-aligned; scaffold and placement numbers shifted
#  c   join: a joined ballast gap, more than 2 GiB copied with shift 1005 from sources that are not aligned, the case behind it
#      gapfill: a ballast unitig placed reversed, copied mirrored and complemented from beyond 2^31, behind a gap that stays
#  d   the case's first unitig 2^32 + 31 bases longer: its gap's sources, the next placement's offset and its scaffold's length
#      carry a high word; d_rev: the same with the unitig stored the other way round, the ballast behind its bytes in useqs
JOIN_WIDE = {"a": dict(front=[G32 - 37]), "a_cut": dict(front=[G32 - 110]), "b": dict(front=[G31 + 5, G31 + 11, G31 + 1]), "c": dict(front=[(G31 + 5, G31 + 11, 1000, 5)]),
             "d": dict(grow=G32 + 31)}
GAPFILL_WIDE = {"a": dict(front=[G32 - 37]), "b": dict(front=[G31 + 5, G31 + 11, G31 + 1]), "c_rev": dict(front=[(G31 + 5, G31 + 11, 40, True)]),
                "d": dict(grow=G32 + 31), "d_rev": dict(grow_rev=G32 + 31)}
BLOCKS = {"join": dict(status=128, gaps=0, S=15, records="joins"), "gapfill": dict(status=192, gaps=0, S=22, records="gaps")}  # bytes, entries


@pytest.fixture(autouse=True)
def _nothing_held():
    _release()
    yield
    torch.cuda.empty_cache()


def _tg():
    from tests import test_gpu_gapfill as tg
    return tg


def _tj():
    from tests import test_gpu_join as tj
    return tj


def _materialise(plan, buf, seed, done):
    """the plan's bytes into buf; a ballast piece that an earlier plan left at the same place stays (done: those pieces)"""
    at = 0
    for i, p in enumerate(plan):
        n = lc.plan_bytes([p])
        if p[0] == "bytes":
            if n:
                buf[at:at + n] = _up(p[1])[:n]
        elif (at,) + p not in done:
            if p[0] == "rand":
                _fill_acgt(buf[at:at + n], seed + i)
            elif p[0] == "N":
                buf[at:at + n] = ord("N")
            else:
                buf[at:at + n] = buf[p[1]:p[1] + n].clone()
            done.add((at,) + p)
        at += n
    return at


def _equal(a, b):
    if a.numel() != b.numel():
        return False
    return all(torch.equal(a[at:at + STEP], b[at:at + STEP]) for at in range(0, a.numel(), STEP))


def _check_bases(out, total, plan, inp, what):
    at = 0
    for p in plan:
        n = lc.plan_bytes([p])
        got = out[at:at + n]
        where = "%s: output bytes [%d, %d), %s" % (what, at, at + n, p[0])
        if p[0] == "in":
            assert _equal(got, inp[p[1]:p[1] + n]), where
        elif p[0] == "inrc":
            assert _equal_revcomp(got, inp[p[1]:p[1] + n]), where
        elif p[0] == "N":
            assert n and int(got.min()) == ord("N") and int(got.max()) == ord("N"), where
        else:
            assert got.cpu().numpy().tobytes() == p[1], where
        at += n
    assert at == total and out.numel() == total + CANARY and _all_ee(out[total:]), "%s: bytes behind the bases were written" % what


def _tables_back(d, sizes, block, what):
    """the small tables on the host, and that nothing behind their entries was written; the bases stay on the device"""
    from siga_amd import _lib
    B = BLOCKS[block]
    h = {k: v.cpu().numpy() for k, v in d.items() if k not in ("seqs", "work")}
    status = h["status"][:B["status"]].view(np.uint64).tolist()
    ng, s = status[B["gaps"]], status[B["S"]]
    lay = h["layout"][:sizes["layout"]].view(_lib.PLACEMENT_DTYPE)
    placed = len(lay)
    while placed and h["layout"][16 * (placed - 1):16 * placed].tobytes() == b"\xee" * 16:
        placed -= 1
    rec = B["records"]
    used = {"sc_offs": 8 * (s + 1), "layout": 16 * placed, rec: 32 * ng, "status": B["status"]}
    for k, v in used.items():
        rest = h[k][v:].tobytes()
        assert len(rest) >= CANARY and rest == b"\xee" * len(rest), "%s: bytes after %s were written" % (what, k)
    assert _all_ee(d["work"][sizes["work"]:]), what
    dt = _lib.JOIN_DTYPE if block == "join" else _lib.GAP_DTYPE
    return {"status": status, "sc_offs": h["sc_offs"][:8 * (s + 1)].view(np.uint64).tolist(),
            "layout": [tuple(int(x) for x in p) for p in lay[:placed].tolist()],
            rec: [tuple(int(x) for x in g) for g in h[rec][:32 * ng].view(dt).tolist()]}


def _same_tables(got, want, block, what):
    B = BLOCKS[block]
    print(what, "status", got["status"], "expected", want["status"])
    skip = (19,) if block == "gapfill" else ()  # rank-table sectors: a diagnostic
    assert [x for i, x in enumerate(got["status"]) if i not in skip] == [x for i, x in enumerate(want["status"]) if i not in skip], what
    for k in ("sc_offs", "layout", B["records"]):
        assert got[k] == want[k], "%s: %s" % (what, k)


def _device_tables(lf, mu):
    from siga_amd import _lib
    tj = _tj()
    scaf = lf["scaf"]
    lay = np.zeros(mu, dtype=_lib.PLACEMENT_DTYPE)
    for i, p in enumerate(scaf["layout"]):
        lay[i] = tuple(p)
    t = {"counts": _up(np.array([mu, len(scaf["sc_lay_offs"]) - 1], dtype=np.uint64)), "so": _up(np.array(lf["res"]["seq_offs"], dtype=np.uint64)),
         "slo": _up(tj._padded(scaf["sc_lay_offs"], mu + 1, np.uint64)), "lay": _up(lay)}
    if "sc_offs" in scaf:
        t["sco"] = _up(tj._padded(scaf["sc_offs"], mu + 1, np.uint64))
    return t


def small_off1(c):
    """the offset of the second placement of the small case's first scaffold, as laid"""
    return c["scaf"]["layout"][1][2]


# ---- join ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(JOIN_WIDE))
def test_join_behind_ballast(shape):
    from siga_amd import _lib
    tj = _tj()
    L = _lib.lib()
    torch.cuda.reset_peak_memory_stats()
    cases = [lc.join_small(w) for w in ("three", "random")]
    smalls = [jc.case_expected(c) for c in cases]
    lifts = [lc.lift_join(c["res"], c["scaf"], c["opts"], **JOIN_WIDE[shape]) for c in cases]
    wants = [lc.shifted_join(e, lf) for e, lf in zip(smalls, lifts)]
    nin = max(lf["scaf"]["sc_offs"][-1] for lf in lifts)
    _require(nin + max(w["status"][11] for w in wants) + 32 * CHUNK)
    buf = torch.empty(nin, dtype=torch.uint8, device="cuda:0")
    done = set()
    for c, small, lf, want in zip(cases, smalls, lifts, wants):
        what = "%s behind %s" % (c["name"], shape)
        nbytes = _materialise(lf["scaf"]["seqs_plan"], buf, 500 + ord(shape[0]) + len(shape), done)
        assert nbytes == lf["scaf"]["sc_offs"][-1]
        o, total = lf["opts"], want["status"][11]
        for g in lf["gaps"]:  # the ballast's overlap is the only match: the expectation does not rest on chance
            a, b = g["at"] + g["lu"], g["at"] + g["lu"] + g["G"]
            tail, head = buf[a - 4096:a].cpu().numpy().tobytes(), buf[b:b + 4096].cpu().numpy().tobytes()
            assert head[:g["v"]] == tail[-g["v"]:] and buf[a:b].cpu().numpy().tobytes() == b"N" * g["G"]
            assert jc.matches_of(tail, head, o["min_overlap"], min(o["max_overlap"], 4095)) == [g["v"]] and o["max_overlap"] <= 4096
        mu = len(lf["res"]["seq_offs"]) - 1
        t = _device_tables(lf, mu)
        ix = tj._open(c["reads"], False)
        try:
            for cap in (total, total - 1) if shape == "a" and c is cases[0] else (total,):
                d, sizes = tj._enqueue(L, ix, mu, t["counts"].data_ptr(), t["so"].data_ptr(), t["counts"].data_ptr() + 8, t["sco"].data_ptr(),
                                       t["slo"].data_ptr(), t["lay"].data_ptr(), buf.data_ptr(), nbytes, o, cap, None)
                torch.cuda.synchronize()
                got = _tables_back(d, sizes, "join", what)
                _same_tables(got, lc.shifted_join(small, lf, capacity=cap), "join", "%s, capacity %d" % (what, cap))
                if cap < total:
                    assert got["status"][14] == 1 and _all_ee(d["seqs"]), "capacity one short, and bases were written"
                else:
                    _check_bases(d["seqs"], total, want["seqs_plan"], buf, what)
                    assert want["case_at"] + len(small["seqs"]) == total
                d.clear()
                torch.cuda.empty_cache()
        finally:
            ix.close()
        # what the shape is for
        kb, sb = lf["kb"], lf["sb"]
        if shape == "a":
            assert lf["scaf"]["sc_offs"][sb] < G32 < lf["scaf"]["sc_offs"][sb + 1] and want["sc_offs"][sb] < G32 < want["sc_offs"][sb + 1]
        if shape == "a_cut" and c is cases[0]:  # the old bytes the first join deletes: [offset[1] - G, offset[1] + v) of the scaffold
            at, (_, _, _, G, v) = lf["scaf"]["sc_offs"][sb], small["joins"][0][:5]
            first, last = at + small_off1(c) - G, at + small_off1(c) + v
            assert small["joins"][0][5] == jc.C["JOINED"] and first < G32 < last and (first, last) == (G32 - 8, G32 + 20)
        if shape == "b":
            assert want["sc_offs"][sb] == G32 + G31 + 17 and want["joins"][0][:3] == tuple(x + 3 for x in small["joins"][0][:3])
        if shape == "c":
            assert want["joins"][0] == (0, 0, 1, 5, 1000, jc.C["JOINED"], 1, 0, G31 + 5 - 1000) and want["sc_offs"][1] == G32 + 16 - 1000
            assert want["layout"][1] == (1, 0, G31 + 5 - 1000) and want["status"][9] == small["status"][9] + 1000
        if shape == "d":
            assert want["sc_offs"][1] > G32 and lf["dhi"] == 0
            if c is cases[0]:  # the first scaffold has a gap: its record and the placement behind it
                assert want["layout"][1][2] > G32 and want["joins"][0][8] > G32 and want["joins"][0][5] == jc.C["JOINED"]
        print(what, "peak device memory", torch.cuda.max_memory_allocated())
    del buf


# ---- gapfill ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(GAPFILL_WIDE))
def test_gapfill_behind_ballast(shape):
    from siga_amd import _lib
    tg = _tg()
    L = _lib.lib()
    torch.cuda.reset_peak_memory_stats()
    c = lc.gapfill_small(shape == "d_rev")
    mw = gc.scratch_needed(c)
    small = gc.expected_gapfill(c["reads"], c["res"], c["scaf"], c["opts"], max_walk_bases=mw)
    lf = lc.lift_gapfill(c["res"], c["scaf"], c["opts"], max_walk_bases=mw, **GAPFILL_WIDE[shape])
    want = lc.shifted_gapfill(small, lf)
    what = "%s behind %s" % (c["name"], shape)
    nin, total = lf["res"]["seq_offs"][-1], want["status"][16]
    _require(nin + total + 32 * CHUNK)
    useqs = torch.empty(nin, dtype=torch.uint8, device="cuda:0")
    assert _materialise(lf["res"]["useqs_plan"], useqs, 700 + ord(shape[0]) + len(shape), set()) == nin
    o, k = lf["opts"], lf["opts"]["k"]
    for g in lf["gaps"]:  # no read holds a k-mer that extends the ballast's ends: DEAD_END does not rest on chance
        a = g["at"] + g["lu"]
        tail = useqs[a - k:a].cpu().numpy().tobytes()
        head = gc.revcomp(useqs[a + g["lv"] - k:a + g["lv"]].cpu().numpy().tobytes()) if g["rev"] else useqs[a:a + k].cpu().numpy().tobytes()
        for src in (tail, gc.revcomp(head)):
            assert all(gc.kmer_count(c["reads"], k, src[1:] + bytes([b])) == 0 for b in b"ACGT")
    mu = len(lf["res"]["seq_offs"]) - 1
    t = _device_tables(lf, mu)
    ix = tg._open(c["reads"], False)
    try:
        for cap in (total, total - 1) if shape == "a" else (total,):
            d, sizes = tg._enqueue(L, ix, mu, t["counts"].data_ptr(), t["so"].data_ptr(), useqs.data_ptr(), nin, t["counts"].data_ptr() + 8,
                                   t["slo"].data_ptr(), t["lay"].data_ptr(), o, cap, lf["max_walk_bases"], None)
            torch.cuda.synchronize()
            got = _tables_back(d, sizes, "gapfill", what)
            _same_tables(got, lc.shifted_gapfill(small, lf, capacity=cap), "gapfill", "%s, capacity %d" % (what, cap))
            assert got["status"][19] > 0
            if cap < total:
                assert got["status"][20] == 1 and _all_ee(d["seqs"]), "capacity one short, and bases were written"
            else:
                _check_bases(d["seqs"], total, want["seqs_plan"], useqs, what)
                assert want["case_at"] + len(small["seqs"]) == total
            d.clear()
            torch.cuda.empty_cache()
    finally:
        ix.close()
    # what the shape is for
    sb = lf["sb"]
    if shape == "a":
        assert want["sc_offs"][sb] < G32 < want["sc_offs"][sb + 1]
    if shape == "b":
        assert want["sc_offs"][sb] == G32 + G31 + 17 and lf["res"]["seq_offs"][lf["kb"]] == G32 + G31 + 17
    if shape == "c_rev":
        assert want["layout"][1] == (1, gc.REV, G31 + 45) and want["gaps"][0] == (0, 0, 1, 40, 0) + (gc.C["DEAD_END"],) * 3 + (0, G31 + 5)
    if shape in ("d", "d_rev"):
        assert want["layout"][1][2] > G32 and want["sc_offs"][1] > G32 and want["gaps"][0][9] > G32
        assert ("inrc" if shape == "d_rev" else "in", lf["grow_at"], G32 + 31) in want["seqs_plan"]
    print(what, "peak device memory", torch.cuda.max_memory_allocated())
    del useqs
