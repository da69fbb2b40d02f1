"""`siga unitig`, its trimmed form and `--scaffold` with more than 2^32 bases (csrc/sigax_unitig.hip, csrc/sigax_scaffold.hip),
and the three paths of the bases pass swept.

Beyond 2^32: a hand-built case runs behind ballast reads that are slices of random bases made on the device (a joined pair
and a joined chain of three among them: tests/ballast_cases.py), so that its offsets, its sources and its status carry a high
word.  The expected tables are the small case's, shifted by the rule tests/test_ballast_cases.py holds against the restatements;
the bases are compared where they lie, on the device: a ballast unitig against its reads, the case's unitigs against the
restatement's bytes, and everything behind them against the 0xEE the buffers were filled with.

The sweep: with min_overlap 1, chains whose reads add stretches of every length 1 .. 40 and 63, 64, 65 on both strands, shifted
to every residue modulo 16 by one leading read; the same behind 0 .. 15 bytes that are not the caller's reads, the first read
stored reverse at the very start of the window; a last read that ends at, and 1 .. 15 bytes before, the end of the reads; and
chains across a scan tile and a workgroup's four windows.  All comparisons are exact."""
import ctypes as C
import functools
import random

import numpy as np
import pytest
import torch  # before the library loads: one HIP runtime per process

from tests import ballast_cases as bc
from tests import scaffold_cases as sc
from tests import trim_cases as tc
from tests import unitig_cases as uc

pytestmark = pytest.mark.gpu
CANARY = 64
G30, G31, G32 = 1 << 30, 1 << 31, 1 << 32
CHUNK = 1 << 26  # bytes per step of a lookup (its int64 indices are eight times that)
ROOM = 1 << 20  # behind the ballast, for the case's reads
REV = uc.PLACED_REV

# The ballast shapes.  The lengths follow from what each must straddle:
#  a  four reads, 2^32 - 37 bases: the case's first unitig begins below 2^32 and ends above it
#  b  2^31 + 5, 2^31 + 11, then a joined pair (2^30 + 3, 2^30 - 9, overlap 1000): the reverse read's sources lie beyond 2^32
#  c  2^32 + 2^31 + 1 bases in three reads: everything of the case beyond 2^32, odd-aligned
#  d  a joined chain of three: lengths are u32, so only a third read lies at an offset beyond 2^32 inside its unitig (the
#     high word of a placement's offset); here 2^32 + 31
SHAPES = {"a": [G30 + 5, G30 - 9, G30 + 3, G30 - 36],
          "b": [G31 + 5, G31 + 11, (G30 + 3, G30 - 9, 1000)],
          "c": [G31 + 1, G31 - 6, G31 + 6],
          "d": [(G31 + 40, G31 + 45, 70, 33, 21)]}
assert sum(SHAPES["a"]) == G32 - 37 and sum(SHAPES["c"]) == G32 + G31 + 1
WIDE = ([("a", "unitigs", n) for n in ("chain1000", "lengths", "heads", "cycle_mid", "withN", "malformed")] +
        [("a", "layout", "cycle_mid")] + [("a", "trim", n) for n in ("graph", "ring_tip", "all_removed")] +
        [("b", "unitigs", n) for n in ("chain1000", "lengths", "heads", "cycle_mid", "withN", "malformed")] +
        [("c", "unitigs", "chain65"), ("d", "unitigs", "heads")])


# ---- torch plumbing ----
def _dev():
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _luts():
    acgt = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=_dev())
    comp = np.arange(256, dtype=np.uint8)
    for a, b in zip(b"ACGT", b"TGCA"):
        comp[a] = b
    return acgt, torch.from_numpy(comp).to(_dev())


def _fill_acgt(buf, seed):
    """random bases into buf, drawn on the device and taken through the ACGT lookup"""
    g = torch.Generator(device=_dev())
    g.manual_seed(seed)
    acgt, _ = _luts()
    for at in range(0, buf.numel(), CHUNK):
        m = min(CHUNK, buf.numel() - at)
        buf[at:at + m] = acgt[torch.randint(0, 4, (m,), dtype=torch.uint8, device=_dev(), generator=g).long()]


def _revcomp(t):
    return _luts()[1][t.flip(0).long()]


def _equal_revcomp(out, src):
    """out == revcomp(src), both on the device, in steps"""
    n = src.numel()
    if out.numel() != n:
        return False
    for at in range(0, n, CHUNK):
        m = min(CHUNK, n - at)
        if not torch.equal(out[at:at + m], _revcomp(src[n - at - m:n - at])):
            return False
    return True


def _all_ee(t):
    return t.numel() == 0 or (int(t.min()) == 0xEE and int(t.max()) == 0xEE)


def _up(a):
    a = np.frombuffer(a, dtype=np.uint8) if isinstance(a, bytes) else np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return torch.from_numpy(a.copy()).to(_dev()) if a.size else torch.zeros(16, dtype=torch.uint8, device=_dev())


def _out(nbytes):
    return torch.full((nbytes + CANARY,), 0xEE, dtype=torch.uint8, device=_dev())


_HELD = {}  # the one ballast on the device: name -> (Ballast, reads buffer)


def _release():
    _HELD.clear()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module", autouse=True)
def _free_at_the_end():
    yield
    _release()


def _require(need):
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip("needs %d bytes of device memory, %d are free" % (need, free))


def _shape(name):
    """the ballast reads of a shape on the device, each a slice of one buffer of random bases; the joined reads' ends rewritten
    so that they overlap as their records say (a read stored reverse-complemented: by flip and lookup)"""
    if name not in _HELD:
        _release()
        bal = bc.Ballast(SHAPES[name])
        _require(2 * (bal.read_bases + ROOM) + 32 * CHUNK)  # the reads, the unitigs, and the steps of a lookup
        seqs = torch.empty(bal.read_bases + ROOM, dtype=torch.uint8, device=_dev())
        _fill_acgt(seqs, 1000 + ord(name))
        offs, r = bal.read_offs, 0
        for it in bal.items:
            if isinstance(it, int):
                r += 1
                continue
            lens, ovs = bc.item_chain(it)
            for i, ov in enumerate(ovs):
                x, y = r + i, r + i + 1
                if i % 2 == 0:  # x forward, y reverse: y ends with the reverse complement of x's last ov bases
                    seqs[offs[y + 1] - ov:offs[y + 1]] = _revcomp(seqs[offs[x + 1] - ov:offs[x + 1]])
                else:  # x reverse, y forward: y begins with the reverse complement of x's first ov bases
                    seqs[offs[y]:offs[y] + ov] = _revcomp(seqs[offs[x]:offs[x] + ov])
            r += len(lens)
        _HELD[name] = (bal, seqs)
    return _HELD[name]


# ---- the device forms over buffers of exactly their size ----
def _call(edges, lengths, offs, d_seqs, m, layout_only=False, trim=None):
    """sigax_unitigs_device, or sigax_unitigs_trim_device with the graph (trim = (max_rounds, L, C)), over reads already on the
    device.  Every output buffer has exactly its size plus CANARY bytes of 0xEE; the small tables come to the host, the bases stay
    -> dict(status, seq_offs, lay_offs, uflags, layout, [removed, uedges,] useqs (device, to status[1]))"""
    from siga_amd import _lib
    L = _lib.lib()
    n, ne, nb = len(lengths), len(edges), int(offs[-1]) - int(offs[0])
    e = np.ascontiguousarray(np.array(edges, dtype=np.uint64).astype(np.uint32).reshape(-1, 4)).view(_lib.EDGE_DTYPE).reshape(-1)
    d_edges, d_len, d_offs = _up(e), _up(np.array(lengths, dtype=np.uint32)), _up(np.array(offs, dtype=np.uint64))
    wb = C.c_uint64()
    sizes = {"seq_offs": 8 * (n + 1), "lay_offs": 8 * (n + 1), "uflags": 4 * n, "layout": 16 * n, "useqs": nb}
    if trim is None:
        assert L.sigax_unitigs_workspace(n, ne, C.byref(wb)) == 0
        sizes.update(status=48, work=wb.value)
    else:
        assert L.sigax_unitigs_trim_workspace(n, ne, 1, C.byref(wb)) == 0
        sizes.update(removed=4 * n, uedges=16 * ne, status=96, work=wb.value)
    d = {k: _out(v) for k, v in sizes.items()}
    torch.cuda.synchronize()
    p = {k: v.data_ptr() for k, v in d.items()}
    if trim is None:
        rc = L.sigax_unitigs_device(0, d_edges.data_ptr(), ne, d_len.data_ptr(), d_seqs.data_ptr(), d_offs.data_ptr(), n, m, p["seq_offs"],
                                    p["lay_offs"], p["uflags"], p["layout"], None if layout_only else p["useqs"], p["status"], p["work"],
                                    wb.value, None)
    else:
        opts = _lib.TrimOpts(trim[0], trim[1], _lib.SIGAX_TRIM_NO_COVERAGE if trim[2] is None else trim[2], 0)
        rc = L.sigax_unitigs_trim_device(0, d_edges.data_ptr(), ne, d_len.data_ptr(), d_seqs.data_ptr(), d_offs.data_ptr(), n, m, C.byref(opts),
                                         p["seq_offs"], p["lay_offs"], p["uflags"], p["layout"], None if layout_only else p["useqs"],
                                         p["removed"], p["uedges"], p["status"], p["work"], wb.value, None)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    h = {k: v.cpu().numpy() for k, v in d.items() if k not in ("useqs", "work")}
    status = h["status"][:sizes["status"]].view(np.uint64).tolist()
    u, total = status[0], status[1]
    placed = n - status[9] if trim else n
    lifted = status[11] if trim else 0
    assert u <= n and total <= nb and lifted <= ne
    used = {"seq_offs": 8 * (u + 1), "lay_offs": 8 * (u + 1), "uflags": 4 * u, "layout": 16 * placed, "status": sizes["status"]}
    if trim:
        used.update(removed=4 * n, uedges=16 * lifted)
    for k, v in used.items():  # the canaries, and inside the buffers what lies beyond the entries the call had to write
        rest = h[k][v:].tobytes()
        assert len(rest) >= CANARY and rest == b"\xee" * len(rest), "bytes after %s were written" % k
    assert _all_ee(d["work"][sizes["work"]:]), "bytes after the workspace were written"
    assert _all_ee(d["useqs"][0 if layout_only else total:]), "bytes after the unitigs' bases were written"
    res = {"status": status, "seq_offs": h["seq_offs"][:used["seq_offs"]].view(np.uint64).tolist(),
           "lay_offs": h["lay_offs"][:used["lay_offs"]].view(np.uint64).tolist(), "uflags": h["uflags"][:used["uflags"]].view(np.uint32).tolist(),
           "layout": [tuple(int(x) for x in q) for q in h["layout"][:used["layout"]].view(_lib.PLACEMENT_DTYPE).tolist()],
           "useqs": None if layout_only else d["useqs"][:total]}
    if trim:
        res["removed"] = h["removed"][:4 * n].view(np.uint32).tolist()
        res["uedges"] = [tuple(int(x) for x in q) for q in h["uedges"][:16 * lifted].view(_lib.EDGE_DTYPE).tolist()]
    return res


def _same_tables(res, exp, what):
    for k in ("status", "seq_offs", "lay_offs", "uflags", "layout") + (("removed", "uedges") if "removed" in exp else ()):
        assert res[k] == exp[k], "%s: %s" % (what, k)


def _same_small(res, exp, what):
    _same_tables(res, exp, what)
    assert res["useqs"].cpu().numpy().tobytes() == exp["useqs"], what


# ---- beyond 2^32 ----
@functools.lru_cache(maxsize=None)
def _uc_expected(name):
    c = next(c for c in uc.hand_built() if c["name"] == name)
    return c, uc.expected(c["reads"], c["edges"], c["m"])


def _ballast_unit_on_device(useqs, at, lay, bal, seqs, what):
    """a ballast unitig at useqs[at:] against its reads where they lie: the first whole, of every next one what it adds"""
    end = 0
    for r, fl, off in lay:
        ln, ro, skip = bal.lens[r], bal.read_offs[r], end - off
        got = useqs[at + off + skip:at + off + ln]
        if fl & REV:
            assert _equal_revcomp(got, seqs[ro:ro + ln - skip]), "%s: ballast read %d, placed reversed" % (what, r)
        else:
            assert torch.equal(got, seqs[ro + skip:ro + ln]), "%s: ballast read %d" % (what, r)
        end = off + ln


@pytest.mark.parametrize("shape,kind,name", WIDE, ids=["%s-%s-%s" % w for w in WIDE])
def test_behind_ballast(shape, kind, name):
    bal, seqs = _shape(shape)
    if kind == "trim":
        case = tc.case_named(name)
        exp = bc.shifted_trim(tc.expected_of(name), bal, case["x"], case["L"], case["C"])
        gone = exp["ballast_gone"]
    else:
        case, small = _uc_expected(name)
        exp = bc.shifted_unitigs(small, bal)
        gone = [False] * len(bal.units)
    edges, lengths, offs = bc.concat_tables(case, bal)
    mine = b"".join(case["reads"])
    assert len(mine) <= ROOM and offs[bal.k] == bal.read_bases and offs[-1] == bal.read_bases + len(mine)
    seqs[bal.read_bases:bal.read_bases + len(mine)] = _up(mine)[:len(mine)]
    what = "%s behind %s" % (name, shape)
    res = _call(edges, lengths, offs, seqs, case["m"], layout_only=kind == "layout", trim=(case["x"], case["L"], case["C"]) if kind == "trim" else None)
    print(what, "status", res["status"], "seq_offs of the case from", exp["case_at"])
    _same_tables(res, exp, what)
    if kind == "layout":
        return
    useqs, at = res["useqs"], 0
    for (bases, lay), g in zip(bal.units, gone):
        if not g:
            _ballast_unit_on_device(useqs, at, lay, bal, seqs, what)
            at += bases
    assert at == exp["case_at"] and useqs.numel() == at + len(exp["case_useqs"])
    assert torch.equal(useqs[at:], _up(exp["case_useqs"])[:len(exp["case_useqs"])]), "%s: the case's unitigs" % what
    # what the shape is for
    if shape == "a" and kind == "unitigs":
        assert exp["seq_offs"][bal.k] < G32 < exp["seq_offs"][bal.k + 1]
    if shape == "a" and kind == "trim":
        assert (name == "all_removed") == any(gone) and exp["status"][1] > (G31 if any(gone) else G32)
    if shape == "b":
        assert bal.read_offs[3] > G32 and exp["layout"][3] == (3, REV, G30 + 3 - 1000)
    if shape == "c":
        assert exp["seq_offs"][bal.k] == G32 + G31 + 1
    if shape == "d":
        assert exp["layout"][2] == (2, 0, G32 + 31) and exp["seq_offs"][1] > G32


# ---- scaffolds over unitigs beyond 2^32 ----
@pytest.mark.parametrize("name", ["cycle_and_path", "sizes_mixed"])
def test_scaffolds_behind_ballast(name):
    from siga_amd import _lib
    from tests import test_gpu_scaffold as ts
    _release()
    L = _lib.lib()
    _, res, links, o = sc.case_named(name)
    wide = dict(o, insert_size=o["insert_size"] + 1000)  # room for the ballast's gap; the case's spans rise as much, its gaps stay
    bal = bc.ScaffoldBallast([(G31 + 5, G31 + 11, 1000)], wide["insert_size"])
    lu, lv = bal.lens
    small = sc.expected_scaffolds(res, links, [0] * 24, o)
    exp = bc.shifted_scaffolds(small, bal)
    plain = {k: v for k, v in res.items() if k != "useqs"}
    big_res, big_links = bc.concat_scaffold_input(plain, bc.raise_spans(links, 1000), bal)
    direct = sc.expected_scaffolds(big_res, big_links, [0] * 24, wide)  # the restatement itself over the tables: no bases
    tables = ("sc_offs", "sc_lay_offs", "sc_flags", "layout", "status")
    for k in tables:
        assert direct[k] == exp[k], k
    assert exp["layout"][:2] == [(0, 0, 0), (1, REV, lu + 1000)] and exp["sc_offs"][1] > G32
    if name == "cycle_and_path":
        assert exp["status"][11] == 1 and exp["status"][10] >= 5 and any(fl for _, fl, _ in exp["layout"][2:])
    mu, ml, total, nbu = len(big_res["uflags"]), len(big_links), exp["status"][1], bal.bases + len(res["useqs"])
    _require(bal.bases + 2 * total + 32 * CHUNK)
    useqs = torch.empty(nbu, dtype=torch.uint8, device=_dev())
    _fill_acgt(useqs[:bal.bases], 77)
    useqs[bal.bases:] = _up(bytes(res["useqs"]))[:len(res["useqs"])]
    counts = _up(np.array([mu, ml], dtype=np.uint64))
    d_so, d_uf = _up(np.array(big_res["seq_offs"], dtype=np.uint64)), _up(np.array(big_res["uflags"], dtype=np.uint32))
    d_links, d_s24 = _up(ts._links_array(big_links)), _up(np.zeros(24, dtype=np.uint64))
    for cap in (total, total - 1):
        d, sizes = ts._enqueue(L, mu, ml, counts.data_ptr(), d_so.data_ptr(), d_uf.data_ptr(), useqs.data_ptr(), nbu, d_links.data_ptr(),
                               counts.data_ptr() + 8, d_s24.data_ptr(), wide, cap, None)
        torch.cuda.synchronize()
        h = {k: v.cpu().numpy() for k, v in d.items() if k not in ("seqs", "work")}
        status = h["status"][:128].view(np.uint64).tolist()
        s = status[0]
        used = {"sc_offs": 8 * (s + 1), "sc_lay_offs": 8 * (s + 1), "sc_flags": 4 * s, "layout": 16 * mu, "status": 128}
        for k, v in used.items():
            rest = h[k][v:].tobytes()
            assert len(rest) >= CANARY and rest == b"\xee" * len(rest), "capacity %d: bytes after %s were written" % (cap, k)
        assert _all_ee(d["work"][sizes["work"]:])
        got = {"status": status, "sc_offs": h["sc_offs"][:used["sc_offs"]].view(np.uint64).tolist(),
               "sc_lay_offs": h["sc_lay_offs"][:used["sc_lay_offs"]].view(np.uint64).tolist(), "sc_flags": h["sc_flags"][:4 * s].view(np.uint32).tolist(),
               "layout": [tuple(int(x) for x in q) for q in h["layout"][:16 * mu].view(_lib.PLACEMENT_DTYPE).tolist()]}
        want = dict(exp, status=exp["status"][:15] + [int(cap < total)])
        print(name, "capacity", cap, "status", status)
        for k in tables:
            assert got[k] == want[k], "capacity %d: %s" % (cap, k)
        ss = d["seqs"]
        if cap < total:  # no room: nothing written
            assert _all_ee(ss), "capacity one short, and bases were written"
            continue
        assert torch.equal(ss[:lu], useqs[:lu]), "the forward copy"
        assert ss[lu:lu + 1000].cpu().numpy().tobytes() == b"N" * 1000, "the gap"
        assert _equal_revcomp(ss[lu + 1000:lu + 1000 + lv], useqs[lu:lu + lv]), "the reverse-complemented copy"
        assert exp["case_at"] == lu + 1000 + lv and total - exp["case_at"] == len(small["seqs"])
        assert torch.equal(ss[exp["case_at"]:total], _up(small["seqs"])[:len(small["seqs"])]), "the case's scaffolds"
        assert _all_ee(ss[total:])
        del ss
        d.clear()
        torch.cuda.empty_cache()


# ---- the bases pass's three paths, swept ----
STRETCHES = list(range(1, 41)) + [63, 64, 65]
LEADS = list(range(16, 32))


def _bases(n, seed):
    rng = random.Random(seed)
    return bytes(rng.choice(b"ACGT") for _ in range(n))


@functools.lru_cache(maxsize=None)
def _sweep_case(lead=0, flip=False, first=48, first_rc=None, last=0):
    """min_overlap 1.  One read of `lead` bases on its own (it shifts everything behind it); a chain whose reads alternate between 2
    bases and s + 1 bases, s over STRETCHES in a fixed shuffled order -- next to a read of 2 bases _Build.chain can only draw the
    overlap 1, so a read of s + 1 bases adds exactly s -- begun by a read of `first` bases; a chain of 120 reads of 2 .. 70 bases;
    a last read of `last` bases on its own, stored forward.  Strands by a fixed pattern, all turned by `flip` (the first read of
    the first chain: first_rc, when given).  The bytes of `lead` and `last` come from generators of their own, so the chains'
    draws are the same whatever they are -> (case, expected)"""
    b = uc._Build(7000, m=1)
    if lead:
        b.read(_bases(lead, 7100 + lead))
    order = list(STRETCHES)
    random.Random(7001).shuffle(order)
    lens = [first]
    for s in order:
        lens += [2, s + 1]
    pat = random.Random(7002)
    rc = [(pat.random() < 0.5) != flip for _ in lens]
    if first_rc is not None:
        rc[0] = first_rc
    b.chain(len(lens), lens=lens, rc=rc)
    more = random.Random(7003)
    lens2 = [more.randint(2, 70) for _ in range(120)]
    b.chain(120, lens=lens2, rc=[(more.random() < 0.5) != flip for _ in lens2])
    if last:
        b.read(_bases(last, 7200 + last))
    case = b.case("sweep lead %d flip %d first %d last %d" % (lead, flip, first, last))
    return case, uc.expected(case["reads"], case["edges"], case["m"])


def _triples(case, exp):
    """(destination residue modulo 16, stretch length, placed reversed) of every stretch, from the expected layout alone"""
    out = set()
    for u in range(len(exp["uflags"])):
        end = 0
        for r, fl, off in exp["layout"][exp["lay_offs"][u]:exp["lay_offs"][u + 1]]:
            skip = end - off
            out.add(((exp["seq_offs"][u] + off + skip) % 16, len(case["reads"][r]) - skip, fl & REV))
            end = off + len(case["reads"][r])
    return out


@functools.lru_cache(maxsize=None)
def _sweep_is_complete():
    seen = set()
    for lead in LEADS:
        for flip in (False, True):
            seen |= _triples(*_sweep_case(lead, flip))
    missing = [(res, s, st) for res in range(16) for s in STRETCHES for st in (0, REV) if (res, s, st) not in seen]
    assert not missing, "the sweep lacks (residue, stretch, strand) %s" % missing[:10]
    return True


def _device_small(case, window=0):
    """the device form over the case's reads behind `window` bytes that are not the caller's reads (offs[0] = window)"""
    edges, lengths, seqs, offs = uc.arrays(case)
    d_seqs = _up(b"#" * window + seqs)
    assert d_seqs.numel() == window + len(seqs)  # the reads end where the buffer ends
    return _call(case["edges"], lengths.tolist(), [int(x) + window for x in offs], d_seqs, case["m"])


def _host_small(case, exp, what, window=0):
    import siga_amd
    edges, lengths, seqs, offs = uc.arrays(case)
    res = siga_amd.unitigs(edges, lengths, b"#" * window + seqs, offs + np.uint64(window), case["m"])
    got = {"status": res["status"].tolist(), "seq_offs": res["seq_offs"].tolist(), "lay_offs": res["lay_offs"].tolist(),
           "uflags": res["uflags"].tolist(), "layout": [tuple(int(x) for x in q) for q in res["layout"].tolist()]}
    _same_tables(got, exp, what + ", host")
    assert res["useqs"].tobytes() == exp["useqs"], what + ", host"


def test_the_sweep_holds_every_triple():
    assert _sweep_is_complete()
    # and the chain is what its docstring says: every read of s + 1 bases adds s
    case, exp = _sweep_case(16, False)
    assert {s for _, s, _ in _triples(case, exp)} >= set(STRETCHES)


@pytest.mark.parametrize("lead", LEADS)
def test_sweep(lead):
    assert _sweep_is_complete()
    for flip in (False, True):
        case, exp = _sweep_case(lead, flip)
        _same_small(_device_small(case), exp, case["name"])
        _host_small(case, exp, case["name"])


@pytest.mark.parametrize("window", range(16))
def test_sweep_in_a_window(window):
    """offs[0] = window.  The first read is stored reverse and lies at the very start of the window; its length 48 .. 63 puts the
    source of its last whole 16-byte piece 0 .. 15 bytes behind the window's start (with window 0 and 48 bases that load begins
    at byte 0 of the buffer: the lowest a reverse load may go), and shifts every stretch behind it to another residue."""
    _release()
    residues = set()
    for first in range(48, 64):
        case, exp = _sweep_case(0, (first + window) % 2 == 1, first, True)
        assert exp["layout"][0] == (0, REV, 0)
        residues |= {r for r, s, _ in _triples(case, exp) if s == 64}
        _same_small(_device_small(case, window), exp, "%s, offs[0] = %d" % (case["name"], window))
        if first in (48, 48 + window):
            _host_small(case, exp, "%s, offs[0] = %d" % (case["name"], window), window)
    assert residues == set(range(16))


def test_last_read_against_the_end_of_the_reads():
    """a last read stored forward: its final whole 16-byte piece ends exactly at offs[n] when the unitigs' bases are a multiple of
    16, and 1 .. 15 bytes before it otherwise"""
    short = set()
    for last in range(40, 56):
        case, exp = _sweep_case(16, False, last=last)
        n = len(case["reads"])
        assert exp["layout"][-1] == (n - 1, 0, 0) and exp["seq_offs"][-1] - exp["seq_offs"][-2] == last
        short.add(exp["status"][1] % 16)
        _same_small(_device_small(case), exp, case["name"])
        _host_small(case, exp, case["name"])
        _same_small(_device_small(case, 5), exp, case["name"] + ", offs[0] = 5")
    assert short == set(range(16))


@functools.lru_cache(maxsize=None)
def _long_chain(n):
    b = uc._Build(8000 + n)
    b.chain(n, rc=[b.rng.random() < 0.5 for _ in range(n)])
    case = b.case("chain%d" % n)
    return case, uc.expected(case["reads"], case["edges"], case["m"])


@pytest.mark.parametrize("n", [767, 769, 2047, 2048, 2049])
def test_chains_across_a_scan_tile_and_a_workgroup(n):
    """2048: a launch_scan tile; 4 * 64 * 3: a workgroup's four windows of 64 placements"""
    case, exp = _long_chain(n)
    assert exp["status"][0] == 1 and exp["status"][4] == n - 1
    _same_small(_device_small(case), exp, case["name"])
    _host_small(case, exp, case["name"])
