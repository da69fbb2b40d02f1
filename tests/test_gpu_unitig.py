"""`siga unitig` on the GPU (csrc/sigax_unitig.hip) against the serial restatement of its rules (tests/unitig_cases.py): every
hand-built graph through the host and the device entry point, exactly -- offsets, flags, layout, bytes, status counts; the
layout-only call; refusals and canaries; and end to end over the edge records of a GPU overlap run, through the wrapper and
the command line."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import torch  # before the library loads: one HIP runtime per process

from oracle import pyoracle as po
from tests import unitig_cases as uc
from tests.fixtures import CACHE
from tests.golden import make_reads as mr

pytestmark = pytest.mark.gpu
CASES = uc.hand_built()
IDS = [c["name"] for c in CASES]


@functools.lru_cache(maxsize=None)
def _expected(name):
    c = next(c for c in CASES if c["name"] == name)
    return uc.expected(c["reads"], c["edges"], c["m"])


def _same(res, exp, what, bases=True):
    """res: the wrapper's dict (numpy arrays); exp: expected()'s"""
    assert res["status"].tolist() == exp["status"], what
    assert res["seq_offs"].tolist() == exp["seq_offs"] and res["lay_offs"].tolist() == exp["lay_offs"], what
    assert res["uflags"].tolist() == exp["uflags"], what
    assert [tuple(int(x) for x in p) for p in res["layout"].tolist()] == exp["layout"], what
    if bases:
        assert res["useqs"].tobytes() == exp["useqs"], what


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_host_form_equals_brute_force(case):
    import siga_amd
    edges, lengths, seqs, offs = uc.arrays(case)
    exp = _expected(case["name"])
    _same(siga_amd.unitigs(edges, lengths, seqs, offs, case["m"]), exp, case["name"])
    res = siga_amd.unitigs(edges, lengths, seqs, offs, case["m"], bases=False)  # the layout-only call: the same layout
    assert res["useqs"] is None
    _same(res, exp, case["name"] + ", layout only", bases=False)


def test_host_form_takes_a_window_of_a_longer_table():
    import siga_amd
    case = next(c for c in CASES if c["name"] == "heads")
    edges, lengths, seqs, offs = uc.arrays(case)
    res = siga_amd.unitigs(edges, lengths, b"#" * 7 + seqs, offs + np.uint64(7), case["m"])
    _same(res, _expected("heads"), "offs[0] = 7")


CANARY = 64


def _device_call(case, layout_only=False):
    """sigax_unitigs_device over torch buffers, each output buffer of exactly its size plus CANARY bytes of 0xEE -> (dict like
    the wrapper's, the canaries' bytes)"""
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
    assert L.sigax_unitigs_workspace(n, ne, C.byref(wb)) == 0
    d_edges, d_len, d_seqs, d_offs = up(edges), up(lengths), up(seqs), up(offs)
    sizes = {"seq_offs": 8 * (n + 1), "lay_offs": 8 * (n + 1), "uflags": 4 * n, "layout": 16 * n, "useqs": nb, "status": 48, "work": wb.value}
    d = {k: out(v) for k, v in sizes.items()}
    torch.cuda.synchronize()
    rc = L.sigax_unitigs_device(0, d_edges.data_ptr(), ne, d_len.data_ptr(), d_seqs.data_ptr(), d_offs.data_ptr(), n, case["m"],
                                d["seq_offs"].data_ptr(), d["lay_offs"].data_ptr(), d["uflags"].data_ptr(), d["layout"].data_ptr(),
                                None if layout_only else d["useqs"].data_ptr(), d["status"].data_ptr(), d["work"].data_ptr(), wb.value, None)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize()
    h = {k: v.cpu().numpy() for k, v in d.items()}
    status = h["status"][:48].view(np.uint64)
    u = int(status[0])
    res = {"status": status, "seq_offs": h["seq_offs"][:8 * (u + 1)].view(np.uint64), "lay_offs": h["lay_offs"][:8 * (u + 1)].view(np.uint64),
           "uflags": h["uflags"][:4 * u].view(np.uint32), "layout": h["layout"][:16 * n].view(_lib.PLACEMENT_DTYPE),
           "useqs": h["useqs"][:int(status[1])]}
    tails = {k: h[k][sizes[k]:].tobytes() for k in sizes}
    # what lies beyond the entries the call wrote, inside the buffers, is the caller's too
    tails["seq_offs_rest"] = h["seq_offs"][8 * (u + 1):sizes["seq_offs"]].tobytes()
    tails["useqs_rest"] = h["useqs"][int(status[1]):nb].tobytes()
    return res, tails


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_device_form_equals_brute_force(case):
    res, tails = _device_call(case)
    _same(res, _expected(case["name"]), case["name"])
    for k, t in tails.items():
        assert t == b"\xee" * len(t), "%s: bytes after %s were written" % (case["name"], k)


def test_device_form_layout_only():
    case = next(c for c in CASES if c["name"] == "cycle_mid")
    res, tails = _device_call(case, layout_only=True)
    _same(res, _expected("cycle_mid"), "layout only", bases=False)
    assert tails["useqs"] == b"\xee" * CANARY and tails["useqs_rest"] == b"\xee" * len(tails["useqs_rest"])


def test_refusals():
    from siga_amd import _lib
    L = _lib.lib()
    wb = C.c_uint64()
    assert L.sigax_unitigs_workspace(1 << 31, 0, C.byref(wb)) == _lib.SIGAX_E_ARG
    assert L.sigax_unitigs_workspace(10, (1 << 32) + 1, C.byref(wb)) == _lib.SIGAX_E_ARG
    assert L.sigax_unitigs_workspace(10, 1 << 32, None) == _lib.SIGAX_E_ARG
    assert L.sigax_unitigs_workspace(10, 1 << 32, C.byref(wb)) == 0 and wb.value > 0
    z = None
    assert L.sigax_unitigs_device(0, z, 0, z, z, z, 0, 20, z, z, z, z, z, z, z, 0, z) == 0  # n_reads == 0
    assert L.sigax_unitigs_device(0, z, 0, z, z, z, 1 << 31, 20, z, z, z, z, z, z, z, 0, z) == _lib.SIGAX_E_ARG
    assert L.sigax_unitigs_device(0, z, (1 << 32) + 1, z, z, z, 0, 20, z, z, z, z, z, z, z, 0, z) == _lib.SIGAX_E_ARG
    assert L.sigax_unitigs_device(0, z, 0, z, z, z, 4, 20, z, z, z, z, z, z, z, 0, z) == _lib.SIGAX_E_ARG  # NULL buffers
    n = 4
    assert L.sigax_unitigs_workspace(n, 0, C.byref(wb)) == 0
    b = [torch.zeros(4096, dtype=torch.uint8, device="cuda:0") for _ in range(9)]
    p = [t.data_ptr() for t in b]
    work = torch.zeros(wb.value, dtype=torch.uint8, device="cuda:0")
    args = lambda w, nbytes: (0, z, 0, p[0], p[1], p[2], n, 20, p[3], p[4], p[5], p[6], p[7], p[8], w, nbytes, z)  # noqa: E731
    assert L.sigax_unitigs_device(*args(work.data_ptr(), wb.value - 1)) == _lib.SIGAX_E_ARG and "workspace" in _lib.last_error()
    assert L.sigax_unitigs_device(*args(z, wb.value)) == _lib.SIGAX_E_ARG
    assert L.sigax_unitigs_device(*args(work.data_ptr(), wb.value)) == 0, _lib.last_error()  # (lengths and offsets all zero)
    torch.cuda.synchronize()
    nu = C.c_uint64()
    v = [C.c_void_p() for _ in range(5)]
    assert L.sigax_unitigs_host(0, z, 0, z, z, z, 0, 20, C.byref(nu), *[C.byref(x) for x in v]) == 0 and nu.value == 0
    for x in v:
        L.sigax_free(x)
    assert L.sigax_unitigs_host(0, z, 0, z, z, z, 0, 20, None, *[C.byref(x) for x in v]) == _lib.SIGAX_E_ARG
    assert L.sigax_unitigs_host(0, z, 0, z, z, z, 3, 20, C.byref(nu), *[C.byref(x) for x in v]) == _lib.SIGAX_E_ARG


# ---- end to end: the edge records of a GPU overlap run over the 600 reads ----
def _e2e_files():
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
def _e2e_run():
    """-> (edges of the GPU overlap run, the wrapper's result on them, expected() on them)"""
    import siga_amd
    case = uc.end_to_end()
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
    res = siga_amd.unitigs(edges, lengths, b"".join(reads), offs, case["m"])
    exp = uc.expected(reads, [tuple(int(x) for x in e) for e in edges.tolist()], case["m"])
    return edges, res, exp


def test_end_to_end():
    case = uc.end_to_end()
    edges, res, exp = _e2e_run()
    assert len(edges) > 300
    _same(res, exp, "end to end")
    assert exp["status"][2] == 0 and exp["status"][3] == 0 and exp["status"][4] > 0 and 1 <= exp["status"][0] < 600
    g, rg = case["genome"], uc.revcomp(case["genome"])
    for u in range(len(exp["uflags"])):
        seq = res["useqs"][int(res["seq_offs"][u]):int(res["seq_offs"][u + 1])].tobytes()
        if not exp["uflags"][u] & uc.CIRCULAR:
            assert seq in g or seq in rg, "unitig %d is no piece of the genome" % u


def test_cli(tmp_path):
    from siga_amd import host
    case = uc.end_to_end()
    prefix = _e2e_files()
    _, res, _ = _e2e_run()
    names = [n for n, _ in case["reads"]]
    want = {"uflags": res["uflags"], "lay_offs": res["lay_offs"], "seq_offs": res["seq_offs"], "useqs": res["useqs"].tobytes(),
            "layout": res["layout"].tolist()}
    want_fa, want_lay = uc.render(names, want)
    fa, lay = str(tmp_path / "u.fa"), str(tmp_path / "u.layout")
    r = subprocess.run([host.CLI_PATH, "unitig", "-m", str(case["m"]), "-p", prefix, "-o", fa, "--layout", lay, prefix + ".fa"], capture_output=True)
    assert r.returncode == 0, r.stderr.decode()
    assert open(fa).read() == want_fa and open(lay).read() == want_lay
    assert ">unitig-0" in want_fa and " KC:i:" in want_fa
    host.unitig_file(prefix + ".fa", prefix, case["m"], out=fa, layout=None)  # the host class through its C entry point
    assert open(fa).read() == want_fa
    # overlap calls of 97 reads: records between reads of different pieces, every overlap once over the pieces
    host.unitig_file(prefix + ".fa", prefix, case["m"], out=fa, layout=lay, piece_reads=97)
    assert open(fa).read() == want_fa and open(lay).read() == want_lay
    r = subprocess.run([host.CLI_PATH, "unitig", "-p", prefix], capture_output=True)  # no READSFILE: the help text
    assert r.returncode == 0 and r.stdout.startswith(b"siga unitig [OPTION]") and b"--layout" in r.stdout
