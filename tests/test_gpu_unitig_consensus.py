"""The consensus pass of `siga unitig -e` on the GPU (csrc/sigax_consensus.hip) against the serial restatement of its rules
(tests/consensus_cases.py::expected_consensus): the device form, the host form and siga_amd.unitigs_consensus, each exactly --
bases, changed, support and all eight status words; guard bytes before and behind every output; hostile tables; refusals; the
device form enqueued on one stream straight behind the unitig call that feeds it; exact overlaps left as they are behind the
unitig calls."""
import ctypes as C
import os

import numpy as np
import pytest
import torch  # before the library loads: one HIP runtime per process

from tests import consensus_cases as cc
from tests import reduce_cases as rc
from tests import trim_cases as tc
from tests import unitig_cases as uc

pytestmark = pytest.mark.gpu
GUARD = 64
CASES = {c["name"]: c for c in cc.all_cases()}


def _up(a):
    a = np.frombuffer(a, dtype=np.uint8) if isinstance(a, bytes) else np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    return torch.from_numpy(a.copy()).to("cuda:0") if a.size else torch.zeros(16, dtype=torch.uint8, device="cuda:0")


class _Guarded:
    """nbytes of device memory between two runs of GUARD bytes of 0xEE; `fill` goes to the front of the nbytes"""

    def __init__(self, nbytes, fill=None):
        self.n = nbytes
        self.t = torch.full((nbytes + 2 * GUARD,), 0xEE, dtype=torch.uint8, device="cuda:0")
        if fill is not None and len(fill):
            self.t[GUARD:GUARD + len(fill)] = _up(fill)[:len(fill)]
        self.ptr = self.t.data_ptr() + GUARD

    def get(self):
        h = self.t.cpu().numpy()
        assert h[:GUARD].tobytes() == b"\xee" * GUARD and h[GUARD + self.n:].tobytes() == b"\xee" * GUARD, "guard bytes were written"
        return h[GUARD:GUARD + self.n]


def _tables(case, cap_unitigs):
    res = case["res"]
    so = np.full(cap_unitigs + 1, int(res["seq_offs"][-1]), dtype=np.uint64)  # (behind the unitigs: empty ones)
    lo = np.full(cap_unitigs + 1, int(res["lay_offs"][-1]), dtype=np.uint64)
    so[:len(res["seq_offs"])] = np.array(res["seq_offs"], dtype=np.uint64)
    lo[:len(res["lay_offs"])] = np.array(res["lay_offs"], dtype=np.uint64)
    return so, lo


def _device(case, min_votes=1, shift=0, support=True, nu=None, stream=None, hostile=None):
    """sigax_consensus_device over buffers of the sizes a unitig call uses -> expected_consensus's dict.  hostile: dict(seq_offs,
    lay_offs) the device gets in place of the case's; the whole of useqs comes back then"""
    from siga_amd import _lib
    L = _lib.lib()
    lengths, seqs, offs = cc.arrays(case, shift)
    n, res = len(lengths), case["res"]
    bases = int(offs[-1] - offs[0])
    so, lo = _tables(case if hostile is None else {"res": hostile}, n)
    lay = np.zeros(n, dtype=_lib.PLACEMENT_DTYPE)
    lay[:len(res["layout"])] = np.array(res["layout"], dtype=_lib.PLACEMENT_DTYPE)
    nu = len(res["seq_offs"]) - 1 if nu is None else nu
    d_nu, d_so, d_lo, d_lay, d_len, d_seqs, d_offs = _up(np.array([nu], dtype=np.uint64)), _up(so), _up(lo), _up(lay), _up(lengths), _up(seqs), _up(offs)
    wb = C.c_uint64()
    assert L.sigax_consensus_workspace(n, n, C.byref(wb)) == 0
    useqs, changed, sup = _Guarded(bases, bytes(res["useqs"])), _Guarded(4 * n), _Guarded(bases)
    status, work = _Guarded(64), _Guarded(wb.value)
    opts = _lib.ConsensusOpts(min_votes, (0, 0, 0))
    torch.cuda.synchronize()
    rc_ = L.sigax_consensus_device(0, d_nu.data_ptr(), n, d_so.data_ptr(), d_lo.data_ptr(), d_lay.data_ptr(), d_len.data_ptr(), d_seqs.data_ptr(),
                                   d_offs.data_ptr(), n, C.byref(opts), useqs.ptr, changed.ptr, sup.ptr if support else None, status.ptr, work.ptr,
                                   wb.value, stream)
    assert rc_ == 0, _lib.last_error()
    torch.cuda.synchronize()
    work.get()
    if hostile is not None:
        changed.get()
        return {"useqs": useqs.get().tobytes(), "support": sup.get().tobytes(), "status": [int(x) for x in status.get().view(np.uint64)]}
    total = int(res["seq_offs"][nu]) if nu < len(res["seq_offs"]) else int(res["seq_offs"][-1])
    got_changed = changed.get().view(np.uint32)
    assert not got_changed[min(nu, len(res["seq_offs"]) - 1):].any()
    own = bytes(res["useqs"])
    assert useqs.get()[total:].tobytes() == own[total:] + b"\xee" * (bases - len(own)), "useqs was written behind the unitigs"
    return {"useqs": useqs.get()[:total].tobytes(), "changed": [int(x) for x in got_changed[:min(nu, len(res["seq_offs"]) - 1)]],
            "support": sup.get()[:total].tobytes() if support else None, "status": [int(x) for x in status.get().view(np.uint64)]}


def _host(case, min_votes=1, shift=0, support=True):
    import siga_amd
    lengths, seqs, offs = cc.arrays(case, shift)
    res = dict(case["res"])
    before = bytes(res["useqs"])
    res["useqs"] = np.frombuffer(before, dtype=np.uint8)
    got = siga_amd.unitigs_consensus(res, lengths, seqs, offs, min_votes=min_votes, support=support)
    assert bytes(res["useqs"]) == before  # res is not modified
    return {"useqs": got["useqs"].tobytes(), "changed": [int(x) for x in got["changed"]],
            "support": got["support"].tobytes() if support else None, "status": [int(x) for x in got["status"]]}


def _same(got, exp, what):
    print(what, "status", got["status"], "expected", exp["status"])
    assert got["status"] == exp["status"], what
    assert got["changed"] == exp["changed"], what
    assert got["useqs"] == exp["useqs"], what
    assert got["support"] is None or got["support"] == exp["support"], what


@pytest.mark.parametrize("name", sorted(CASES))
def test_cases_device_and_host(name):
    """every shape, depth, vote and invalid placement of consensus_cases, with offs[0] = 0 and offs[0] = 37"""
    case = CASES[name]
    exp = cc.expected_consensus(case["reads"], case["res"], 1)
    _same(_device(case), exp, name + ", device")
    _same(_device(case, shift=37, support=False), exp, name + ", device, offs[0] = 37, no support")
    _same(_host(case), exp, name + ", host")
    _same(_host(case, shift=37, support=False), exp, name + ", host, offs[0] = 37, no support")


@pytest.mark.parametrize("min_votes", (2, 3))
@pytest.mark.parametrize("name", ("votes", "starts", "sizes"))
def test_min_votes(name, min_votes):
    case = CASES[name]
    exp = cc.expected_consensus(case["reads"], case["res"], min_votes)
    assert name != "votes" or exp["status"][5] > 0
    _same(_device(case, min_votes), exp, name + ", device")
    _same(_host(case, min_votes), exp, name + ", host")


def test_planted_errors_give_the_genome():
    for case in cc.planted_cases():
        got = _host(case)
        assert got["useqs"] == case["genomes"][0] != bytes(case["res"]["useqs"]), case["name"]
    deep = _device(CASES["deep300"])
    assert max(deep["support"]) == 255 and deep["status"][6] == 300


def test_count_on_the_device_is_clamped():
    """a count of unitigs above n_reads is taken as n_reads (the tables behind the unitigs say: no columns, no placements)"""
    case = CASES["short"]
    exp = cc.expected_consensus(case["reads"], case["res"], 1)
    got = _device(case, nu=1 << 40)
    n, nu = len(case["reads"]), len(case["res"]["uflags"])
    assert got["status"][0] == n and got["status"][1:] == exp["status"][1:]
    assert got["useqs"] == exp["useqs"] and got["changed"][:nu] == exp["changed"]
    fewer = _device(case, nu=3)
    assert fewer["status"][0] == 3 and fewer["status"][1] == int(case["res"]["seq_offs"][3])


@pytest.mark.parametrize("what", ("lay_offs", "seq_offs", "both"))
def test_tables_that_do_not_ascend_touch_nothing_outside(what):
    """lay_offs and seq_offs reversed, shuffled and filled with large numbers: the call returns, the guard bytes stand, and no byte
    of useqs becomes anything but a letter or what it was"""
    base = CASES["invalid"]
    rng = np.random.default_rng(5)
    own = bytes(base["res"]["useqs"])
    for trial in range(4):
        res = {k: list(base["res"][k]) for k in ("seq_offs", "lay_offs")}
        for key in (("lay_offs", "seq_offs") if what == "both" else (what,)):
            t = res[key]
            if trial == 0:
                t = t[::-1]
            elif trial == 1:
                t = [int(x) for x in rng.permutation(t)]
            elif trial == 2:
                t = [t[0], (1 << 63) + 5, 3, (1 << 64) - 1, t[-1]]
            else:
                t = [t[0], t[2], t[1], t[3], 1 << 33]
            res[key] = t
        got = _device(base, hostile=res)
        print(what, trial, "status", got["status"])
        was = own + b"\xee" * (len(got["useqs"]) - len(own))  # (the buffer holds as many bytes as the reads)
        assert all(b == was[k] or b in b"ACGT" for k, b in enumerate(got["useqs"]))
        assert got["status"][0] == 4 and got["status"][1] <= len(was)


def test_nothing_to_do_and_refusals():
    from siga_amd import _lib
    L = _lib.lib()
    E = _lib.SIGAX_E_ARG if hasattr(_lib, "SIGAX_E_ARG") else -1
    opts = _lib.ConsensusOpts(1, (0, 0, 0))
    st = _Guarded(64)
    assert L.sigax_consensus_device(0, None, 0, None, None, None, None, None, None, 0, C.byref(opts), None, None, None, st.ptr, None, 0, None) == 0
    torch.cuda.synchronize()
    assert not st.get().any()
    # no unitigs: every status word zero but for nothing, nothing written
    case = CASES["short"]
    got = _device(case, nu=0)
    assert got["status"] == [0] * 8 and got["useqs"] == b"" and got["changed"] == []
    # host form without reads
    ch, status = C.c_void_p(), np.ones(8, dtype=np.uint64)
    z = np.zeros(1, dtype=np.uint64)
    assert L.sigax_consensus_host(0, 0, z.ctypes.data, z.ctypes.data, None, None, None, z.ctypes.data, 0, C.byref(opts), None, C.byref(ch), None,
                                  status.ctypes.data) == 0
    assert not status.any()
    L.sigax_free(ch)
    # refusals
    b = [torch.zeros(1 << 16, dtype=torch.uint8, device="cuda:0") for _ in range(12)]
    p = [t.data_ptr() for t in b]
    wb = C.c_uint64()
    assert L.sigax_consensus_workspace(4, 4, C.byref(wb)) == 0 and wb.value <= 1 << 16
    assert L.sigax_consensus_workspace(1 << 31, 4, C.byref(wb)) == E
    assert L.sigax_consensus_workspace(4, 4, None) == E
    assert L.sigax_consensus_workspace(4, 4, C.byref(wb)) == 0

    def call(nulls=(), odd=None, o=opts, n=4, work=None):
        a = list(p)
        for k in nulls:
            a[k] = None
        if odd is not None:
            a[odd[0]] += odd[1]
        return L.sigax_consensus_device(0, a[0], 4, a[1], a[2], a[3], a[4], a[5], a[6], n, o, a[7], a[8], a[9], a[10], a[11],
                                        wb.value if work is None else work, None)

    assert call() == 0
    assert call(nulls=(9,)) == 0  # support is optional
    for k in (0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 11):
        assert call(nulls=(k,)) == E, k
    for k, by in ((0, 4), (1, 4), (2, 4), (6, 4), (10, 4), (3, 8), (7, 8), (9, 8), (11, 8), (4, 2), (8, 2)):
        assert call(odd=(k, by)) == E, (k, by)
    assert call(work=wb.value - 1) == E
    assert call(o=None) == E
    assert call(o=C.byref(_lib.ConsensusOpts(0, (0, 0, 0)))) == E
    for k in range(3):
        r = [0, 0, 0]
        r[k] = 1
        assert call(o=C.byref(_lib.ConsensusOpts(1, tuple(r)))) == E
    assert call(n=1 << 31) == E
    torch.cuda.synchronize()
    ch = C.c_void_p()
    assert L.sigax_consensus_host(0, 5, z.ctypes.data, z.ctypes.data, None, z.ctypes.data, b"", z.ctypes.data, 4, C.byref(opts), None, C.byref(ch), None,
                                  status.ctypes.data) == E  # more unitigs than reads


def _unitigs_then_consensus(case):
    """sigax_unitigs_device and sigax_consensus_device enqueued on one stream, nothing in between, the count of unitigs read from
    the unitig call's status block on the device -> (the unitig call's bases, the consensus dict)"""
    from siga_amd import _lib
    L = _lib.lib()
    edges, lengths, seqs, offs = uc.arrays(case)
    n, ne, nb = len(lengths), len(edges), len(seqs)
    d_edges, d_len, d_seqs, d_offs = _up(edges), _up(lengths), _up(seqs), _up(offs)
    wb, cb = C.c_uint64(), C.c_uint64()
    assert L.sigax_unitigs_workspace(n, ne, C.byref(wb)) == 0 and L.sigax_consensus_workspace(n, n, C.byref(cb)) == 0
    u = {k: _Guarded(v) for k, v in {"seq_offs": 8 * (n + 1), "lay_offs": 8 * (n + 1), "uflags": 4 * n, "layout": 16 * n, "useqs": nb, "status6": 48,
                                     "work": wb.value, "changed": 4 * n, "support": nb, "status8": 64, "cwork": cb.value}.items()}
    st = C.c_void_p()
    assert L.sigax_stream_create(0, C.byref(st)) == 0
    opts = _lib.ConsensusOpts(1, (0, 0, 0))
    torch.cuda.synchronize()
    try:
        rc_ = L.sigax_unitigs_device(0, d_edges.data_ptr(), ne, d_len.data_ptr(), d_seqs.data_ptr(), d_offs.data_ptr(), n, case["m"], u["seq_offs"].ptr,
                                     u["lay_offs"].ptr, u["uflags"].ptr, u["layout"].ptr, u["useqs"].ptr, u["status6"].ptr, u["work"].ptr, wb.value, st)
        assert rc_ == 0, _lib.last_error()
        rc_ = L.sigax_consensus_device(0, u["status6"].ptr, n, u["seq_offs"].ptr, u["lay_offs"].ptr, u["layout"].ptr, d_len.data_ptr(),
                                       d_seqs.data_ptr(), d_offs.data_ptr(), n, C.byref(opts), u["useqs"].ptr, u["changed"].ptr, u["support"].ptr,
                                       u["status8"].ptr, u["cwork"].ptr, cb.value, st)
        assert rc_ == 0, _lib.last_error()
        torch.cuda.synchronize()
    finally:
        L.sigax_stream_destroy(0, st)
    h = {k: v.get() for k, v in u.items()}
    nu, total = int(h["status6"].view(np.uint64)[0]), int(h["status6"].view(np.uint64)[1])
    return {"useqs": h["useqs"][:total].tobytes(), "changed": [int(x) for x in h["changed"].view(np.uint32)[:nu]],
            "support": h["support"][:total].tobytes(), "status": [int(x) for x in h["status8"].view(np.uint64)]}


def test_enqueued_behind_the_unitig_call():
    for case in cc.planted_cases()[:2] + (CASES["sizes"], CASES["ring"]):
        exp = cc.expected_consensus(case["reads"], case["res"], 1)
        _same(_unitigs_then_consensus(case), exp, case["name"])


def test_exact_overlaps_change_nothing_behind_the_unitig_calls():
    """behind unitigs, unitigs_trim and unitigs_reduce on their own case sets: no byte changes, changed is zero everywhere"""
    import siga_amd
    runs = []
    for c in uc.hand_built():
        edges, lengths, seqs, offs = uc.arrays(c)
        runs.append((c["name"], siga_amd.unitigs(edges, lengths, seqs, offs, c["m"]), lengths, seqs, offs))
    for c in tc.hand_built():
        edges, lengths, seqs, offs = uc.arrays(c)
        runs.append((c["name"], siga_amd.unitigs_trim(edges, lengths, seqs, offs, c["m"], c["x"], c["L"], c["C"]), lengths, seqs, offs))
    for c in rc.hand_built():
        edges, lengths, seqs, offs = uc.arrays(c)
        kw = dict(delta=c["delta"], careful=c["careful"], num_reads=c["N"], genome_size=c["G"], uniq_threshold=c["T"], min_chimeric_length=c["Lc"],
                  min_chimeric_coverage=c["Ac"], chimeric_delta=c["delta_c"], chimeric_threshold=c["Tc"], max_bubble_span=c["Lb"],
                  bubble_divergence=c["D"], max_edits=c["Ed"], edit_permille=c["De"], reduce=c.get("reduce", True))
        runs.append((c["name"], siga_amd.unitigs_reduce(edges, lengths, seqs, offs, c["m"], c["x"], c["L"], c["C"], **kw), lengths, seqs, offs))
    for name, res, lengths, seqs, offs in runs:
        got = siga_amd.unitigs_consensus(res, lengths, seqs, offs, support=True)
        assert got["useqs"].tobytes() == res["useqs"].tobytes(), name
        assert not got["changed"].any() and int(got["status"][2]) == 0 and int(got["status"][7]) == 0, name
        assert int(got["status"][0]) == len(res["uflags"]) and int(got["status"][1]) == len(res["useqs"]), name


# ---- whole runs: the host class and the command line, on the noisy sets ----
def _cli(args, cwd):
    import subprocess
    from siga_amd import host
    return subprocess.run([host.CLI_PATH, "unitig"] + args, capture_output=True, cwd=cwd)


ALL_EXTS = (".bwt", ".sai", ".rbwt", ".rsai", ".fa")


def _files(refs, names, d, exts=ALL_EXTS):
    from tests.test_gpu_mmoverlap import _index, _link_index
    return _link_index(_index(refs, names, both=True), d, exts)


def _expected_files(case, exp, consensus=True):
    """the FASTA, layout, contained and graph texts of `siga unitig -e` over a noisy set"""
    red, names = exp["reduced"], case["names"]
    bases = exp["consensus"]["useqs"] if consensus else bytes(red["useqs"])
    fa, lay, vt = [], [], []
    for u in range(len(red["uflags"])):
        a, b = red["lay_offs"][u], red["lay_offs"][u + 1]
        if b - a == 1 and exp["contained"][red["layout"][a][0]]:
            continue
        seq = bases[red["seq_offs"][u]:red["seq_offs"][u + 1]].decode()
        head = ">unitig-%d" % u + (" KC:i:%d" % (b - a) if b - a > 1 else "") + (" changed=%d" % exp["consensus"]["changed"][u] if consensus else "")
        fa.append(head + "\n" + seq + "\n")
        vt.append("VT\tunitig-%d\t%s\tSS:i:0" % (u, seq) + ("\tCR:i:%d" % (b - a) if b - a > 1 else "") + "\n")
        lay += ["unitig-%d\t%s\t%s\t%d\n" % (u, names[r], "-" if fl & 1 else "+", o) for r, fl, o in red["layout"][a:b]]
    assert red["uedges"] == []
    graph = "HT\tVN:i:1\tOL:i:%d\tCN:i:1\n" % cc.NOISY["M"] + "".join(vt)
    return "".join(fa), "".join(lay), "".join(n + "\n" for n, c in zip(names, exp["contained"]) if c), graph


NOISY_ARGS = ["-e", "40", "--reduce", "-m", "30", "--seed-length", "12", "--seed-stride", "4"]


@pytest.mark.parametrize("seed,mixed", ((0, False), (1, True)))
def test_cli_and_host_on_noisy_reads(seed, mixed, tmp_path):
    from siga_amd import host
    case, exp = cc.noisy_case(seed, mixed), cc.noisy_expected(seed, mixed)
    d = str(tmp_path)
    prefix = _files([r.decode() for r in case["reads"]], case["names"], d)
    fa, lay, contained, graph = _expected_files(case, exp)
    r = _cli(NOISY_ARGS + ["-o", "u.fa", "--layout", "u.lay", "--contained", "u.contained", "--graph", "u.asqg", "reads.fa"], d)
    assert r.returncode == 0, r.stderr.decode()
    read = lambda name: open(os.path.join(d, name)).read()
    assert read("u.fa") == fa and fa.count(">") == 1 and fa.split("\n")[1].encode() in (case["genome"], cc.uc.revcomp(case["genome"]))
    assert read("u.lay") == lay and read("u.contained") == contained and read("u.asqg") == graph
    # the copy bases
    r = _cli(NOISY_ARGS + ["--no-consensus", "-o", "copy.fa", "reads.fa"], d)
    assert r.returncode == 0, r.stderr.decode()
    copy = _expected_files(case, exp, consensus=False)[0]
    assert read("copy.fa") == copy and copy.split("\n")[1] != fa.split("\n")[1]
    # the wrapper gives the same files
    st = host.unitig_file(prefix + ".fa", prefix, 30, out=os.path.join(d, "w.fa"), layout=os.path.join(d, "w.lay"), reduce=True, error_permille=40,
                          contained=os.path.join(d, "w.contained"), graph=os.path.join(d, "w.asqg"), seed_length=12, seed_stride=4)
    assert (read("w.fa"), read("w.lay"), read("w.contained"), read("w.asqg")) == (fa, lay, contained, graph)
    assert st["contained_reads"] == sum(exp["contained"]) and st["columns_changed"] == exp["consensus"]["status"][2]


def test_e0_is_the_exhaustive_run_and_consensus_alone_changes_nothing(tmp_path):
    """equal lengths at distinct places, neither contained nor duplicate reads: -e 0 --reduce gives the FASTA of --exhaustive
    --reduce, headers apart; --consensus without -e changes no base"""
    from tests import mmoverlap_cases as mc
    refs, names = mc.exact_case()
    d = str(tmp_path)
    _files(refs, names, d)
    runs = {"e0": ["-e", "0", "--reduce", "--seed-length", "12", "--seed-stride", "4"], "exh": ["--exhaustive", "--reduce"],
            "exh_cons": ["--exhaustive", "--reduce", "--consensus"], "plain": [], "plain_cons": ["--consensus", "--consensus-min-votes", "2"]}
    text = {}
    for k, args in runs.items():
        r = _cli(args + ["-m", "45", "-o", k + ".fa", "reads.fa"], d)
        assert r.returncode == 0, r.stderr.decode()
        text[k] = open(os.path.join(d, k + ".fa")).read().split("\n")
    assert text["e0"][1::2] == text["exh"][1::2] and len(text["exh"]) > 2
    assert [h + " changed=0" for h in text["exh"][0::2] if h] == [h for h in text["e0"][0::2] if h] == [h for h in text["exh_cons"][0::2] if h]
    assert text["exh_cons"][1::2] == text["exh"][1::2] and text["plain_cons"][1::2] == text["plain"][1::2]
    assert [h + " changed=0" for h in text["plain"][0::2] if h] == [h for h in text["plain_cons"][0::2] if h]


def test_cli_refusals_of_e(tmp_path):
    from tests import mmoverlap_cases as mc
    from tests import test_gpu_match as tgm
    refs, names = mc.exact_case()
    d = str(tmp_path)
    _files(refs, names, d)
    for opt, word in ((["--seed-length=16"], b"--seed-length"), (["--seed-stride=4"], b"--seed-stride"), (["--max-seed-hits=9"], b"--max-seed-hits"),
                      (["--max-candidates=9"], b"--max-candidates"), (["--contained", "c.txt"], b"--contained"),
                      (["--consensus-min-votes", "2"], b"--consensus-min-votes"), (["-e", "40", "--no-consensus", "--consensus-min-votes", "2"], b"--consensus-min-votes"),
                      (["--consensus", "--consensus-min-votes", "0"], b"--consensus-min-votes"),
                      (["-e", "40", "--exhaustive"], b"--exhaustive"), (["-e", "40", "--no-opposite-strand"], b"--no-opposite-strand"),
                      (["-e", "300"], b"error_permille"), (["-e", "40", "--seed-length=11"], b"seed_length")):
        r = _cli(opt + ["-o", "no.fa", "reads.fa"], d)
        assert r.returncode == 1 and word in r.stderr and not os.path.exists(os.path.join(d, "no.fa")), (opt, r.stderr)
    nosai = os.path.join(d, "nosai")
    os.makedirs(nosai)
    _files(refs, names, nosai, (".bwt", ".rbwt", ".fa"))
    r = _cli(["-e", "40", "-o", "no.fa", "reads.fa"], nosai)
    assert r.returncode != 0 and b".sai" in r.stderr and not os.path.exists(os.path.join(nosai, "no.fa"))
    withn, fa = tgm._files(1)
    r = _cli(["-e", "40", "-o", os.path.join(d, "no.fa"), "-p", withn, fa], d)
    assert r.returncode != 0 and b"ACGT" in r.stderr and not os.path.exists(os.path.join(d, "no.fa"))
    r = _cli(["--help"], d)
    for word in (b"--error-permille", b"--seed-length", b"--consensus", b"--no-consensus", b"--consensus-min-votes", b"--contained", b"--reduce"):
        assert word in r.stdout


def test_pairs_with_a_contained_mate(tmp_path):
    """mates by name: a pair with a contained mate is no pair, and the JSON says how many there were"""
    import json
    case, exp = cc.noisy_case(1, True), cc.noisy_expected(1, True)
    n = len(case["reads"])
    names = ["p%d/%d" % (k // 2, 1 + k % 2) for k in range(n)]  # reads 2k and 2k + 1 are mates
    d = str(tmp_path)
    _files([r.decode() for r in case["reads"]], names, d)
    r = _cli(NOISY_ARGS + ["-o", "u.fa", "--pairs", "p.json", "reads.fa"], d)
    assert r.returncode == 0, r.stderr.decode()
    got = json.load(open(os.path.join(d, "p.json")))["pairs"]
    # (the names changed, so the name ranks did: the contained flags of duplicates may move; this set has none)
    c = exp["contained"]
    with_contained = sum(1 for k in range(0, n - 1, 2) if c[k] or c[k + 1])
    assert got["contained_mates"] == with_contained > 0
    assert got["pairs"] == (n // 2) - with_contained and got["mate_entries"] == 2 * got["pairs"] and got["malformed"] == 0
    assert got["unplaced"] == 0 and got["same"] == got["pairs"]


def test_links_skip_a_contained_mate(tmp_path):
    """two genomes, two unitigs, every pair one read of each: the pairs with neither mate contained go into the LK lines, a pair
    with a contained mate gives none"""
    import json
    a, b = cc.noisy_case(0, False), cc.noisy_case(1, True)
    ca, cb = cc.noisy_expected(0, False)["contained"], cc.noisy_expected(1, True)["contained"]
    na, nb = len(a["reads"]), len(b["reads"])
    k = min(na, nb)
    names = ["p%d/1" % i if i < k else "s%dx" % i for i in range(na)] + ["p%d/2" % i if i < k else "t%dx" % i for i in range(nb)]  # (x: no mate by name)
    d = str(tmp_path)
    _files([r.decode() for r in a["reads"] + b["reads"]], names, d)
    r = _cli(NOISY_ARGS + ["-o", "u.fa", "--contained", "u.contained", "--pairs", "p.json", "--links", "l.txt", "reads.fa"], d)
    assert r.returncode == 0, r.stderr.decode()
    read = lambda name: open(os.path.join(d, name)).read()
    heads = [l for l in read("u.fa").split("\n") if l.startswith(">")]
    assert len(heads) == 2  # the two genomes share no overlap: one unitig each, the contained reads hidden
    assert read("u.contained") == "".join(n + "\n" for n, c in zip(names, ca + cb) if c)
    lost = sum(1 for i in range(k) if ca[i] or cb[i])
    got = json.load(open(os.path.join(d, "p.json")))["pairs"]
    assert 0 < lost < k and got["contained_mates"] == lost
    assert got["pairs"] == got["across"] == got["linked_pairs"] == k - lost and got["unplaced"] == got["same"] == got["malformed"] == 0
    links = [l.split("\t") for l in read("l.txt").split("\n") if l]
    units = {h.split()[0][1:] for h in heads}
    assert links and all(l[0] == "LK" and {l[1], l[3]} == units for l in links)
    assert sum(int(l[5]) for l in links) == k - lost == got["linked_pairs"]
