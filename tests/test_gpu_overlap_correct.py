"""`siga correct -a overlap` on the GPU (csrc/sigax_pileup.hip) against the serial restatement of its rules
(tests/pileup_cases.py): the device form, the host form and the command line, byte for byte -- sequences, valid, changed and
the status words -- over random read sets and the hand-made boundary cases of every rule."""
import ctypes as C
import functools
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import pileup_cases as pc
from tests.fixtures import CACHE, ROOT
from tests.golden import make_reads as mr

pytestmark = pytest.mark.gpu

FIELDS = dict(S="seed_length", T="seed_stride", H="max_seed_hits", M="min_overlap", P="error_permille", C="conflict", D="min_depth",
              K="max_candidates", max_len="max_read_len")
G = pc.random_genome(400, 77)
REF_TEXT_SIZES = (300, 30239, 9680)  # (reads, text bytes, workspace bytes) of _random()'s reference set


def _kw(p, max_len=False):
    return {FIELDS[k]: v for k, v in p.items() if k != "max_len" or max_len}


def _index(refs):
    """the reference set's index files (oracle-built, cached under a name made of the reads) -> prefix"""
    key = hashlib.sha1("\n".join(refs).encode()).hexdigest()[:16]
    d = os.path.join(CACHE, "pileup_" + key)
    os.makedirs(d, exist_ok=True)
    prefix = os.path.join(d, "reads")
    if not all(os.path.exists(prefix + e) for e in (".bwt", ".sai")):
        po.Index.build(refs).save(prefix + ".bwt", prefix + ".sai")
    return prefix


def _open(refs):
    import siga_amd
    return siga_amd.FMIndexPair.load_forward(_index(refs), device=0)


class _Device:
    """device buffers of exactly their size, prefilled with 0xEE, on the HIP runtime the library is bound to"""

    def __init__(self):
        hip = C.CDLL("libamdhip64.so")
        hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        hip.hipFree.argtypes = [C.c_void_p]
        hip.hipStreamSynchronize.argtypes = [C.c_void_p]
        self.hip = hip
        self.held = []

    def buf(self, nbytes, src=None):
        q = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(q), max(nbytes, 1)) == 0
        self.held.append(q)
        assert self.hip.hipMemset(q, 0xEE, max(nbytes, 1)) == 0
        if src is not None and src.nbytes:
            assert self.hip.hipMemcpy(q, src.ctypes.data, src.nbytes, 1) == 0
        return q

    def get(self, q, dtype, count):
        out = np.zeros(count, dtype=dtype)
        if out.nbytes:
            assert self.hip.hipMemcpy(out.ctypes.data, q, out.nbytes, 2) == 0
        return out

    def free(self):
        for q in self.held:
            self.hip.hipFree(q)


def _device_round(pair, queries, p, hits_cap, lead=b"", max_len=False, then=None):
    """one sigax_pileup_device call on a stream -> (sequences as one bytes object, valid, changed, status8); `lead`: bytes in
    front of the first read, so that the offsets do not start at 0; then = (queries, hits_cap): a second call over the same d_work,
    as the first one has left it, and the result is the second call's"""
    from siga_amd import _lib
    L = _lib.lib()
    dev = _Device()
    stream = C.c_void_p()
    assert L.sigax_stream_create(0, C.byref(stream)) == 0
    ref = C.c_void_p()
    assert L.sigax_pile_ref_create(pair.handle, C.byref(ref)) == 0, _lib.last_error()
    try:
        d_text, d_toffs = C.c_void_p(), C.c_void_p()
        assert L.sigax_pile_ref_buffers(ref, C.byref(d_text), C.byref(d_toffs), None) == 0
        d_work, work_bytes = None, 0
        for queries, hits_cap in [(queries, hits_cap)] + ([then] if then else []):
            buf, offs = po.pack_reads(queries)
            buf = np.frombuffer(lead + buf, dtype=np.uint8)
            offs = offs + np.uint64(len(lead))
            n, nb = len(queries), int(offs[-1] - offs[0])
            params = _lib.PileParams(**_kw(p, max_len))
            wb = C.c_uint64()
            assert L.sigax_pileup_workspace(n, nb, C.byref(params), hits_cap, C.byref(wb)) == 0, _lib.last_error()
            if d_work is None:
                d_work, work_bytes = dev.buf(wb.value), wb.value
            assert wb.value <= work_bytes
            d_seqs, d_offs = dev.buf(buf.nbytes, buf), dev.buf(offs.nbytes, offs)
            d_out, d_valid, d_changed = dev.buf(buf.nbytes), dev.buf(n), dev.buf(n)
            d_stat = dev.buf(64)
            assert dev.hip.hipDeviceSynchronize() == 0
            assert L.sigax_pileup_device(pair.handle, d_seqs, d_offs, n, nb, C.byref(params), d_text, d_toffs, d_out, d_valid, d_changed, d_stat,
                                         d_work, wb.value, hits_cap, stream) == 0, _lib.last_error()
            assert dev.hip.hipStreamSynchronize(stream) == 0
            got = (dev.get(d_out, np.uint8, buf.nbytes).tobytes(), dev.get(d_valid, np.uint8, n), dev.get(d_changed, np.uint8, n),
                   dev.get(d_stat, np.uint64, 8))
            assert not then or got[3][0] <= hits_cap  # with a second call to come, the first one ran through
        return got
    finally:
        L.sigax_pile_ref_destroy(ref)
        dev.free()
        L.sigax_stream_destroy(0, stream)


def _check_forms(refs, queries, p, rounds=1, device=True):
    """the host form over `rounds` and the device form over one round against the restatement -> the restatement's result"""
    want = pc.expected_pileup(refs, queries, p, rounds)
    pair = _open(refs)
    try:
        seqs, valid, changed, status, run = pair.correct_overlap(queries, rounds=rounds, **_kw(p))
        assert [s.decode() for s in seqs] == want["seqs"]
        assert valid.tolist() == want["valid"] and changed.tolist() == want["changed"]
        assert status.tolist() == want["status"] and run == want["rounds_run"]
        if device:
            outs, v1, c1, st1 = pc.expected_round(refs, queries, p)
            need = st1[0]
            got = _device_round(pair, queries, p, need, max_len=True)
            assert got[0].decode() == "".join(outs)
            assert got[1].tolist() == v1 and got[2].tolist() == c1 and got[3].tolist() == st1
    finally:
        pair.close()
    return want


# ---- random read sets ----
@functools.lru_cache(maxsize=None)
def _random():
    case = pc.random_case()
    g = case["genome"]
    # the lengths around the seed and the wave: S - 1, S, 63, 64, 65, 129
    extra = [g[500:500 + n] for n in (23, 24, 63, 64, 65, 129)] + [pc.mutate(g[900:900 + n], [n // 2]) for n in (63, 64, 65, 129)]
    return case["refs"], case["queries"] + extra


def test_random_reads_all_forms():
    refs, queries = _random()
    p = pc.params(C=3)
    want = _check_forms(refs, queries, p)
    assert 0 in want["valid"] and 1 in want["valid"] and want["status"][7] > 10 and 1 in want["changed"]
    assert want["status"][6] < want["status"][5]  # some candidates are refused
    assert any(q not in refs for q, v in zip(queries, want["valid"]) if v)  # queries that are not in the index
    assert any("N" in q and "N" not in s for q, s in zip(queries, want["seqs"]))  # an N replaced


def test_random_reads_short_seeds_three_rounds():
    refs, queries = _random()
    p = pc.params(S=12, T=5, M=30, P=60, C=2, D=1, H=64)
    want = _check_forms(refs, queries[::2], p, rounds=3)
    assert want["rounds_run"] >= 2


def test_reference_text_is_the_reads():
    from siga_amd import _lib
    L = _lib.lib()
    refs, _ = _random()
    pair = _open(refs)
    dev = _Device()
    try:
        tb, wb = C.c_uint64(), C.c_uint64()
        assert L.sigax_reference_text_workspace(pair.handle, C.byref(tb), C.byref(wb)) == 0
        assert tb.value == sum(len(r) for r in refs)
        d_text, d_offs, d_stat, d_work = dev.buf(tb.value), dev.buf(8 * (len(refs) + 1)), dev.buf(32), dev.buf(wb.value)
        assert L.sigax_reference_text_device(pair.handle, d_text, tb.value, d_offs, d_stat, d_work, wb.value, None) == 0, _lib.last_error()
        assert dev.hip.hipStreamSynchronize(None) == 0
        offs = dev.get(d_offs, np.uint64, len(refs) + 1)
        text = dev.get(d_text, np.uint8, tb.value).tobytes().decode()
        assert [text[int(offs[i]):int(offs[i + 1])] for i in range(len(refs))] == refs
        assert dev.get(d_stat, np.uint64, 4).tolist() == [len(refs), tb.value, 0, 0]
        assert L.sigax_reference_text_device(pair.handle, d_text, tb.value - 1, d_offs, d_stat, d_work, wb.value, None) == _lib.SIGAX_E_ARG
        assert L.sigax_reference_text_device(pair.handle, d_text, tb.value, d_offs, d_stat, d_work, wb.value - 1, None) == _lib.SIGAX_E_ARG
        assert L.sigax_reference_text_device(pair.handle, None, tb.value, d_offs, d_stat, d_work, wb.value, None) == _lib.SIGAX_E_ARG
    finally:
        dev.free()
        pair.close()


def test_reference_text_workspace_sizes():
    """the two sizes for _random()'s reference set, as recorded before the reference text moved to sigax_seeded.cpp"""
    from siga_amd import _lib
    refs, _ = _random()
    pair = _open(refs)
    try:
        tb, wb = C.c_uint64(), C.c_uint64()
        assert _lib.lib().sigax_reference_text_workspace(pair.handle, C.byref(tb), C.byref(wb)) == 0
        assert (len(refs), tb.value, wb.value) == REF_TEXT_SIZES
    finally:
        pair.close()


def test_two_calls_in_one_workspace():
    """a call with fewer reads over the d_work of an earlier one gives what it gives in fresh memory: the seeding stage zeroes
    what the kernels behind it take as zero"""
    refs, queries = _random()
    p = pc.params(C=3)
    few = queries[5:40:3]
    outs, valid, changed, st = pc.expected_round(refs, few, p)
    pair = _open(refs)
    try:
        fresh = _device_round(pair, few, p, st[0], max_len=True)
        again = _device_round(pair, queries, p, 1 << 18, max_len=True, then=(few, st[0]))
        for got in (fresh, again):
            assert got[0].decode() == "".join(outs)
            assert got[1].tolist() == valid and got[2].tolist() == changed and got[3].tolist() == st
        assert st[5] > st[6] > 0 and 1 in changed
    finally:
        pair.close()


# ---- the hand-made sets: one per rule ----
def test_diagonals_and_strands():
    """positive, zero and negative diagonals, a candidate inside and one around the query, mixed lengths, each on both strands"""
    q = G[100:160]
    spans = [(90, 150), (100, 160), (110, 170), (105, 155), (80, 180), (60, 140)]
    refs = [G[a:b] for a, b in spans] + [pc.revcomp(G[a:b]) for a, b in spans]
    p = pc.params(S=12, T=6, M=40, P=0, C=3, D=1)
    want = _check_forms(refs, [q, pc.revcomp(q), pc.mutate(q, [31])], p)
    assert want["status"][5] == want["status"][6] + 12 == 36 and want["valid"] == [1, 1, 0]  # the mutated query is refused by all at P = 0 ...
    want = _check_forms(refs, [pc.mutate(q, [31])], pc.params(S=12, T=6, M=40, P=25, C=3, D=1))
    assert want["seqs"] == [q] and want["changed"] == [1]  # ... and repaired at P = 25


def test_acceptance_edges():
    q = G[100:160]
    refs = [G[115:200], G[115:201], G[100:160], G[100:160]]  # overlaps of 45 columns; the query itself twice, for depth
    bad = pc.mutate(q, [20, 30])
    for p in (pc.params(S=12, T=6, M=45, P=0, D=1), pc.params(S=12, T=6, M=46, P=0, D=1), pc.params(S=12, T=6, M=45, P=45, D=1),
              pc.params(S=12, T=6, M=45, P=44, D=1)):
        _check_forms(refs, [q, bad], p)
    a = pc.expected_round(refs, [bad], pc.params(S=12, T=6, M=45, P=45, D=1))[3]
    b = pc.expected_round(refs, [bad], pc.params(S=12, T=6, M=45, P=44, D=1))[3]
    assert a[6] == b[6] + 2  # m = floor(l P / 1000) and one more


def test_distinct_candidates():
    q = G[100:160]
    p = pc.params(S=12, T=1, M=20, P=0, C=1, D=1)
    want = _check_forms([q], [q], p)
    assert want["status"][0] == 49 and want["status"][5] == 1  # one triple through 49 seeds
    unit = G[0:30]
    want = _check_forms([unit + unit + G[200:220]], [unit], p)
    assert want["status"][5] == want["status"][6] == 2  # one read at two diagonals


def _vote_case(n_good, n_bad):
    q = pc.mutate(G[100:160], [30])
    refs = [G[100 - i:160 + i] for i in range(1, n_good + 1)] + [pc.mutate(G, [130])[100 - i:160 + i] for i in range(20, 20 + n_bad)]
    return q, refs


@pytest.mark.parametrize("good,bad,conflict", [(3, 2, 3), (2, 1, 3), (4, 3, 3), (3, 3, 3), (3, 3, 4)])
def test_vote_edges(good, bad, conflict):
    """cnt[c] = C and C - 1, cnt[b] = C - 1 and C, a tie"""
    q, refs = _vote_case(good, bad)
    want = _check_forms(refs, [q], pc.params(S=12, T=6, M=40, P=50, C=conflict, D=1))
    assert want["changed"] == [1 if (good, bad) == (3, 2) else 0]


def test_depth_and_n():
    q = G[100:160]
    refs = [G[100:160], G[100:160], G[110:200]]
    withn = q[:30] + "N" + q[31:]
    for depth in (2, 3):  # D at and above the thinnest column
        want = _check_forms(refs, [q, withn, "N" * 60], pc.params(S=12, T=6, M=40, P=50, C=2, D=depth))
        assert want["valid"] == [1 if depth == 2 else 0] * 2 + [0]
    assert want["seqs"][1] == withn


def test_seed_and_candidate_caps():
    q = G[100:160]
    refs = [q] * 5
    for h, k in ((5, 512), (4, 512), (256, 5), (256, 4)):  # a seed at H hits and at H + 1; K and K + 1 distinct candidates
        want = _check_forms(refs, [q, G[200:260]], pc.params(S=12, T=6, M=40, P=0, C=2, D=1, H=h, K=k))
        assert want["valid"] == [1 if (h, k) in ((5, 512), (256, 5)) else 0, 0]


def test_hits_cap_one_too_small_then_sized_from_it():
    refs, queries = _random()
    p = pc.params(C=3)
    outs, valid, changed, st = pc.expected_round(refs, queries, p)
    need = st[0]
    pair = _open(refs)
    try:
        got = _device_round(pair, queries, p, need - 1, max_len=True)
        assert got[3].tolist() == [need, 0, 0, 0, 0, 0, 0, 0]
        assert got[0] == b"\xee" * len(got[0]) and got[1].tobytes() == b"\xee" * len(queries) == got[2].tobytes()
        got = _device_round(pair, queries, p, int(got[3][0]), lead=b"ACGTAC", max_len=True)  # offsets that do not start at 0
        assert got[0] == b"\xee" * 6 + "".join(outs).encode()
        assert got[1].tolist() == valid and got[2].tolist() == changed and got[3].tolist() == st
    finally:
        pair.close()


def test_longest_read_and_one_above():
    g = pc.random_genome(5000, 3)
    refs = [g[o:o + 200] for o in range(0, 4800, 50)]
    top = pc.PILE_MAX_LEN
    q = pc.mutate(g[100:100 + top], [7, 1000, 4000])
    p = pc.params(C=3, D=1)
    want = _check_forms(refs, [q, g[100:101 + top], g[300:400]], p)
    assert want["valid"] == [1, 2, 1] and want["seqs"][0] == g[100:100 + top] and want["status"][1] == 1
    assert want["status"][7] == 3


def test_reverse_candidates_across_column_2048():
    """a read of 4096 bases under 200-base reads of which every second one is reverse-complemented, with substitutions below
    and from column 2048 on: the second held word of a candidate together with the reversed text"""
    g = pc.random_genome(5000, 3)
    refs = [g[o:o + 200] if k % 2 else pc.revcomp(g[o:o + 200]) for k, o in enumerate(range(0, 4800, 50))]
    top = pc.PILE_MAX_LEN
    q = pc.mutate(g[100:100 + top], [7, 1000, 2047, 2048, 2111, 4000, 4090])
    want = _check_forms(refs, [q], pc.params(C=3, D=1))
    assert want["valid"] == [1] and want["seqs"] == [g[100:100 + top]] and want["status"][7] == 7


def test_rounds():
    g = pc.random_genome(600, 9)
    truth = g[200:300]
    q = pc.mutate(truth, [3, 9, 17])  # three substitutions inside the first 20 bases, 20-fold cover
    refs = [g[200 - 5 * i:300 - 5 * i] for i in range(-10, 11) if i]
    want = _check_forms(refs, [q], pc.params(), rounds=1)
    assert want["seqs"] == [truth] and want["status"][7] == 3  # what one round gives
    case = pc.second_round_case()
    one = _check_forms(case["refs"], case["queries"], case["params"], rounds=1)
    two = _check_forms(case["refs"], case["queries"], case["params"], rounds=4, device=False)
    assert one["seqs"] != two["seqs"] and two["seqs"] == [case["truth"]] and two["rounds_run"] == 3


def test_empty_batch_and_pieces(monkeypatch):
    refs, queries = _random()
    p = pc.params(C=3)
    pair = _open(refs)
    try:
        seqs, valid, changed, status, run = pair.correct_overlap([], **_kw(p))
        assert seqs == [] and len(valid) == 0 and not status.any() and run == 0
        # pieces of seven reads, and a first try whose hits do not fit: the same answer
        monkeypatch.setenv("SIGAX_TEST_PILE_PIECE", "7")
        monkeypatch.setenv("SIGAX_TEST_PILE_HITS_CAP", "3")
        want = pc.expected_pileup(refs, queries, p, 2)
        seqs, valid, changed, status, run = pair.correct_overlap(queries, rounds=2, **_kw(p))
        assert [s.decode() for s in seqs] == want["seqs"] and valid.tolist() == want["valid"] and changed.tolist() == want["changed"]
        assert status.tolist() == want["status"] and run == want["rounds_run"]
    finally:
        pair.close()


_CHILD = """
import sys
import numpy as np
sys.path.insert(0, %r)
import siga_amd
pair = siga_amd.FMIndexPair.load_forward(%r, device=0)
assert pair.info()["wide"] == %d
queries = open(%r).read().split()
seqs, valid, changed, status, run = pair.correct_overlap(queries, rounds=2, conflict=3)
np.savez(%r, np.frombuffer(b"".join(seqs), dtype=np.uint8), valid, changed, status)
pair.close()
"""


@pytest.mark.parametrize("env,wide", [({"SIGAX_TWO_STEP": "0"}, 0), ({"SIGAX_FORCE_WIDE": "1"}, 1)])
def test_without_two_step_tables_and_wide_positions(env, wide, tmp_path):
    refs, queries = _random()
    want = pc.expected_pileup(refs, queries, pc.params(C=3), 2)
    qf, out = str(tmp_path / "q.txt"), str(tmp_path / "res.npz")
    with open(qf, "w") as f:
        f.write("\n".join(queries))
    r = subprocess.run([sys.executable, "-c", _CHILD % (ROOT, _index(refs), wide, qf, out)], cwd=ROOT, env=dict(os.environ, **env),
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    z = np.load(out)
    assert z["arr_0"].tobytes().decode() == "".join(want["seqs"])
    assert z["arr_1"].tolist() == want["valid"] and z["arr_2"].tolist() == want["changed"] and z["arr_3"].tolist() == want["status"]


# ---- errors ----
def test_errors():
    import siga_amd
    from siga_amd import _lib
    from tests import test_gpu_match as tgm
    L = _lib.lib()
    refs, queries = _random()
    pair = _open(refs)
    try:
        wb = C.c_uint64()
        for field, bad in (("seed_length", 11), ("seed_length", 65), ("seed_stride", 0), ("seed_stride", 25), ("max_seed_hits", 0),
                           ("max_seed_hits", 4097), ("min_overlap", 0), ("error_permille", 251), ("conflict", 0), ("min_depth", 0),
                           ("max_candidates", 0), ("max_candidates", 4097), ("max_read_len", pc.PILE_MAX_LEN + 1)):
            params = _lib.PileParams(**{field: bad})
            assert L.sigax_pileup_workspace(1, 100, C.byref(params), 10, C.byref(wb)) == _lib.SIGAX_E_ARG, field
            assert field in _lib.last_error()
            with pytest.raises(siga_amd.overlap.SigaxError):
                pair.correct_overlap(queries[:2], **{field: bad})
        params = _lib.PileParams()
        assert L.sigax_pileup_workspace(1, 100, None, 10, C.byref(wb)) == _lib.SIGAX_E_ARG
        assert L.sigax_pileup_workspace(1, 100, C.byref(params), 10, None) == _lib.SIGAX_E_ARG
        assert L.sigax_pileup_workspace(1, 100, C.byref(params), 10, C.byref(wb)) == 0
        st = np.zeros(8, dtype=np.uint64)
        # NULL buffers: refused before anything is queued; an empty batch needs none but the status words
        assert L.sigax_pileup_device(pair.handle, None, None, 1, 100, C.byref(params), None, None, None, None, None, None, None, 0, 10,
                                     None) == _lib.SIGAX_E_ARG
        assert L.sigax_pileup_device(pair.handle, None, None, 1, 100, C.byref(params), None, None, None, None, None, st.ctypes.data, None, 0,
                                     10, None) == _lib.SIGAX_E_ARG
        assert L.sigax_pileup_batch(pair.handle, None, b"ACGT", st.ctypes.data, 1, C.byref(params), 1, None, None, None, None,
                                    None) == _lib.SIGAX_E_ARG
        with pytest.raises(siga_amd.overlap.SigaxError):
            pair.correct_overlap(queries[:2], rounds=0)
    finally:
        pair.close()
    pair = siga_amd.FMIndexPair.load_forward(_index(refs), device=0, with_sai=False)  # no .sai table
    try:
        with pytest.raises(siga_amd.overlap.SigaxError) as e:
            pair.correct_overlap(queries[:2])
        assert e.value.code == _lib.SIGAX_E_STATE and ".sai" in str(e.value)
        tb = C.c_uint64()
        assert L.sigax_reference_text_workspace(pair.handle, C.byref(tb), C.byref(tb)) == _lib.SIGAX_E_STATE
    finally:
        pair.close()
    prefix, _ = tgm._files(1)  # an index whose reads hold an N
    pair = siga_amd.FMIndexPair.load(prefix, device=0, with_sai=True, resident=False)
    try:
        with pytest.raises(siga_amd.overlap.SigaxError) as e:
            pair.correct_overlap(queries[:2])
        assert e.value.code == _lib.SIGAX_E_STATE and "ACGT" in str(e.value)
    finally:
        pair.close()


# ---- the host class and the command line ----
def _cli(args, cwd):
    from siga_amd import host
    return subprocess.run([host.CLI_PATH, "correct"] + args, capture_output=True, cwd=cwd)


def _fastq(named):
    return "".join("@%s\n%s\n+\n%s\n" % (n, s, "".join(chr(33 + (i * 7 + len(n)) % 40) for i in range(len(s)))) for n, s in named)


def test_cli_and_host_class(tmp_path):
    from siga_amd import host
    refs, queries = _random()
    prefix = _index(refs)
    d = str(tmp_path)
    named = [("q%d" % i, q) for i, q in enumerate(queries)]
    with open(os.path.join(d, "q.fa"), "w") as f:
        f.write(mr.fasta_text(named))
    with open(os.path.join(d, "q.fastq"), "w") as f:
        f.write(_fastq(named))
    want = pc.expected_pileup(refs, queries, pc.params(C=3), 2)
    keep = [(n, s) for (n, _), s, v in zip(named, want["seqs"], want["valid"]) if v == 1]
    assert 0 < len(keep) < len(named)
    r = _cli(["-a", "overlap", "-p", prefix, "--conflict=3", "-i", "2", "-o", "out.fa", "q.fa"], d)
    assert r.returncode == 0, r.stderr.decode()
    assert open(os.path.join(d, "out.fa")).read() == mr.fasta_text(keep)
    assert ("%d written" % len(keep)).encode() in r.stderr
    # FASTQ in, FASTQ out, the qualities as they came
    r = _cli(["--algorithm=overlap", "-p", prefix, "--conflict", "3", "--rounds=2", "-o", "out.fastq", "q.fastq"], d)
    assert r.returncode == 0, r.stderr.decode()
    quals = {n: l for n, l in zip([n for n, _ in named], _fastq(named).split("\n")[3::4])}
    assert open(os.path.join(d, "out.fastq")).read() == "".join("@%s\n%s\n+\n%s\n" % (n, s, quals[n]) for n, s in keep)
    # every option on the line
    p = pc.params(S=16, T=4, H=100, M=30, P=60, C=2, D=1, K=300)
    want = pc.expected_pileup(refs, queries, p, 1)
    r = _cli(["-a", "overlap", "-p", prefix, "--seed-length=16", "--seed-stride=4", "--max-seed-hits=100", "-m", "30", "-e", "60",
              "--conflict=2", "--min-depth=1", "--max-candidates=300", "-o", "out2.fa", "q.fa"], d)
    assert r.returncode == 0, r.stderr.decode()
    assert open(os.path.join(d, "out2.fa")).read() == mr.fasta_text([(n, s) for (n, _), s, v in zip(named, want["seqs"], want["valid"]) if v == 1])
    status = host.correct_file(os.path.join(d, "q.fa"), prefix, os.path.join(d, "out3.fa"), algorithm="overlap", **_kw(p))
    assert status.tolist() == want["status"]
    assert open(os.path.join(d, "out3.fa")).read() == open(os.path.join(d, "out2.fa")).read()


def test_cli_refusals(tmp_path):
    from tests import test_gpu_match as tgm
    refs, queries = _random()
    prefix = _index(refs)
    d = str(tmp_path)
    with open(os.path.join(d, "q.fa"), "w") as f:
        f.write(mr.fasta_text([("q%d" % i, q) for i, q in enumerate(queries[:5])]))
    for opt, name in ((["-k", "21"], b"-k"), (["-x", "2"], b"-x"), (["-O", "2"], b"-O")):
        r = _cli(["-a", "overlap", "-p", prefix] + opt + ["-o", "o.fa", "q.fa"], d)
        assert r.returncode == 1 and name in r.stderr and not os.path.exists(os.path.join(d, "o.fa"))
    for opt, name in ((["--seed-length=11"], b"seed_length"), (["-e", "300"], b"error_permille"), (["--max-candidates=5000"], b"max_candidates"),
                      (["-i", "0"], b"rounds"), (["--seed-stride=x"], b"seed_stride")):
        r = _cli(["-a", "overlap", "-p", prefix] + opt + ["-o", "o.fa", "q.fa"], d)
        assert r.returncode == 1 and name in r.stderr, (opt, r.stderr)
    nosai = os.path.join(d, "nosai")
    os.makedirs(nosai)
    os.symlink(prefix + ".bwt", os.path.join(nosai, "reads.bwt"))
    r = _cli(["-a", "overlap", "-p", os.path.join(nosai, "reads"), "-o", "o.fa", "q.fa"], d)
    assert r.returncode == 1 and b".sai" in r.stderr
    withn, _ = tgm._files(1)
    r = _cli(["-a", "overlap", "-p", withn, "-o", "o.fa", "q.fa"], d)
    assert r.returncode == 1 and b"ACGT" in r.stderr
    r = _cli(["-a", "nosuch", "-p", prefix, "-o", "o.fa", "q.fa"], d)
    assert r.returncode == 255 and b"not built" in r.stderr


def test_default_algorithm_is_kmer(tmp_path):
    refs, queries = _random()
    prefix = _index(refs)
    d = str(tmp_path)
    with open(os.path.join(d, "q.fa"), "w") as f:
        f.write(mr.fasta_text([("q%d" % i, q) for i, q in enumerate(queries)]))
    a = _cli(["-p", prefix, "-k", "21", "-o", "a.fa", "q.fa"], d)
    b = _cli(["-a", "kmer", "-p", prefix, "-k", "21", "-o", "b.fa", "q.fa"], d)
    assert a.returncode == 0 and b.returncode == 0, a.stderr + b.stderr
    out = open(os.path.join(d, "a.fa"), "rb").read()
    assert out == open(os.path.join(d, "b.fa"), "rb").read() and out.count(b">") > 0
    assert (a.stdout, a.stderr) == (b.stdout, b.stderr)
