"""`siga preqc` on the GPU (csrc/sigax_spectrum.hip) against tests/spectrum_cases.py: index rows back to text -- every row of
`corner` and `ragged_n`, both strands, device and host form, out-of-range rows, cut walks, wrong slots -- and the k-mer count
distribution over every class of string, k around every edge of the kernel, saturating bins, accumulation, with and without
the table of 13-mer intervals; rows -> strings -> spectrum on the device; the command line.
tests/test_gpu_spectrum_forms.py runs this file again with 64-bit positions, small superblocks and without two-step lines."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import match_cases as mc
from tests import spectrum_cases as sc
from tests.fixtures import fixture

pytestmark = pytest.mark.gpu
E_ARG, E_STATE = -1, -6


def _open(prefix, both=True):
    import siga_amd
    from siga_amd import _lib
    if both:
        return siga_amd.FMIndexPair.load(prefix, device=0, with_sai=False, resident=False)
    h = C.c_void_p()
    assert _lib.lib().sigax_index_open((prefix + ".bwt").encode(), None, None, None, 0, C.byref(h)) == 0, _lib.last_error()
    return siga_amd.FMIndexPair(h.value)


class Device:
    """buffers in device memory, pre-filled with 0xEE, and a stream of the caller's own"""

    def __init__(self):
        from siga_amd import _lib
        self.L = _lib.lib()
        hip = C.CDLL("libamdhip64.so")
        hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        hip.hipFree.argtypes = [C.c_void_p]
        hip.hipStreamSynchronize.argtypes = [C.c_void_p]
        self.hip = hip
        self.held = []
        self.stream = C.c_void_p()
        assert self.L.sigax_stream_create(0, C.byref(self.stream)) == 0

    def buf(self, nbytes, src=None, fill=0xEE):
        q = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(q), max(nbytes, 16)) == 0
        self.held.append(q)
        assert self.hip.hipMemset(q, fill, max(nbytes, 16)) == 0
        if src is not None and src.nbytes:
            assert self.hip.hipMemcpy(q, src.ctypes.data, src.nbytes, 1) == 0
        assert self.hip.hipDeviceSynchronize() == 0
        return q

    def get(self, q, dtype, count):
        assert self.hip.hipStreamSynchronize(self.stream) == 0
        out = np.zeros(count, dtype=dtype)
        if out.nbytes:
            assert self.hip.hipMemcpy(out.ctypes.data, q, out.nbytes, 2) == 0
        return out

    def close(self):
        self.hip.hipStreamSynchronize(self.stream)
        for q in self.held:
            self.hip.hipFree(q)
        self.L.sigax_stream_destroy(0, self.stream)


def _walks(ix, rows, n_symbols, max_len=None):
    """the oracle's (text, stretch) per row; out of range: ("", None)"""
    return [sc.walk(ix, int(r), max_len) if int(r) < n_symbols else ("", None) for r in rows]


def _row_orders(n_symbols):
    every = np.arange(n_symbols, dtype=np.uint64)
    return np.concatenate([every, every[::-1][:300], np.array([7, 7, 0, 7, n_symbols - 1, 0], dtype=np.uint64)])


@pytest.mark.parametrize("which", (0, 1))
@pytest.mark.parametrize("name", ("corner", "ragged_n"))
def test_rows_to_text_host_form(name, which):
    """every row, then rows in descending and in repeated order: text and stretch index"""
    fx = fixture(name)
    ix = fx.rev if which else fx.fwd
    pair = _open(fx.prefix)
    try:
        n = pair.info()["n_symbols"]
        assert n == len(ix)
        rows = _row_orders(n)
        got, stretch = pair.get_strings(rows, which=which, stretch=True)
        want = _walks(ix, rows, n)
        for i, (text, st) in enumerate(want):
            assert got[i].decode() == text, "%s strand %d row %d" % (name, which, rows[i])
            assert int(stretch[i]) == st
    finally:
        pair.close()


@pytest.mark.parametrize("which", (0, 1))
@pytest.mark.parametrize("name", ("corner", "ragged_n"))
def test_rows_to_text_device_form(name, which):
    """lengths pass, the caller's prefix sum, write pass; a row = n_symbols and a row = 2^64 - 1 have length 0 and are counted"""
    fx = fixture(name)
    ix = fx.rev if which else fx.fwd
    pair = _open(fx.prefix)
    dev = Device()
    try:
        n = pair.info()["n_symbols"]
        rows = np.concatenate([_row_orders(n)[::-1], np.array([n, (1 << 64) - 1], dtype=np.uint64)])
        want = _walks(ix, rows, n)
        m = len(rows)
        d_rows, d_lens, d_stretch, d_status = dev.buf(rows.nbytes, rows), dev.buf(4 * m), dev.buf(8 * m), dev.buf(24)
        assert dev.L.sigax_string_lengths_device(pair.handle, which, d_rows, m, 1 << 20, d_lens, d_stretch, d_status, dev.stream) == 0
        lens, stretch, status = dev.get(d_lens, np.uint32, m), dev.get(d_stretch, np.uint64, m), dev.get(d_status, np.uint64, 2)
        assert [int(x) for x in lens] == [len(t) for t, _ in want]
        assert [int(x) for x in stretch] == [sc.NO_STRETCH if s is None else s for _, s in want]
        assert [int(x) for x in status] == [2, 0]
        assert lens[-1] == 0 and lens[-2] == 0
        # the same without the stretch indexes
        d_lens2 = dev.buf(4 * m)
        assert dev.L.sigax_string_lengths_device(pair.handle, which, d_rows, m, 1 << 20, d_lens2, None, d_status, dev.stream) == 0
        assert np.array_equal(dev.get(d_lens2, np.uint32, m), lens)
        offs = np.zeros(m + 1, dtype=np.uint64)
        offs[1:] = np.cumsum(lens, dtype=np.uint64)
        total = int(offs[-1])
        d_offs, d_seqs = dev.buf(offs.nbytes, offs), dev.buf(total + 32)
        assert dev.L.sigax_get_strings_device(pair.handle, which, d_rows, m, 1 << 20, d_offs, d_seqs, d_status, dev.stream) == 0
        text = dev.get(d_seqs, np.uint8, total + 32).tobytes()
        assert [int(x) for x in dev.get(d_status, np.uint64, 3)] == [2, 0, 0]
        assert text[:total].decode() == "".join(t for t, _ in want)
        assert text[total:] == b"\xee" * 32, "bytes behind the last string were written"
    finally:
        dev.close()
        pair.close()


def test_max_len_keeps_the_last_symbols_and_counts_the_cut_walks():
    fx = fixture("tiny")
    pair = _open(fx.prefix, both=False)
    dev = Device()
    try:
        n = pair.info()["n_symbols"]
        rows = np.arange(n, dtype=np.uint64)
        want = _walks(fx.fwd, rows, n, max_len=10)
        n_cut = sum(1 for _, s in want if s is None)
        assert n_cut > n // 2 and any(len(t) == 10 and s is not None for t, s in want)  # walks of exactly 10 symbols are not cut
        got, stretch = pair.get_strings(rows, max_len=10, stretch=True)
        assert [g.decode() for g in got] == [t for t, _ in want]
        assert [int(x) for x in stretch] == [sc.NO_STRETCH if s is None else s for _, s in want]
        d_rows, d_lens, d_status = dev.buf(rows.nbytes, rows), dev.buf(4 * n), dev.buf(16)
        assert dev.L.sigax_string_lengths_device(pair.handle, 0, d_rows, n, 10, d_lens, None, d_status, dev.stream) == 0
        assert [int(x) for x in dev.get(d_status, np.uint64, 2)] == [0, n_cut]
        assert int(dev.get(d_lens, np.uint32, n).max()) == 10
    finally:
        dev.close()
        pair.close()


def test_wrong_slot_is_counted_and_left_untouched():
    fx = fixture("corner")
    pair = _open(fx.prefix, both=False)
    dev = Device()
    try:
        n = pair.info()["n_symbols"]
        rows = np.arange(n, dtype=np.uint64)
        want = [t for t, _ in _walks(fx.fwd, rows, n)]
        big = max(range(n), key=lambda i: len(want[i]))
        small = next(i for i in range(n) if len(want[i]) >= 2 and i != big)
        slots = [len(t) for t in want]
        slots[big] += 1
        slots[small] -= 1
        offs = np.zeros(n + 1, dtype=np.uint64)
        offs[1:] = np.cumsum(slots, dtype=np.uint64)
        total = int(offs[-1])
        d_rows, d_offs, d_seqs, d_status = dev.buf(rows.nbytes, rows), dev.buf(offs.nbytes, offs), dev.buf(total), dev.buf(24)
        assert dev.L.sigax_get_strings_device(pair.handle, 0, d_rows, n, 1 << 20, d_offs, d_seqs, d_status, dev.stream) == 0
        assert [int(x) for x in dev.get(d_status, np.uint64, 3)] == [0, 0, 2]
        text = dev.get(d_seqs, np.uint8, total).tobytes()
        for i in range(n):
            slot = text[int(offs[i]):int(offs[i + 1])]
            assert slot == (b"\xee" * slots[i] if i in (big, small) else want[i].encode()), "row %d" % i
    finally:
        dev.close()
        pair.close()


def test_reverse_strand_on_a_forward_only_index():
    from siga_amd.overlap import SigaxError
    fx = fixture("corner")
    pair = _open(fx.prefix, both=False)
    dev = Device()
    try:
        rows = np.arange(5, dtype=np.uint64)
        assert [g.decode() for g in pair.get_strings(rows)] == [sc.walk(fx.fwd, r)[0] for r in range(5)]
        with pytest.raises(SigaxError) as e:
            pair.get_strings(rows, which=1)
        assert e.value.code == E_STATE
        d_rows, d_lens, d_offs, d_status = dev.buf(40, rows), dev.buf(20), dev.buf(48, np.zeros(6, dtype=np.uint64)), dev.buf(24)
        assert dev.L.sigax_string_lengths_device(pair.handle, 1, d_rows, 5, 100, d_lens, None, d_status, dev.stream) == E_STATE
        assert dev.L.sigax_get_strings_device(pair.handle, 1, d_rows, 5, 100, d_offs, d_lens, d_status, dev.stream) == E_STATE
        assert dev.L.sigax_string_lengths_device(pair.handle, 2, d_rows, 5, 100, d_lens, None, d_status, dev.stream) == E_ARG
        assert dev.L.sigax_string_lengths_device(pair.handle, 0, d_rows, 0, 100, d_lens, None, d_status, dev.stream) == 0
        assert [int(x) for x in dev.get(d_status, np.uint64, 2)] == [0, 0]
    finally:
        dev.close()
        pair.close()


# ---- k-mer spectrum ----
def _index(which):
    """-> (prefix, the oracle's forward index, the reads, palindromes among them)"""
    if which == "tiny":
        fx = fixture("tiny")
        return fx.prefix, fx.fwd, fx.seqs, ()
    case = mc.match_case(1)
    reads = [s for _, s in case["reads"]]
    pal = dict(case["reads"])["pal"]
    return sc.match_files(1), mc.oracle_index(1), reads, (pal, pal[20:80], pal[35:65])


def _leave_prefix_table(pair):
    """one correction call leaves the table of 13-mer intervals on the device"""
    from siga_amd import _lib
    seqs = np.frombuffer(b"ACGTACGTTGCATGCAACGTACGTTGCATGCAACGT", dtype=np.uint8)
    offs = np.array([0, len(seqs)], dtype=np.uint64)
    out, valid = np.zeros(len(seqs), dtype=np.uint8), np.zeros(1, dtype=np.uint8)
    assert _lib.lib().sigax_correct_batch(pair.handle, seqs.tobytes(), None, offs.ctypes.data, 1, 31, 3, 10, 1, out.ctypes.data,
                                          valid.ctypes.data) == 0, _lib.last_error()


def _assert_spectrum(pair, fwd, strings, k, what):
    for n_bins in sc.BINS:
        want, n, L, windows = sc.spectrum(fwd, strings, k, n_bins)
        hist, st = pair.kmer_spectrum(k, n_bins, seqs=strings)
        assert [int(x) for x in hist] == want, "%s k %d, %d bins" % (what, k, n_bins)
        assert (st["strings"], st["bases"], st["windows"]) == (n, L, windows), "%s k %d" % (what, k)
    # a second call into the same bins adds to them
    hist2, _ = pair.kmer_spectrum(k, n_bins, seqs=strings, hist=hist)
    assert hist2 is hist and [int(x) for x in hist] == [2 * x for x in want]


@pytest.mark.parametrize("k", sc.KS)
@pytest.mark.parametrize("which", ("tiny", "match1"))
def test_spectrum_of_every_class_of_string(which, k):
    prefix, fwd, reads, pals = _index(which)
    named = sc.spectrum_strings(reads, k, 1, extra=pals)
    strings = [s for _, s in named]
    pair = _open(prefix, both=which != "tiny")
    try:
        _assert_spectrum(pair, fwd, strings, k, "no prefix table")
        # one string per call, one of every class: a wrong window cannot hide behind another string's
        seen = set()
        for cls, s in named:
            if cls in seen:
                continue
            seen.add(cls)
            want, n, L, windows = sc.spectrum(fwd, [s], k, 1024)
            hist, st = pair.kmer_spectrum(k, 1024, seqs=[s])
            assert [int(x) for x in hist] == want, "%s alone (%d bases), k %d" % (cls, len(s), k)
            assert (st["strings"], st["bases"], st["windows"]) == (n, L, windows)
        _leave_prefix_table(pair)
        _assert_spectrum(pair, fwd, strings, k, "with the prefix table")
    finally:
        pair.close()


def test_spectrum_device_form_and_arguments():
    from siga_amd import _lib
    L = _lib.lib()
    fx = fixture("tiny")
    strings = [s for _, s in sc.spectrum_strings(fx.seqs, 31, 2)]
    want, n, bases, windows = sc.spectrum(fx.fwd, strings, 31, 64)
    pair = _open(fx.prefix, both=False)
    dev = Device()
    try:
        buf, offs = po.pack_reads(strings)
        buf = np.frombuffer(buf, dtype=np.uint8)
        need = C.c_uint64()
        assert L.sigax_kmer_spectrum_workspace(len(strings), C.byref(need)) == 0 and need.value > 0
        d_seqs, d_offs, d_hist = dev.buf(buf.nbytes, buf), dev.buf(offs.nbytes, offs), dev.buf(64 * 8, fill=0)
        d_stat, d_work = dev.buf(32), dev.buf(need.value)
        for rep in (1, 2):  # the bins are added to, the statistics written
            assert L.sigax_kmer_spectrum_device(pair.handle, d_seqs, d_offs, len(strings), 31, 64, d_hist, d_stat, d_work, need.value,
                                                dev.stream) == 0, _lib.last_error()
            assert [int(x) for x in dev.get(d_hist, np.uint64, 64)] == [rep * x for x in want]
            assert [int(x) for x in dev.get(d_stat, np.uint64, 3)] == [n, bases, windows]
        assert int(dev.get(d_stat, np.uint64, 4)[3]) > 0
        args = (d_hist, d_stat, d_work, need.value, dev.stream)
        assert L.sigax_kmer_spectrum_device(pair.handle, d_seqs, d_offs, len(strings), 0, 64, *args) == E_ARG
        assert L.sigax_kmer_spectrum_device(pair.handle, d_seqs, d_offs, len(strings), 31, 0, *args) == E_ARG
        assert L.sigax_kmer_spectrum_device(pair.handle, d_seqs, d_offs, len(strings), 31, 64, d_hist, d_stat, d_work, 0, dev.stream) == E_ARG
        assert L.sigax_kmer_spectrum_device(pair.handle, None, None, 0, 31, 64, None, None, None, 0, None) == 0
        assert L.sigax_kmer_spectrum_batch(pair.handle, None, None, 0, 31, 64, None, None) == 0
        assert L.sigax_kmer_spectrum_batch(pair.handle, b"ACGT", offs.ctypes.data, 1, 0, 64, d_hist, None) == E_ARG
        assert [int(x) for x in dev.get(d_hist, np.uint64, 64)] == [2 * x for x in want]
    finally:
        dev.close()
        pair.close()


def test_rows_to_strings_to_spectrum_on_the_device():
    fx = fixture("tiny")
    pair = _open(fx.prefix, both=False)
    try:
        n = pair.info()["n_strings"]
        assert n == len(fx.seqs)
        for k, n_bins in ((31, 1025), (13, 8)):
            want, ns, L, windows = sc.spectrum(fx.fwd, fx.seqs, k, n_bins)
            hist, st = pair.kmer_spectrum(k, n_bins, rows=np.arange(n))
            assert [int(x) for x in hist] == want
            assert (st["strings"], st["bases"], st["windows"]) == (ns, L, windows)
        # any rows: the strings the oracle walks to
        rows = np.array([0, 399, 400, 5000, 24399, 12345, 12345], dtype=np.uint64)
        strings = [sc.walk(fx.fwd, int(r))[0] for r in rows]
        want, ns, L, windows = sc.spectrum(fx.fwd, strings, 12, 1024)
        hist, st = pair.kmer_spectrum(12, 1024, rows=rows)
        assert [int(x) for x in hist] == want and (st["strings"], st["bases"], st["windows"]) == (ns, L, windows)
    finally:
        pair.close()


# ---- command line ----
def _cli(args, cwd):
    from siga_amd import host
    return subprocess.run([host.CLI_PATH] + args, capture_output=True, cwd=cwd)


@pytest.fixture(scope="module")
def indexed_tiny(tmp_path_factory):
    """`siga index` on tiny's reads -> the directory that holds tiny.fa and its index"""
    fx = fixture("tiny")
    d = str(tmp_path_factory.mktemp("preqc"))
    shutil.copy(fx.fa, os.path.join(d, "tiny.fa"))
    r = _cli(["index", "tiny.fa"], d)
    assert r.returncode == 0, r.stderr.decode()
    return d


def _distribution(hist):
    return [[c, v] for c, v in enumerate(hist) if v]


def test_cli_all_reads(indexed_tiny):
    fx = fixture("tiny")
    r = _cli(["preqc", "--all", "-k", "31", "tiny.fa"], indexed_tiny)
    assert r.returncode == 0, r.stderr.decode()
    got = json.loads(r.stdout.decode())["KmerDistribution"]
    want, n, L, windows = sc.spectrum(fx.fwd, fx.seqs, 31, 1025)
    assert (L, windows) == (24000, 11600)
    assert got == {"k": 31, "mode": "all", "samples": 400, "seed": 1, "strings": n, "bases": L, "windows": windows, "max_count": 1024,
                   "distribution": _distribution(want)}
    r = _cli(["preqc", "--all", "--kmer=31", "--max-count", "4", "-o", "tiny", "-t", "2", "tiny.fa"], indexed_tiny)
    assert r.returncode == 0, r.stderr.decode()
    got = json.loads(r.stdout.decode())["KmerDistribution"]
    want4 = sc.spectrum(fx.fwd, fx.seqs, 31, 5)[0]
    assert got["max_count"] == 4 and got["distribution"] == _distribution(want4)
    assert got["distribution"][-1] == [4, sum(want[4:])] and sum(want[5:]) > 0  # the last bin took the higher counts


def test_cli_sampled_rows(indexed_tiny):
    a = _cli(["preqc", "--samples", "500", "--seed", "7", "tiny.fa"], indexed_tiny)
    b = _cli(["preqc", "--samples", "500", "--seed", "7", "tiny.fa"], indexed_tiny)
    assert a.returncode == 0 and b.returncode == 0, a.stderr.decode() + b.stderr.decode()
    assert a.stdout == b.stdout
    got = json.loads(a.stdout.decode())["KmerDistribution"]
    assert got["samples"] == 500 and got["seed"] == 7 and got["mode"] == "sample" and got["k"] == 31
    assert sum(v for _, v in got["distribution"]) == got["windows"] > 0
    assert [c for c, _ in got["distribution"]] == sorted(c for c, _ in got["distribution"])
    other = json.loads(_cli(["preqc", "-n", "500", "--seed", "8", "tiny.fa"], indexed_tiny).stdout.decode())["KmerDistribution"]
    assert other["windows"] != got["windows"]


def test_cli_simple_is_not_built_and_help(indexed_tiny):
    r = _cli(["preqc", "--simple", "tiny.fa"], indexed_tiny)
    assert r.returncode == 255 and r.stdout == b"" and b"--simple" in r.stderr
    r = _cli(["preqc"], indexed_tiny)
    assert r.returncode == 0 and r.stdout.startswith(b"siga preqc [OPTION] READSFILE")
    assert b"preqc" in _cli([], indexed_tiny).stdout
    r = _cli(["preqc", "-o", "nothing", "tiny.fa"], indexed_tiny)
    assert r.returncode == 255 and r.stdout == b""
