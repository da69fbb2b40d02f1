"""The scratch sizes sigax_pileup_workspace and sigax_mmoverlap_workspace ask for, against the numbers recorded before the two
layouts got their common front and back from one seed_work (tests/golden/seeded_workspace.json: rows of n_reads, n_bases,
seed_length, seed_stride, hits_cap, then [rc, bytes] of the pile-up's and of the mismatch overlap's call, bytes 0xDEAD where the
call refused and wrote nothing).  A workspace sized by one build must serve the next, so no size may move.  Host arithmetic: no
GPU.  (sigax_reference_text_workspace needs an index: tests/test_gpu_overlap_correct.py.)"""
import ctypes as C
import json
import os

from siga_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "seeded_workspace.json")
N_READS = (0, 1, 7, 1000, 2 ** 20 + 1)
SEEDS = ((24, 12), (12, 1), (64, 64))
HITS_CAP = (0, 4096, 2 ** 30)
LOCATE_MAX_SLOTS = 0x7FFFFFFF * 256  # the hits one locate call walks (sigax_kernels.h)


def _bases(n):
    return (0, 150 * n, 2 ** 32 + 5)


def _sizes(L, n, nb, S, T, hits_cap):
    """-> [rc, bytes] of the two calls"""
    out = []
    for name, params in (("sigax_pileup_workspace", _lib.PileParams(seed_length=S, seed_stride=T)),
                         ("sigax_mmoverlap_workspace", _lib.MmoParams(40, seed_length=S, seed_stride=T))):
        wb = C.c_uint64(0xDEAD)
        out.append([getattr(L, name)(n, nb, C.byref(params), hits_cap, C.byref(wb)), wb.value])
    return out


def _grid():
    return [(n, nb, S, T, h) for n in N_READS for nb in _bases(n) for S, T in SEEDS for h in HITS_CAP]


def test_sizes_are_the_recorded_ones():
    L = _lib.lib()
    rows = json.load(open(GOLDEN))
    assert [tuple(r[:5]) for r in rows] == _grid()
    n_ok = 0
    for n, nb, S, T, h, pile, mmo in rows:
        assert _sizes(L, n, nb, S, T, h) == [pile, mmo], (n, nb, S, T, h)
        for rc, b in (pile, mmo):
            assert (rc == 0 and b % 16 == 0) or (rc == _lib.SIGAX_E_ARG and b == 0xDEAD), (n, nb, S, T, h)
        if pile[0] == 0:  # the overlap's own arrays lie between the seeds' parts: two u32 and one u64 a read, each rounded to 16
            up16 = lambda v: (v + 15) & ~15
            assert mmo[1] - pile[1] == 2 * up16(4 * n) + up16(8 * (n + 1)), (n, nb, S, T, h)
            n_ok += 1
    assert n_ok > len(rows) // 2


def test_refusals():
    L = _lib.lib()
    E = [_lib.SIGAX_E_ARG, 0xDEAD]  # refused, and nothing written
    # more seed slots than the 32 bits in which a hit names its seed: n_bases / T + n_reads
    assert _sizes(L, 5, 2 ** 32, 12, 1, 0) == [E, E]
    assert _sizes(L, 2 ** 20, 2 ** 32 - 2 ** 20, 12, 1, 4096) == [E, E]
    assert [r[0] for r in _sizes(L, 2 ** 20 - 1, 2 ** 32 - 2 ** 20, 12, 1, 4096)] == [0, 0]  # 2^32 - 1 slots: taken
    assert _sizes(L, 1, 24 * (2 ** 32 - 1), 24, 24, 0) == [E, E]
    # more hits than one locate call walks
    assert _sizes(L, 7, 1050, 24, 12, LOCATE_MAX_SLOTS + 1) == [E, E]
    assert [r[0] for r in _sizes(L, 7, 1050, 24, 12, LOCATE_MAX_SLOTS)] == [0, 0]
    for name, params in (("sigax_pileup_workspace", _lib.PileParams()), ("sigax_mmoverlap_workspace", _lib.MmoParams(40))):
        assert getattr(L, name)(7, 1050, C.byref(params), 4096, None) == _lib.SIGAX_E_ARG
