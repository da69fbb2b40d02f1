"""The scratch sizes the five sigax_unitigs*_workspace calls ask for, against the numbers recorded before the five layouts became one
(tests/golden/unitig_workspace.json: rows of n_reads, n_edges, want_graph, careful, then the unitig, trim, prune, chimeric and bubble
call's bytes).  A call at one level may run as a lower one over the same scratch, so no size may move.  Host arithmetic: no GPU."""
import ctypes as C
import json
import os

from siga_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "unitig_workspace.json")
N_READS = (0, 1, 7, 8, 9, 1000, 2 ** 20 + 1, 2 ** 31 - 1)
N_EDGES = (0, 1, 5, 2 ** 20, 2 ** 32)


def _sizes(L, n, ne, graph, careful):
    """-> [rc, bytes] of the five calls, bottom level first"""
    out = []
    for name, extra in (("sigax_unitigs_workspace", ()), ("sigax_unitigs_trim_workspace", (graph,)), ("sigax_unitigs_prune_workspace", (graph, careful)),
                        ("sigax_unitigs_chimeric_workspace", (graph, careful)), ("sigax_unitigs_bubble_workspace", (graph, careful))):
        wb = C.c_uint64(0xDEAD)
        out.append([getattr(L, name)(n, ne, *extra, C.byref(wb)), wb.value])
    return out


def test_sizes_are_the_recorded_ones():
    L = _lib.lib()
    rows = json.load(open(GOLDEN))
    assert [tuple(r[:4]) for r in rows] == [(n, ne, g, c) for n in N_READS for ne in N_EDGES for g in (0, 1) for c in (0, 1)]
    for n, ne, g, c, *want in rows:
        assert _sizes(L, n, ne, g, c) == [[0, w] for w in want], (n, ne, g, c)
        assert want == sorted(want) and all(w % 16 == 0 for w in want), (n, ne, g, c)  # each level holds the one below it


def test_refusals():
    L = _lib.lib()
    E = _lib.SIGAX_E_ARG
    for n, ne in ((2 ** 31, 0), (2 ** 31, 5), (10, 2 ** 32 + 1), (2 ** 31 - 1, 2 ** 32 + 1)):
        for g in (0, 1):
            assert _sizes(L, n, ne, g, g) == [[E, 0xDEAD]] * 5, (n, ne)  # refused, and nothing written
    assert L.sigax_unitigs_workspace(10, 100, None) == E
    assert L.sigax_unitigs_trim_workspace(10, 100, 1, None) == E
    for name in ("prune", "chimeric", "bubble"):
        assert getattr(L, "sigax_unitigs_%s_workspace" % name)(10, 100, 1, 1, None) == E
