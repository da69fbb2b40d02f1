"""k_filter_extract_fast at every lane-group width and hand-off of launch_fx_stages (siga_amd/csrc/sigax_kernels.hip), on the
sets of tests/fx_width_cases.py: items of exactly 15 .. 17, 31 .. 33, 63 .. 65, 255 .. 257 and some 300 blocks, width from one
list only, two top-level blocks, containment blocks that count into the width, GFx::body_big items that run 31 rounds, that
leave through each of its exits (a branch, '$' below the top level, a range across a granule) and that finish.
tests/test_fx_width_cases.py proves on the CPU that the sets hold these items.

Parity is bit-exact against the oracle: hits and ASQG text, and through a batch object the blocks, substring flags and edge
records (three runs: the second uses the first's queue sizes, the third follows sigax_index_prepare_overlap).  That the lane
groups, and not the one-lane general kernel, did the work is read off sigax_stats.n_slow_reads, against bounds computed from
the reads.  test_forms_* re-run the batch tests in a child process under each switch that selects another instantiation of
the kernel or another finder in front of it."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import fx_width_cases as fw
from tests.fixtures import ROOT

pytestmark = pytest.mark.gpu

FORM = os.environ.get("SIGA_FXW_FORM", "")  # set in the child processes of test_forms_*: the switches' name
MODES = pytest.mark.parametrize("irr", [True, False], ids=["irreducible", "exhaustive"])
# sets in which nothing branches, no read is a substring and every range is one row: a lane group finishes every item it holds
PLAIN = ("stair_fwd", "stair_fwd250", "stair_rev", "stair_coin", "stair_both", "landings")
_PAIRS, _RUNS = {}, {}


def _pair(b):
    """one resident index per set for the whole module, reused by every run"""
    import siga_amd
    from siga_amd.overlap import name_ranks
    if b.name not in _PAIRS:
        pair = siga_amd.FMIndexPair.load(b.prefix)
        pair.set_reads(b.lens, name_ranks([n for n, _ in b.reads]))
        _PAIRS[b.name] = pair
    return _PAIRS[b.name]


def _one_run(L, bt, b, flags, irr, what):
    """upload, run, finish, download: everything against the oracle -> (stats, run info)"""
    from siga_amd import _lib
    from siga_amd.overlap import pack_reads
    from tests.test_gpu_tail_edges import _check_blocks, _check_edges, _download
    want = b.want(irr)
    want_edges = {"edges": b.edges(irr)}
    buf, offs = pack_reads(b.seqs)
    assert L.sigax_batch_upload(bt, buf, offs.ctypes.data, len(b.seqs), None) == 0, _lib.last_error()
    assert L.sigax_batch_run(bt, 0, b.m, flags, None) == 0, _lib.last_error()
    stats, ri = _lib.Stats(), _lib.RunInfo()
    assert L.sigax_batch_finish(bt, None, C.byref(stats)) == 0, _lib.last_error()
    assert L.sigax_batch_run_info(bt, C.byref(ri)) == 0, _lib.last_error()
    boffs, blocks, sub, eds = _download(L, bt)
    _check_blocks(boffs, blocks, sub, want, what)
    _check_edges(eds, want_edges, what)
    assert stats.n_blocks == len(want["blocks"]), what
    assert stats.n_edges == len(want_edges["edges"]), what
    assert stats.n_occ_find + stats.n_occ_extract == want["n_occ_min"], what
    return stats.as_dict(), ri.as_dict()


def _runs(name, irr):
    """three runs of one batch object over the set, checked; [(stats, run info)] kept for the path tests"""
    from siga_amd import _lib
    if (name, irr) not in _RUNS:
        b = fw.built(name)
        L = _lib.lib()
        pair = _pair(b)
        flags = (_lib.SIGAX_IRREDUCIBLE if irr else 0) | _lib.SIGAX_RC | _lib.SIGAX_EDGES
        bt = C.c_void_p()
        assert L.sigax_batch_create(pair.handle, len(b.seqs), int(b.lens.sum()), int(b.lens.max()), C.byref(bt)) == 0, _lib.last_error()
        out = []
        try:
            what = "%s irr=%d form=%s" % (name, irr, FORM or "default")
            out.append(_one_run(L, bt, b, flags, irr, what + " run 1"))
            out.append(_one_run(L, bt, b, flags, irr, what + " run 2 (queue hints)"))
            pair.prepare_overlap(b.m)
            out.append(_one_run(L, bt, b, flags, irr, what + " run 3 (prepared index)"))
        finally:
            L.sigax_batch_destroy(bt)
        print("%s: n_slow_reads %s of %d reads, bound %d, reruns %s, cap %d worst_cap %d" % (
            what, [s["n_slow_reads"] for s, _ in out], len(b.seqs), b.facts().slow_bound(irr), [r["reruns"] for _, r in out],
            out[0][1]["cap"], out[0][1]["worst_cap"]))
        _RUNS[(name, irr)] = out
    return _RUNS[(name, irr)]


# ---- parity ---------------------------------------------------------------------------------------------------------------
@MODES
@pytest.mark.parametrize("name", fw.NAMES)
def test_hits_and_asqg_text(name, irr, tmp_path):
    import siga_amd
    from siga_amd.overlap import format_hits
    b = fw.built(name)
    want_asqg, want_hits = b.oracle_text(irr)
    text, res = siga_amd.OverlapBuilder(_pair(b), b.prefix, irreducible=irr, rc=True).build(b.fa, b.m)
    got_hits = format_hits(res)
    if got_hits != want_hits:
        gl, wl = got_hits.split("\n"), want_hits.split("\n")
        bad = [i for i in range(min(len(gl), len(wl))) if gl[i] != wl[i]]
        f = b.facts()
        raise AssertionError("%s irr=%d: %d reads differ; first: read %d, blocks per side %s\n got  %s\n want %s" % (
            name, irr, len(bad), bad[0], f.T[bad[0]].tolist(), gl[bad[0]][:400], wl[bad[0]][:400]))
    assert text == want_asqg
    s = res["stats"]
    assert s["n_occ_find"] + s["n_occ_extract"] == b.want(irr)["n_occ_min"]


@MODES
@pytest.mark.parametrize("name", fw.NAMES)
def test_batch_blocks_flags_and_edges(name, irr):
    """blocks, substring flags, edge records, n_blocks and the rank evaluations of three runs of one batch object"""
    runs = _runs(name, irr)
    ri = runs[2][1]
    if os.environ.get("SIGAX_ROWEND") != "0":
        # on the prepared, reused index the text forms of the kernel are what ran (they need a row table or direct maps)
        assert ri["row_text"] or ri["row_bits"] or ri["row_direct"], ri
    if os.environ.get("SIGAX_CAND_CAP") == "2" and irr and name.startswith("stair"):
        # two candidate slots per chain on an index that has seen no run yet (the irreducible case is the set's first in the
        # child process): the first run repeats itself with what its chains reported -- in stair_fwd, whose chains are as
        # long as chains get, with the largest arena
        assert runs[0][1]["reruns"] >= 1, runs[0][1]
        assert name != "stair_fwd" or runs[0][1]["cap"] == runs[0][1]["worst_cap"], runs[0][1]


# ---- path evidence: bounds from the reads (tests/fx_width_cases.py), never from a GPU run ---------------------------------
@MODES
@pytest.mark.parametrize("name", fw.NAMES)
def test_too_wide_items_go_to_the_general_kernel(name, irr):
    """no lane group holds an item of more than FX_BIGCAP blocks (more than 64 in exhaustive mode): at least the reads with
    such a side are queued for the general kernel.  In every form."""
    f = fw.built(name).facts()
    for stats, _ in _runs(name, irr):
        assert stats["n_slow_reads"] >= f.slow_bound(irr), (stats["n_slow_reads"], f.slow_bound(irr))


@pytest.mark.parametrize("name", PLAIN)
def test_plain_items_finish_on_lane_groups(name):
    """Irreducible mode, sets without branches, substring reads or ranges of several rows: the general kernel gets the reads
    with a side over FX_BIGCAP blocks and no other -- none at all of the staircase of 250 (widest side: 251).  An item of
    exactly FX_BIGCAP blocks stays (stair_fwd, stair_coin, stair_both and landings hold some).  Asserted of the default form;
    the switches of test_forms_* may route otherwise."""
    f = fw.built(name).facts()
    if name == "stair_fwd250":
        assert f.slow_bound(True) == 0
    got = [s["n_slow_reads"] for s, _ in _runs(name, True)]
    if not FORM:
        assert got == 3 * [f.slow_bound(True)], (got, f.slow_bound(True))


@pytest.mark.parametrize("name", ["private8", "private40"])
def test_private_variants_against_the_group_slots(name):
    """V reads split off into groups of their own inside a landing item of at most 64 blocks: 8 fit the FX_NSLOT group slots,
    40 do not and the item is redone by the general kernel."""
    b = fw.built(name)
    f = b.facts()
    assert f.T[b.case.landing_reads[0]].max() <= 64 and f.slow_bound(True) == 0
    got = [s["n_slow_reads"] for s, _ in _runs(name, True)]
    if b.case.private > fw.GROUP_SLOTS:
        assert min(got) >= 1, got
    elif not FORM:
        assert max(got) <= f.slow_bound(True), got


@pytest.mark.parametrize("name", ["landings_hap", "landings_ragged", "stair_dup"])
def test_body_big_exits_reach_the_general_kernel(name):
    """items of 65..256 blocks that branch (landings_hap), meet '$' below the top level (landings_ragged) or hold a range across
    two granules (landings_ragged, stair_dup) cannot finish in GFx::body_big; the narrow items of the same set stay on lane
    groups"""
    b = fw.built(name)
    assert b.facts().big_items().any()
    for stats, _ in _runs(name, True):
        assert 1 <= stats["n_slow_reads"] < len(b.seqs), stats["n_slow_reads"]


# ---- forms ----------------------------------------------------------------------------------------------------------------
def _child(form, env_extra, select="batch or general or plain or private or exits"):
    """this file's batch and path tests in a child process under `env_extra` (the library reads its switches once)"""
    env = dict(os.environ, SIGA_FXW_FORM=form, **env_extra)
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-s", os.path.abspath(__file__), "-k", "not forms and (%s)" % select],
                       cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    summary = r.stdout.strip().split("\n")[-1]
    assert " passed" in summary and "skipped" not in summary, summary
    return r.stdout


def _super12():
    from siga_amd import build as sbuild
    return sbuild.build_libsigax(out=os.path.join(ROOT, "build", "libsigax_super12.so"), defines=("SIGAX_SUPER_SHIFT=12",))


def test_forms_wide_positions():
    _child("wide", {"SIGAX_FORCE_WIDE": "1"})


def test_forms_wide_positions_many_superblocks():
    _child("wide_super12", {"SIGAX_FORCE_WIDE": "1", "SIGAX_LIB": _super12()})


def test_forms_one_step():
    """modes 2/4 of the kernel"""
    _child("one_step", {"SIGAX_TWO_STEP": "0"})


def test_forms_without_row_tables():
    """modes 1/3"""
    _child("no_rowend", {"SIGAX_ROWEND": "0"})


def test_forms_without_lookahead():
    _child("no_lookahead", {"SIGAX_LOOKAHEAD": "0"})


def test_forms_sixteen_lane_groups():
    """the 16/17 boundary and kNSlot = 16"""
    _child("fx16", {"SIGAX_FX_16": "1"})


def test_forms_one_workgroup():
    _child("grid1", {"SIGAX_FX_GRID": "1"})


def test_forms_no_lean():
    _child("no_lean", {"SIGAX_FX_NO_LEAN": "1"})


def test_forms_skip_strict():
    """the a.no_lean route: the branching launches take their items from the read range"""
    _child("skip_strict", {"SIGAX_FX_SKIP_STRICT": "1"})


def test_forms_candidate_slots_overflow():
    out = _child("cand_cap2", {"SIGAX_CAND_CAP": "2"})
    assert "reruns [" in out


def test_forms_regrowing_pool_and_arena():
    """the general kernel's pool and the final-block arena regrow while items of 257 blocks and more are in it"""
    _child("regrow", {"SIGAX_TEST_POOL_CAP": "24", "SIGAX_TEST_FIN_CAP": "64"})
