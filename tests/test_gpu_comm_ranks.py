"""The multi-rank exchange step (siga_amd/csrc/sigax_comm.cpp: sigax_gather_counts / sigax_gather_edges) with 2, 3 and 8 ranks
on ONE GPU.  RCCL is replaced by a stand-in (tests/rccl_standin.cpp, bound through SIGAX_RCCL_LIB) whose ranks are threads of
one process, so what the one-rank test of tests/test_gpu_multi.py cannot reach runs here: Send / Recv pairs, the root's
displacements (`at += counts[r]`, the root's own share behind the ranks before it), a root other than rank 0, empty shares on
either side of a pair -- and the composition: W ranks' shards of a read set, gathered and, for key shards, put back in read
order, against the one-batch run's bytes and the oracle's ASQG.  Real RCCL between GPUs stays with the two_gpus tests of
tests/test_gpu_multi.py.

Every test body runs in one child process (tests/comm_ranks_child.py) because the library binds RCCL once per process; the
child is the only process with the GPU open, and every wait in it has a deadline (20 s in the stand-in, 120 s for a rank's
thread, the subprocess timeout below), so a wrong pairing fails instead of hanging."""
import os
import subprocess
import sys

import pytest

from tests.fixtures import ROOT
from tests.test_comm_load import build_standin

pytestmark = pytest.mark.gpu


def _child(group, W, *more):
    env = dict(os.environ, SIGAX_RCCL_LIB=build_standin())
    r = subprocess.run([sys.executable, "-m", "tests.comm_ranks_child", group, str(W)] + [str(x) for x in more], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, "status %d\n%s\n%s" % (r.returncode, r.stdout[-4000:], r.stderr[-3000:])
    return r.stdout


@pytest.mark.parametrize("W", [2, 3, 8])
def test_synthetic_records_gathered_from_every_rank(W):
    """Roots first, middle and last; per-rank counts from (0, 1, 7, 1000, 12345) with the root's share empty, a sender's share
    empty, all empty and one rank holding everything; each case twice on the same communicators, every rank on a stream of its
    own with its records uploaded asynchronously just before the calls (the second time between the two calls).  Every rank's
    counts[] is the full list; the root's buffer is the ranks' records in rank order, byte for byte, and the 64 bytes of 0xEE
    behind them are untouched."""
    assert "synthetic: W %d" % W in _child("synthetic", W)


def test_refusals_and_disagreeing_counts_with_three_ranks():
    """Argument errors on every rank of a world of three, each refused before anything is posted (a gather right after them
    pairs up): root outside the world, NULL d_local with records to send, NULL d_out on the root.  Then one sender's counts[]
    says 9 where the root's says 7: both get SIGAX_E_DEVICE from the stand-in's mismatch check, the third rank's pair is
    served, and the child ends by itself."""
    assert "refusals: W 3" in _child("refusals", 3)


@pytest.mark.parametrize("W", [2, 3, 8])
def test_shards_gathered_give_the_one_batch_bytes(W, tmp_path):
    """toy (m = 45), ragged (m = 15), dup (m = 8) and make_case(8) of tests/test_gpu_random.py, sharded over W ranks by
    contiguous file ranges (under read_base) and by locality-key ranges (under read ids).  The overlap runs happen rank by rank
    on the main thread and stay in device memory; the exchange runs on W threads; on the root the gathered records (key
    shards: after sigax_edges_restore_order, flags through sigax_flags_by_read_id) and the substring flags are the one-batch
    run's bytes, and the ASQG text formatted from them is the oracle's."""
    out = _child("end_to_end", W, tmp_path)
    for tag in ("toy", "ragged", "dup", "random8"):
        assert "end to end: %s, W %d" % (tag, W) in out
