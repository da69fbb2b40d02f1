"""tests/test_gpu_spectrum.py again in the forms of the index that the defaults do not take (the mechanism of
tests/test_gpu_wide.py: the library and its switches are chosen at load time, so each form is a subprocess): 64-bit
positions, those with a superblock every 2^12 symbols (ragged_n has three), and one-step granules in place of two-step lines.
The command-line cases stay with the default form: the CLI loads the product library whatever SIGAX_LIB says."""
import os
import subprocess
import sys

import pytest

from tests.fixtures import ROOT

pytestmark = pytest.mark.gpu


def _rerun(env_extra):
    env = dict(os.environ, **env_extra)
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", os.path.join(ROOT, "tests", "test_gpu_spectrum.py"), "-k", "not cli"],
                       cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]


def test_spectrum_wide_positions():
    _rerun({"SIGAX_FORCE_WIDE": "1"})


def test_spectrum_wide_positions_small_superblocks():
    lib = os.path.join(ROOT, "build", "libsigax_super12.so")
    assert os.path.exists(lib)
    _rerun({"SIGAX_FORCE_WIDE": "1", "SIGAX_LIB": lib})


def test_spectrum_without_two_step_tables():
    _rerun({"SIGAX_TWO_STEP": "0"})
    _rerun({"SIGAX_TWO_STEP": "0", "SIGAX_FORCE_WIDE": "1"})
