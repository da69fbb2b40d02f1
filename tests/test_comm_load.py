"""How siga_amd/csrc/sigax_comm.cpp binds RCCL (no GPU needed): SIGAX_RCCL_LIB=<path> opens exactly that library, and a library
that is not there, or that lacks entry points, is SIGAX_E_DEVICE with the cause in sigax_last_error() -- the return code
bench.py's fall-back to torch.distributed relies on -- every time it is asked, not a crash.  The library tries once per
process, so every case is a fresh child; the child loads libsigax.so alone (no torch)."""
import os
import subprocess
import sys

from tests.fixtures import ROOT

STANDIN_SRC = os.path.join(ROOT, "tests", "rccl_standin.cpp")


def build_standin(one_symbol=False):
    """tests/rccl_standin.cpp -> build/librccl_standin.so, the stand-in for RCCL whose ranks are threads of one process
    (one_symbol: the variant that exports ncclGetUniqueId alone); linked against the HIP runtime the way libsigax.so is"""
    from siga_amd import build as sbuild
    out = os.path.join(ROOT, "build", "librccl_standin_one.so" if one_symbol else "librccl_standin.so")
    if os.path.exists(out) and os.path.getmtime(out) >= os.path.getmtime(STANDIN_SRC):
        return out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    tmp = "%s.%d.tmp" % (out, os.getpid())
    cmd = [sbuild.HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-x", "hip", "-o", tmp]
    subprocess.check_call(cmd + (["-DRCCL_STANDIN_ONE_SYMBOL"] if one_symbol else []) + [STANDIN_SRC])
    os.replace(tmp, out)
    return out


CHILD = r"""
import ctypes as C, json, sys
L = C.CDLL(sys.argv[1])
L.sigax_last_error.restype = C.c_char_p
L.sigax_comm_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
out = []
idb = (C.c_uint8 * 128)()
for what in sys.argv[2:]:
    if what == "id":
        rc = L.sigax_comm_unique_id(idb)
        out.append([rc, L.sigax_last_error().decode(errors="replace"), None])
    else:
        comm = C.c_void_p(0xDEAD0)
        rc = L.sigax_comm_create(0, 0, 2, idb, C.byref(comm))
        out.append([rc, L.sigax_last_error().decode(errors="replace"), comm.value])
print(json.dumps(out))
"""


def _ask(rccl_lib, calls):
    """a fresh process with SIGAX_RCCL_LIB set makes `calls` ("id" = sigax_comm_unique_id, "create" = sigax_comm_create) ->
    [code, error text, *out] per call; it must end by itself with status 0"""
    import json
    from siga_amd import _lib
    r = subprocess.run([sys.executable, "-c", CHILD, _lib.LIB_PATH] + list(calls), env=dict(os.environ, SIGAX_RCCL_LIB=rccl_lib),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, "status %d\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return json.loads(r.stdout.strip().split("\n")[-1])


E_DEVICE = -3
MISSING = "/nonexistent/librccl.so"


def test_a_library_that_is_not_there_is_a_code_with_the_path_in_the_text():
    first, second = _ask(MISSING, ["id", "id"])
    assert first[0] == E_DEVICE and MISSING in first[1] and "RCCL unavailable" in first[1], first
    assert second[0] == E_DEVICE and MISSING in second[1], second  # asked again: the same answer, not a second attempt


def test_a_library_without_the_entry_points_is_refused():
    lib = build_standin(one_symbol=True)
    exported = subprocess.check_output(["nm", "-D", "--defined-only", lib]).decode()
    assert " ncclGetUniqueId" in exported and "ncclSend" not in exported and "ncclCommInitRank" not in exported
    first, second = _ask(lib, ["id", "id"])
    for got in (first, second):
        assert got[0] == E_DEVICE and "lacks one of the nccl* entry points" in got[1] and lib in got[1], got


def test_comm_create_without_rccl_is_a_code_and_leaves_out_null():
    for lib, text in ((MISSING, MISSING), (build_standin(one_symbol=True), "lacks one of the nccl* entry points")):
        for calls in (["create", "create"], ["id", "create"]):
            for call, got in zip(calls, _ask(lib, calls)):
                assert got[0] == E_DEVICE and text in got[1], (lib, calls, got)
                assert call == "id" or got[2] is None, (lib, calls, got)  # *out, 0xDEAD0 before the call, is NULL after it


def test_the_stand_in_exports_what_sigax_comm_binds():
    """the nine names rccl_load() asks for (siga_amd/csrc/sigax_comm.cpp) are the stand-in's exports"""
    import re
    src = open(os.path.join(ROOT, "siga_amd", "csrc", "sigax_comm.cpp")).read()
    bound = set(re.findall(r'sym\("(nccl[A-Za-z]+)"\)', src))
    assert len(bound) == 9, sorted(bound)
    exported = subprocess.check_output(["nm", "-D", "--defined-only", build_standin()]).decode()
    assert bound <= set(re.findall(r" T (nccl[A-Za-z]+)", exported)), exported
