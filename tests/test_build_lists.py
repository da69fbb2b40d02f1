"""The build lists of siga_amd/build.py keep up with siga_amd/csrc: a source missing from SOURCES is not linked, a header
missing from HEADERS does not make an old library stale, and the three kernels whose traffic figures bench.py keys to a hash
of sigax_kernels.hip are defined in that file."""
import os
import re

from siga_amd import build as sbuild

CSRC = sbuild.CSRC


def _files(*suffixes):
    return sorted(f for f in os.listdir(CSRC) if f.endswith(suffixes))


def test_every_source_is_compiled_exactly_once():
    assert sorted(sbuild.SOURCES) == _files(".hip", ".cpp"), "SOURCES of siga_amd/build.py and the .hip/.cpp files of csrc differ"
    assert len(set(sbuild.SOURCES)) == len(sbuild.SOURCES)


def test_every_header_makes_the_library_stale():
    missing = [h for h in _files(".h") if h not in sbuild.HEADERS]
    assert not missing, "in csrc, not in HEADERS of siga_amd/build.py: %s" % missing


def test_every_local_include_names_a_listed_header():
    listed = {os.path.normpath(h if os.path.isabs(h) else os.path.join(CSRC, h)) for h in sbuild.HEADERS}
    seen = 0
    for f in _files(".hip", ".cpp", ".h"):
        with open(os.path.join(CSRC, f), errors="replace") as fh:
            for inc in re.findall(r'^\s*#\s*include\s+"([^"]+)"', fh.read(), re.M):
                seen += 1
                assert os.path.normpath(os.path.join(CSRC, inc)) in listed, "%s includes %s, which HEADERS does not list" % (f, inc)
    assert seen > 30, seen  # the scan sees the includes


def test_the_hashed_file_holds_the_kernels_whose_traffic_is_keyed_to_it():
    """bench.py's kernels_sha() hashes sigax_kernels.hip (and fm_layout.h) and keys the traffic figures of k_find,
    k_filter_extract_fast and k_correct in profiles/traffic.json to that hash: a kernel defined elsewhere would keep a figure
    that its own source no longer vouches for."""
    with open(os.path.join(CSRC, "sigax_kernels.hip")) as fh:
        src = fh.read()
    for k in ("k_find_n", "k_filter_extract_fast", "k_correct"):
        assert re.search(r"__global__[^;{]*\bvoid %s\(\w+ A\) \{" % k, src), "%s is not defined in sigax_kernels.hip" % k
