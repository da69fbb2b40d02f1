"""The documentation keeps up with the native library: every SIGAX_* switch it reads is listed in INTEGRATION.md."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_sigax_switch_is_documented():
    csrc = os.path.join(ROOT, "siga_amd", "csrc")
    names = set()
    for f in sorted(os.listdir(csrc)):
        with open(os.path.join(csrc, f), errors="replace") as fh:
            names.update(re.findall(r'getenv\("(SIGAX_[A-Z0-9_]+)"\)', fh.read()))
    assert "SIGAX_VERBOSE" in names and "SIGAX_FX_16" in names, sorted(names)  # the scan sees the settings and the launch code
    with open(os.path.join(ROOT, "INTEGRATION.md")) as fh:
        doc = fh.read()
    missing = sorted(n for n in names if not re.search(r"`%s[`=]" % n, doc))
    assert not missing, "read by libsigax.so, not listed in INTEGRATION.md: %s" % missing
