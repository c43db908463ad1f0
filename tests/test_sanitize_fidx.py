"""The host code of the fixed path (pbs_fidx.cpp) under ASan + UBSan: `make sanitize-fidx` builds
the stand-alone program tests/cpp/fidx_sanitize.cpp and runs it.  No GPU; nothing loaded into
Python runs under a sanitizer."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_fidx_host_code_under_sanitizers():
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "proxmox-backup_amd", "csrc"), "sanitize-fidx"],
                       capture_output=True, text=True, timeout=900)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "fidx_sanitize ok" in out, out[-4000:]
    assert "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
