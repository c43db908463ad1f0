"""The host mirror of the verify job (pbs_verify_host.cpp, with the host inflater) under ASan + UBSan: `make sanitize-verify`
builds the stand-alone program tests/cpp/verify_sanitize.cpp and runs it.  No GPU; nothing loaded into
Python runs under a sanitizer."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_verify_host_code_under_sanitizers():
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "proxmox-backup_amd", "csrc"), "sanitize-verify"],
                       capture_output=True, text=True, timeout=900)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "verify_sanitize ok" in out, out[-4000:]
    assert "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
