"""The host mirror of the backup session (pbs_backup_host.cpp with backup_common.h, over the verify mirror's blob
verdict, the host inflater and both index writers) under ASan + UBSan: `make sanitize-backup` builds the stand-alone
program tests/cpp/backup_sanitize.cpp and runs it.  No GPU; nothing loaded into Python runs under a sanitizer."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_backup_host_code_under_sanitizers():
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "proxmox-backup_amd", "csrc"), "sanitize-backup"],
                       capture_output=True, text=True, timeout=900)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "backup_sanitize ok" in out, out[-4000:]
    assert "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
