"""The zstd format code the GPU inflater shares with its host mirror (csrc/zstd_dec.h) under
AddressSanitizer + UndefinedBehaviorSanitizer: `make -C proxmox-backup_amd/csrc
sanitize-inflate` builds the stand-alone tests/cpp/inflate_sanitize.cpp with
pbs_inflate_host.cpp and runs it over the whole corpus of tests/iplanted.py, bad frames
included, written to a temporary directory; any sanitizer report fails the run
(halt_on_error).  No Python is loaded into the checked program and no device is involved."""
import os
import shutil
import subprocess

import pytest

import iplanted as ip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_inflate_mirror_under_sanitizers(tmp_path):
    c = ip.corpus()
    items = c["good"] + c["bad"]
    for i, it in enumerate(items):
        (tmp_path / f"{i:04d}_{it.cap}.zst").write_bytes(it.frame)
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "proxmox-backup_amd", "csrc"), "sanitize-inflate",
                        f"INFLATE_CORPUS={tmp_path}"], capture_output=True, text=True, timeout=900)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert f"inflate_sanitize ok (0 failures): {len(items)} frames" in out, out[-4000:]
    assert "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
