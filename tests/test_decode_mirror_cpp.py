"""The read side of the C++ host mirror (pbs::blob_decode_host, pbs::CryptConfig::decrypt_host,
host/pbs_chunker.hpp): compiles against the C ABI and gives the reference's outcome for an
intact and a corrupted blob of the plain and the encrypted kind.  No GPU."""
import os
import subprocess

import pytest

import dplanted as d
import gplanted as g

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "decode_mirror_main.cpp")
LIBDIR = os.path.join(ROOT, "proxmox-backup_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory, pbschunk):
    pbschunk.lib()  # (the library is built)
    path = str(tmp_path_factory.mktemp("decode_mirror") / "decode_mirror")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "proxmox-backup_amd", "host"), SRC, "-L", LIBDIR,
                    "-lpbschunk", f"-Wl,-rpath,{LIBDIR}", "-o", path], check=True)
    return path


def _items(oracle):
    h = {it.label: it for it in d.corrupt_items(oracle)}
    a = d.stream("a")
    return [a[0], a[77], h["h/kind0/len12-empty"], h["h/kind0/wrong-digest"], h["h/kind0/wrong-size"],
            h["h/kind2/tag15"], h["h/kind2/len30"], h["h/kind0/magic-bit"], h["h/kind2/crc-bit"], h["h/kind0/len0"]]


def test_decode_mirror(exe, oracle):
    for it in _items(oracle):
        r = subprocess.run([exe, it.blob.hex() or "-", it.digest.hex(), str(it.size)], capture_output=True, text=True,
                           check=True)
        lines = dict((ln.split(" ", 1) + [""])[:2] for ln in r.stdout.splitlines())
        st, _ = d.reference_outcome(oracle, it, g.KEY1)
        assert st == it.status
        assert (int(lines["kind"]), int(lines["status"])) == (it.kind, it.status), it.label
        assert lines["payload"].strip() == it.payload.hex(), it.label
        if it.kind in (2, 3):  # (opened again without a config, digest or size)
            assert int(lines["status_without_config"]) == d.reference_outcome(oracle, it, None)[0], it.label
        assert lines["roundtrip"].strip() == "1" and lines["forged"].strip() == "1"
