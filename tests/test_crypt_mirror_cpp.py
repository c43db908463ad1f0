"""The crypt wrapper of the C++ host mirror (pbs::CryptConfig, host/pbs_chunker.hpp):
compiles against the C ABI and gives the reference's id_key, ciphertext and tag.  No GPU."""
import os
import subprocess

import pytest

import aesgcm_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "crypt_mirror_main.cpp")
LIBDIR = os.path.join(ROOT, "proxmox-backup_amd", "csrc")


@pytest.mark.parametrize("n", [0, 77, 4105])
def test_crypt_mirror(tmp_path, pbschunk, n):
    pbschunk.lib()  # (the library is built)
    exe = str(tmp_path / "crypt_mirror")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "proxmox-backup_amd", "host"), SRC, "-L", LIBDIR,
                    "-lpbschunk", f"-Wl,-rpath,{LIBDIR}", "-o", exe], check=True)
    r = subprocess.run([exe, str(n)], capture_output=True, text=True, check=True)
    lines = dict((ln.split(" ", 1) + [""])[:2] for ln in r.stdout.splitlines())
    key = bytes([1]) * 32
    ct, tag = aesgcm_ref.cipher(key).encrypt(bytes(range(0x40, 0x50)), bytes(i % 255 for i in range(n)))
    assert lines["id_key"].strip() == aesgcm_ref.id_key(key).hex()
    assert lines["ct"].strip() == ct.hex() and lines["tag"].strip() == tag.hex()
