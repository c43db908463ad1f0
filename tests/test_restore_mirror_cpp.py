"""pbs::DynamicIndexReader of the C++ host mirror (host/pbs_chunker.hpp): compiles
tests/cpp/restore_mirror_main.cpp against the C ABI and reads a built .didx file back.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import rplanted as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "restore_mirror_main.cpp")
LIBDIR = os.path.join(ROOT, "proxmox-backup_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory, pbschunk):
    pbschunk.lib()  # (the library is built)
    path = str(tmp_path_factory.mktemp("restore_mirror") / "restore_mirror")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "proxmox-backup_amd", "host"), SRC, "-L", LIBDIR,
                    "-lpbschunk", f"-Wl,-rpath,{LIBDIR}", "-o", path], check=True)
    return path


def test_reader_mirror(exe, pbschunk, tmp_path):
    ends, digests = rc.make_index(9, seed=4, zero_runs=True)
    uuid = bytes(range(16))
    image, csum = pbschunk.didx_build(ends, digests, uuid, 1700000000)
    path = tmp_path / "x.didx"
    path.write_bytes(image)
    py = [int(e) for e in ends]
    offsets = sorted({0} | {o for e in py for o in (e - 1, e, e + 1) if o >= 0})
    r = subprocess.run([exe, str(path)] + [str(o) for o in offsets], capture_output=True, text=True, check=True)
    lines = dict((ln.split(" ", 1) + [""])[:2] for ln in r.stdout.splitlines())
    assert (int(lines["count"]), int(lines["bytes"]), int(lines["size"]), int(lines["ctime"])) == (9, py[-1], len(image), 1700000000)
    assert lines["uuid"] == uuid.hex() and lines["index_csum"] == csum.hex() == lines["computed_csum"]
    assert int(lines["csum_end"]) == py[-1]
    for i in range(9):
        start, end, dig = lines[f"chunk{i}"].split()
        assert (int(start), int(end), dig) == (py[i - 1] if i else 0, py[i], digests[i].tobytes().hex())
    for o in offsets:
        want = rc.ref_chunk_from_offset(py, o)
        assert lines[f"offset{o}"] == ("none" if want is None else f"{want[0]} {want[1]}"), o
    # a flipped entry byte: the computed checksum moves, the header's stays
    bad = bytearray(image)
    bad[4096 + 40 * 3 + 20] ^= 1
    path.write_bytes(bytes(bad))
    lines = dict((ln.split(" ", 1) + [""])[:2] for ln in subprocess.run([exe, str(path)], capture_output=True, text=True,
                                                                      check=True).stdout.splitlines())
    assert lines["index_csum"] == csum.hex() != lines["computed_csum"]
    # what the reader refuses
    for img in (image[:4095], image + b"\0", b"\0" + image[1:]):
        path.write_bytes(img)
        r = subprocess.run([exe, str(path)], capture_output=True, text=True)
        assert r.returncode == 3 and r.stdout.startswith("error"), r.stdout
    assert np.array_equal(pbschunk.DynamicIndexReader(image).ends, ends)
