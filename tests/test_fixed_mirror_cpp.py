"""pbs::FixedChunkStream, pbs::FixedIndexReader and pbs::FixedIndexWriter of the C++ host mirror
(host/pbs_chunker.hpp): compiles tests/cpp/fixed_mirror_main.cpp against the C ABI.  No GPU."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import fplanted as f

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "fixed_mirror_main.cpp")
LIBDIR = os.path.join(ROOT, "proxmox-backup_amd", "csrc")
UUID = bytes(range(16))


@pytest.fixture(scope="module")
def exe(tmp_path_factory, pbschunk):
    pbschunk.lib()  # (the library is built)
    path = str(tmp_path_factory.mktemp("fixed_mirror") / "fixed_mirror")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "include"),
                    "-I", os.path.join(ROOT, "proxmox-backup_amd", "host"), SRC, "-L", LIBDIR,
                    "-lpbschunk", f"-Wl,-rpath,{LIBDIR}", "-o", path], check=True)
    return path


def run(exe, *args, code=0):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == code, (r.returncode, r.stdout, r.stderr)
    return dict((ln.split(" ", 1) + [""])[:2] for ln in r.stdout.splitlines())


def test_reader_mirror(exe, pbschunk, tmp_path):
    c, size = 4096, 5 * 4096 + 1
    dig = f.digests_of(6, 9)
    image = f.model_image(dig, size, c, UUID, 1700000000)
    path = tmp_path / "x.fidx"
    path.write_bytes(image)
    offsets = [0, c - 1, c, size - 1, size, size + 1]
    lines = run(exe, "read", path, *offsets)
    assert (int(lines["count"]), int(lines["bytes"]), int(lines["chunk_size"]), int(lines["ctime"])) == (6, size, c, 1700000000)
    csum = hashlib.sha256(dig.tobytes()).hexdigest()
    assert lines["uuid"] == UUID.hex() and lines["index_csum"] == csum == lines["computed_csum"]
    assert int(lines["csum_end"]) == size and lines["past"] == "0 0"
    for i in range(6):
        start, end, d = lines[f"chunk{i}"].split()
        assert (int(start), int(end), d) == (i * c, min((i + 1) * c, size), dig[i].tobytes().hex())
    for o in offsets:
        assert lines[f"offset{o}"] == ("none" if o >= size else f"{o // c} {o % c}"), o
    # what the reader refuses
    three = f.model_image(f.digests_of(f.count(size, 3)), size, 3, UUID, 0)
    for img in (image[:4095], image + b"\0", b"\0" + image[1:], image[:-32], three):
        path.write_bytes(img)
        assert run(exe, "read", path, code=3).get("error") is not None


@pytest.mark.parametrize("piece", (1, 7, 4095, 4096, 4097, 1 << 20))
def test_chunk_stream_mirror(exe, pbschunk, tmp_path, piece):
    c = 4096
    for total in (0, c, 3 * c + 5):
        data = np.random.default_rng([11, total]).integers(0, 256, total, dtype=np.uint8).tobytes()
        path = tmp_path / f"data{total}"
        path.write_bytes(data)
        lines = run(exe, "stream", c, piece, path)
        want = list(pbschunk.FixedChunkStream(c).chunks([data]))
        assert int(lines["chunks"]) == len(want) == f.count(total, c)
        for k, ch in enumerate(want):
            assert lines[f"chunk{k}"] == f"{len(ch)} {hashlib.sha256(ch).hexdigest()}"


def test_writer_mirror(exe, pbschunk, tmp_path):
    c, size = 4096, 7 * 4096 + 33
    dig = f.digests_of(8, 2)
    image = f.model_image(dig, size, c, UUID, 42)
    src, out = tmp_path / "in.fidx", tmp_path / "out.fidx"
    src.write_bytes(image)
    lines = run(exe, "write", src, out)
    csum = hashlib.sha256(dig.tobytes()).hexdigest()
    assert lines["csum"] == csum == lines["clone_csum"]
    assert lines["errors"] == "15" and lines["same"] == "1"  # out of range, bad chunk, double close, count mismatch
    assert out.read_bytes() == image
