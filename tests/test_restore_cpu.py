"""The host side of the restore path (include/pbs_restore.h, csrc/pbs_didx_read.cpp): the index
reader against the builder, read_didx and hashlib; chunk_from_offset against a restatement of
the reference's recursion (dynamic_index.rs:172-195, :258-274); the lookup mirror against a
dict.  No GPU."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

from rplanted import (MISSING, csum_of, make_index, model_lookup, planted_lookup_sets, ref_chunk_from_offset)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, CAPACITY = -6, -5


# ---- pbs_didx_parse ---------------------------------------------------------------------------

@pytest.mark.parametrize("n,zero_runs", [(0, False), (1, False), (1000, False), (12, True)])
def test_parse_inverts_build(pbschunk, n, zero_runs):
    ends, digests = make_index(n, zero_runs=zero_runs)
    if zero_runs:
        assert (np.diff(ends) == 0).any()
    uuid = bytes(range(100, 116))
    image, csum = pbschunk.didx_build(ends, digests, uuid, -1234567890123)
    assert pbschunk.didx_count(len(image)) == n
    got = pbschunk.didx_parse(image)
    ref = pbschunk.read_didx(image)
    assert got[0] == ref[0] == uuid and got[1] == ref[1] == -1234567890123 and got[2] == ref[2] == csum
    assert np.array_equal(got[4], ref[3]) and np.array_equal(got[4], ends)
    assert np.array_equal(got[5], ref[4]) and np.array_equal(got[5], digests)
    assert got[3] == csum == csum_of(ends, digests)
    r = pbschunk.DynamicIndexReader(image)
    assert (r.index_count(), r.index_bytes(), r.uuid, r.ctime, r.index_csum) == (n, int(ends[-1]) if n else 0, uuid, -1234567890123, csum)
    assert r.compute_csum() == (csum, int(ends[-1]) if n else 0) and r.size == len(image)
    for pos in range(min(n, 20)):
        assert r.chunk_info(pos) == (int(ends[pos - 1]) if pos else 0, int(ends[pos]), digests[pos].tobytes())
        assert r.chunk_end(pos) == int(ends[pos]) and r.index_digest(pos) == digests[pos].tobytes()
    assert r.chunk_info(n) is None and r.index_digest(n) is None
    with pytest.raises(IndexError):
        r.chunk_end(n)


def test_reader_from_path(pbschunk, tmp_path):
    ends, digests = make_index(5)
    w = pbschunk.DynamicIndexWriter(str(tmp_path / "a.didx"), uuid=bytes(16), ctime=77)
    for e, d in zip(ends, digests):
        w.add_chunk(int(e), d.tobytes())
    csum = w.close()
    r = pbschunk.DynamicIndexReader(tmp_path / "a.didx")
    assert r.index_csum == csum == r.compute_csum()[0] and r.ctime == 77 and np.array_equal(r.ends, ends)


def test_flipped_entry_byte_changes_the_computed_checksum_only(pbschunk):
    ends, digests = make_index(50)
    image, csum = pbschunk.didx_build(ends, digests)
    for at in (4096 + 40 * 7 + 9, 4096 + 40 * 49 + 39, 4096 + 40 * 49 + 7):  # digest bytes; the last end's top byte
        bad = bytearray(image)
        bad[at] ^= 0x40
        got = pbschunk.didx_parse(bytes(bad))
        assert got[2] == csum and got[3] != csum
        assert got[3] == csum_of(got[4], got[5])


def test_parse_errors(pbschunk):
    ends, digests = make_index(10)
    image, _ = pbschunk.didx_build(ends, digests)

    def code(img, cap=None):
        with pytest.raises(pbschunk.ChunkerError) as e:
            pbschunk.didx_parse(img, cap)
        return e.value.code

    assert pbschunk.didx_count(4095) is None and code(image[:4095], 0) == INVALID
    assert code(bytes([image[0] ^ 1]) + image[1:]) == INVALID
    assert code(image[:7] + bytes([image[7] ^ 0x80]) + image[8:]) == INVALID
    assert pbschunk.didx_count(len(image) + 1) is None and code(image + b"\0", 11) == INVALID
    dec = bytearray(image)
    dec[4096 + 40 * 6:4096 + 40 * 6 + 8] = struct.pack("<Q", int(ends[5]) - 1)
    assert code(bytes(dec)) == INVALID
    eq = bytearray(image)  # equal neighbours: a legal zero-length chunk
    eq[4096 + 40 * 6:4096 + 40 * 6 + 8] = struct.pack("<Q", int(ends[5]))
    assert int(pbschunk.didx_parse(bytes(eq))[4][6]) == int(ends[5])
    assert code(image, 9) == CAPACITY
    assert pbschunk.didx_parse(image, 10)[4].size == 10 and pbschunk.didx_parse(image, 11)[4].size == 10
    for bad in (image[:4095], image + b"\0", bytes(dec)):
        with pytest.raises(pbschunk.ChunkerError):
            pbschunk.DynamicIndexReader(bad)


# ---- pbs_didx_chunk_from_offset ---------------------------------------------------------------

@pytest.mark.parametrize("n,zero_runs", [(1, False), (2, False), (3, False), (1000, False), (3, True), (41, True),
                                         (1000, True)])
def test_chunk_from_offset_follows_the_reference(pbschunk, n, zero_runs):
    ends, _ = make_index(n, seed=3, zero_runs=zero_runs)
    py = [int(e) for e in ends]
    offsets = sorted({0} | {o for e in py for o in (e - 1, e, e + 1) if o >= 0})
    for off in offsets:
        got = pbschunk.didx_chunk_from_offset(ends, off)
        assert got == ref_chunk_from_offset(py, off), (n, off)
        if got is not None:  # the entry holds the byte
            i, within = got
            assert (py[i - 1] if i else 0) + within == off < py[i]
    total = py[-1]
    assert pbschunk.didx_chunk_from_offset(ends, total) is None
    assert pbschunk.didx_chunk_from_offset(ends, total - 1)[0] == max(i for i in range(n) if py[i] > (py[i - 1] if i else 0))
    assert pbschunk.lib().pbs_didx_chunk_from_offset(ends.ctypes.data, n, total, None, None) == INVALID
    assert pbschunk.DynamicIndexReader(pbschunk.didx_build(ends, np.zeros((n, 32), np.uint8))[0]).chunk_from_offset(0) == \
        ref_chunk_from_offset(py, 0)


def test_chunk_from_offset_of_an_empty_index(pbschunk):
    assert pbschunk.didx_chunk_from_offset(np.zeros(0, np.uint64), 0) is None
    assert pbschunk.didx_chunk_from_offset(np.zeros(3, np.uint64), 0) is None  # three empty chunks: no byte


# ---- pbs_digest_lookup_host -------------------------------------------------------------------

def test_lookup_host_against_a_dict(pbschunk):
    index, store = planted_lookup_sets()
    pos, first, nm, nu = pbschunk.digest_lookup_host(index, store)
    mp, mf, mm, mu = model_lookup(index, store)
    assert np.array_equal(pos, mp) and np.array_equal(first, mf) and (nm, nu) == (mm, mu)
    # what the planted sets are for
    assert nm > 0 and (first != np.arange(first.size)).any()
    assert len({d.tobytes() for d in store}) < store.shape[0] and not (np.diff(store[:, 0].astype(int)) >= 0).all()
    found = {index[i].tobytes() for i in range(index.shape[0]) if pos[i] != MISSING}
    assert any(index[i, 8] in (1, 2, 3, 4) and index[i].tobytes() in found for i in range(12, 16))
    assert any(pos[i] == MISSING for i in range(12, 16)) and any(pos[i] == MISSING for i in range(28, 32))
    # an empty store, an empty index, random sets
    pos, first, nm, nu = pbschunk.digest_lookup_host(index, np.zeros((0, 32), np.uint8))
    assert (pos == MISSING).all() and nm == index.shape[0] and np.array_equal(first, mf)
    assert pbschunk.digest_lookup_host(np.zeros((0, 32), np.uint8), store)[2:] == (0, 0)
    rng = np.random.default_rng(5)
    pool = rng.integers(0, 256, (300, 32), dtype=np.uint8)
    index, store = pool[rng.integers(0, 300, 2000)], pool[rng.integers(0, 200, 500)]
    got, want = pbschunk.digest_lookup_host(index, store), model_lookup(index, store)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2:] == want[2:]


# ---- the host code under sanitizers: a stand-alone program ------------------------------------

@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_restore_host_code_under_sanitizers():
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "proxmox-backup_amd", "csrc"), "sanitize-restore"],
                       capture_output=True, text=True, timeout=900)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert "restore_sanitize ok" in out, out[-4000:]
    assert "ERROR: AddressSanitizer" not in out and "runtime error" not in out, out[-4000:]
