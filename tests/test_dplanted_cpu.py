"""The inputs of the read side's tests (tests/dplanted.py) proved on the CPU, and the host
mirror of the read side (pbs_blob_decode_host, pbs_aes256gcm_decrypt_host) against them.

Expected values come from tests/aesgcm_ref.py, the oracle, zlib, hashlib and
tests/golden/aesgcm_vectors.json -- never from the library under test.
"""
import hashlib
import json
import os
import struct
import zlib

import numpy as np
import pytest

import aesgcm_ref
import dplanted as d
import gplanted as g

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "aesgcm_vectors.json")


@pytest.fixture(scope="module")
def cfg(pbschunk):
    with pbschunk.CryptConfig(g.KEY1) as c:
        yield c


def test_constants_match_the_library(pbschunk):
    p = pbschunk
    assert (p.BLOB_ST_OK, p.BLOB_ST_TOO_SMALL, p.BLOB_ST_BAD_MAGIC, p.BLOB_ST_BAD_CRC, p.BLOB_ST_NO_CONFIG,
            p.BLOB_ST_BAD_TAG, p.BLOB_ST_BAD_DIGEST, p.BLOB_ST_BAD_SIZE) == (
        d.OK, d.TOO_SMALL, d.BAD_MAGIC, d.BAD_CRC, d.NO_CONFIG, d.BAD_TAG, d.BAD_DIGEST, d.BAD_SIZE)
    assert (p.BLOB_KIND_UNCOMPRESSED, p.BLOB_KIND_COMPRESSED, p.BLOB_KIND_ENCRYPTED, p.BLOB_KIND_ENCR_COMPR,
            p.BLOB_KIND_NONE) == (0, 1, 2, 3, d.KIND_NONE)
    assert p.BLOB_HEADER_SIZE == d.HDR and p.BLOB_ENC_HEADER_SIZE == d.EHDR


def test_family_a_reaches_every_residue_triple():
    """Over the 16 residues of the blob stream's start and the 16 of the packed output's, family
    a shows every (length mod 16, source residue, destination residue): 16^3 triples.  One output
    residue shows an eighth of them (a length class meets two destinations, 8 apart), so the
    output residues 0..7 (OUT_PADS, what the GPU test runs) are enough."""
    assert len(d.tail_triples()) == 16 ** 3
    assert len(d.tail_triples(out_pads=(0,))) == 16 ** 3 // 8
    assert len(d.tail_triples(out_pads=d.OUT_PADS)) == 16 ** 3 and len(d.OUT_PADS) == 8
    assert g.tail_pairs() == {(r, s) for r in range(16) for s in range(16)}


def test_flip_positions_are_where_they_are_named():
    assert d.flips_hold()
    n = d.H_LEN
    for name, at in d.H_FLIPS:
        w = g.where(n, at + d.EHDR)
        if name.startswith("seg"):
            assert ("segment 0 of 2" in w) == name.endswith("lo") and ("segment 1 of 2" in w) == name.endswith("hi"), w
        if name.startswith("row"):
            assert ("lane 255" in w) == name.endswith("lo") and ("lane 0 " in w) == name.endswith("hi"), w
        if name == "last":
            assert "the partial last block" in w, w


def test_reference_outcomes_of_the_corruptions(oracle):
    """The reference functions alone give every item of families g, h and h-nocfg its wanted
    status (and payload, where the blob passes): this proves the inputs, not the library."""
    wrong = []
    for fam, key in (("g", g.KEY1), ("h", g.KEY1), ("h-nocfg", None)):
        items = d.stream(fam, oracle)
        for it in items:
            st, pay = d.reference_outcome(oracle, it, key)
            if st != it.status or (pay is not None and st == d.OK and pay != it.payload):
                wrong.append(f"{it.label}: the reference says {d.STATUS_NAMES[st]}, planted {d.STATUS_NAMES[it.status]}")
    assert not wrong, "\n".join(wrong[:20])
    h = d.corrupt_items(oracle)
    assert {it.status for it in h} == set(range(8)) - {d.NO_CONFIG}
    assert {it.kind for it in h} == {0, 1, 2, 3, d.KIND_NONE}
    hs = d.stream("h", oracle)  # every corrupted blob between two intact neighbours
    assert all(hs[i].status == d.OK and hs[i].label.startswith("h/neighbour") for i in range(0, len(hs), 2))
    assert len(hs) == 2 * len(h) + 1
    assert {it.status for it in d.stream("h-nocfg", oracle)} == {d.OK, d.NO_CONFIG, d.BAD_CRC, d.TOO_SMALL}


def test_mixed_stream_switches_header_length(oracle):
    items = d.stream("g", oracle)
    assert {it.kind for it in items} == {0, 1, 2, 3}
    hdrs = [d.EHDR if it.kind >= 2 else d.HDR for it in items]
    assert sum(a != b for a, b in zip(hdrs, hdrs[1:])) >= len(items) // 3
    assert all(len(items[i].payload) == 0 for i in range(1, len(items), 2))
    assert any(len(it.payload) > g.SEG for it in items if it.kind == 2)
    assert any(len(it.payload) > g.SEG for it in items if it.kind == 0)
    assert any(len(it.payload) > 4096 for it in items if it.kind == 3)
    assert any(len(it.payload) > 4096 for it in items if it.kind == 1)


def _host(pbschunk, cfg, it):
    return pbschunk.blob_decode_host(it.blob, cfg, it.digest, it.size)


def _assert_host(pbschunk, cfg, items):
    wrong = []
    for it in items:
        pay, kind, st = _host(pbschunk, cfg, it)
        if (kind, st) != (it.kind, it.status) or pay != it.payload:
            wrong.append(f"{it.label}: kind {kind} status {st} ({len(pay)} bytes), wanted kind {it.kind} status "
                         f"{it.status} ({len(it.payload)} bytes, equal: {pay == it.payload})")
    assert not wrong, f"{len(wrong)} of {len(items)}:\n" + "\n".join(wrong[:20])


def test_host_mirror_family_a(pbschunk, cfg):
    _assert_host(pbschunk, cfg, d.stream("a"))


def test_host_mirror_family_b_small_members(pbschunk, cfg):
    items = [it for it in d.stream("b") if len(it.payload) <= 5 * g.SEG // 4]
    assert len(items) >= 30
    _assert_host(pbschunk, cfg, items)


def test_host_mirror_mixed_and_corrupted(pbschunk, oracle, cfg):
    _assert_host(pbschunk, cfg, d.stream("g", oracle))
    _assert_host(pbschunk, cfg, d.stream("h", oracle))
    _assert_host(pbschunk, None, d.stream("h-nocfg", oracle))


def test_host_capacity_and_arguments(pbschunk, cfg):
    import ctypes

    it = d.stream("a")[100]
    L = pbschunk.lib()
    out = np.zeros(200, np.uint8)
    olen, kind, st = ctypes.c_size_t(7), ctypes.c_uint8(9), ctypes.c_uint8(9)
    blob = np.frombuffer(it.blob, np.uint8)
    rc = L.pbs_blob_decode_host(blob.ctypes.data, blob.size, cfg.handle, None, None, out.ctypes.data, 99,
                                ctypes.byref(olen), ctypes.byref(kind), ctypes.byref(st))
    assert rc == pbschunk.PBS_ERR_CAPACITY and not out.any()
    rc = L.pbs_blob_decode_host(blob.ctypes.data, blob.size, cfg.handle, None, None, out.ctypes.data, 100,
                                ctypes.byref(olen), ctypes.byref(kind), ctypes.byref(st))
    assert (rc, olen.value, kind.value, st.value) == (0, 100, 2, 0) and out[:100].tobytes() == it.payload
    assert pbschunk.blob_decode_bound([0, 5, 100, 112, 112]) == 83
    assert pbschunk.blob_decode_bound([3, 103, 203]) == 200 - 24


def test_golden_vectors_open_and_every_tag_bit_counts(pbschunk):
    with open(GOLDEN) as f:
        vectors = json.load(f)
    vs = vectors["cases"]
    assert len(vs) >= 4
    cfgs = {}
    try:
        for v in vs:
            key = bytes.fromhex(v["key"])
            c = cfgs.setdefault(key, pbschunk.CryptConfig(key))
            iv, tag = bytes.fromhex(v["iv"]), bytes.fromhex(v["tag"])
            plain = aesgcm_ref.golden_plaintext(v["len"], v["seed"])
            # (the file holds the ciphertext's SHA-256: the reference's ciphertext is the golden one)
            ct, ref_tag = aesgcm_ref.cipher(key).encrypt(iv, plain)
            assert hashlib.sha256(ct).hexdigest() == v["ct_sha256"] and ref_tag == tag
            assert c.decrypt_host(iv, ct, tag) == plain
            for bit in range(128):
                t = bytearray(tag)
                t[bit // 8] ^= 1 << (bit % 8)
                with pytest.raises(pbschunk.ChunkerError) as e:
                    c.decrypt_host(iv, ct, bytes(t))
                assert e.value.code == pbschunk.PBS_ERR_TAG
    finally:
        for c in cfgs.values():
            c.close()


def test_seal_then_open_is_the_identity(pbschunk, cfg):
    for n in range(601):
        data = g._bytes(5000 + n, n).tobytes()
        iv = g._iv(5000 + n)
        ct, tag = cfg.encrypt_host(iv, data)
        assert cfg.decrypt_host(iv, ct, tag) == data, n
        if n:
            with pytest.raises(pbschunk.ChunkerError):
                cfg.decrypt_host(iv, ct[:-1] + bytes([ct[-1] ^ 0x80]), tag)


def test_failed_open_leaves_zeros(pbschunk, cfg):
    import ctypes

    data = g._bytes(1, 100).tobytes()
    iv = g._iv(1)
    ct, tag = cfg.encrypt_host(iv, data)
    out = np.full(100, 0xEE, np.uint8)
    a = np.frombuffer(ct, np.uint8)
    rc = pbschunk.lib().pbs_aes256gcm_decrypt_host(cfg.handle, ctypes.create_string_buffer(iv, 16), a.ctypes.data, 100,
                                                   ctypes.create_string_buffer(bytes(16), 16), out.ctypes.data)
    assert rc == pbschunk.PBS_ERR_TAG and not out.any()
    assert "tag" in pbschunk.strerror(pbschunk.PBS_ERR_TAG).lower()


def test_cpu_encoded_blobs_open(pbschunk):
    for n in (0, 1, 4095, 70000):
        data = g._bytes(6000 + n, n).tobytes()
        blob = pbschunk.blob_encode_uncompressed(data, zlib.crc32(data))
        assert struct.unpack("<I", blob[8:12])[0] == zlib.crc32(data)
        assert pbschunk.blob_decode_host(blob, None, d.plain_digest(data), n) == (data, 0, d.OK)
        assert pbschunk.blob_decode_host(blob, None, d.plain_digest(data), n + 1)[2] == d.BAD_SIZE
