"""CPU tests of the encrypted blob path: the independent AES-256-GCM reference
(tests/aesgcm_ref.py) against the libcrypto golden vectors, the library's crypt config and
host AES-GCM against the reference, and the encrypted arm of the blob verifier on the
reference's fixture (tests/blob_writer.rs:11-32, :89-105).  No GPU.
"""
import ctypes
import ctypes.util
import hashlib
import json
import os
import struct
import zlib

import numpy as np
import pytest

import aesgcm_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEY = bytes([1]) * 32
IV = bytes(range(0x40, 0x50))


@pytest.fixture(scope="module")
def vectors():
    with open(os.path.join(GOLDEN, "aesgcm_vectors.json")) as f:
        return json.load(f)["cases"]


@pytest.fixture(scope="module")
def fixture():
    with open(os.path.join(GOLDEN, "blob_writer_digests.json")) as f:
        g = json.load(f)
    data = bytes(i % 255 for i in range(100000))
    assert hashlib.sha256(data).hexdigest() == g["digest_plain"]
    return data, g


def test_reference_reproduces_golden(vectors):
    assert len({c["key"] for c in vectors}) == 2
    assert {c["len"] for c in vectors} >= {0, 1, 15, 16, 17, 31, 32, 33, 255, 4105, 65536, 100000}
    wraps = set()
    for c in vectors:
        key, iv = bytes.fromhex(c["key"]), bytes.fromhex(c["iv"])
        ct, tag = aesgcm_ref.cipher(key).encrypt(iv, aesgcm_ref.golden_plaintext(c["len"], c["seed"]))
        assert len(ct) == c["len"]
        assert tag.hex() == c["tag"], c
        assert hashlib.sha256(ct).hexdigest() == c["ct_sha256"], c
        if "j0_low32" in c:
            assert "%08x" % (aesgcm_ref.cipher(key).j0(iv) & 0xFFFFFFFF) == c["j0_low32"]
            wraps.add(c["j0_low32"])
    assert wraps == {"fffffff0", "ffffffff"}


def test_reference_matches_live_libcrypto(vectors):
    import sys

    sys.path.insert(0, GOLDEN)
    try:
        import make_aesgcm_golden as gen

        L = gen.libcrypto()
        L.EVP_aes_256_gcm
    except (OSError, AttributeError, TypeError):
        pytest.skip("no loadable libcrypto")
    finally:
        sys.path.remove(GOLDEN)
    rng = np.random.default_rng(11)
    key = rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
    c = aesgcm_ref.cipher(key)
    ivs = [rng.integers(0, 256, 16, dtype=np.uint8).tobytes(), c.iv_for_j0((0x5EED << 40) | 0xFFFFFFFE)]
    for iv in ivs:
        for n in (0, 33, 77, 100, 5000):
            data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
            assert c.encrypt(iv, data) == gen.evp_encrypt(L, key, iv, data)


def test_crypt_config_id_key(pbschunk, fixture):
    _, g = fixture
    with pbschunk.CryptConfig(KEY) as cfg:
        assert cfg.id_key.hex() == g["id_key"]
        assert cfg.id_key == aesgcm_ref.id_key(KEY)
    with pytest.raises(RuntimeError):
        cfg.id_key
    with pytest.raises(ValueError):
        pbschunk.CryptConfig(bytes(31))
    out = ctypes.c_void_p()
    assert pbschunk.lib().pbs_crypt_config_new(None, ctypes.byref(out)) == pbschunk.PBS_ERR_INVALID
    assert not out.value
    pbschunk.lib().pbs_crypt_config_free(None)  # a no-op


def test_host_encrypt_equals_reference(pbschunk, vectors):
    cfgs = {}
    try:
        for c in vectors:
            key, iv = bytes.fromhex(c["key"]), bytes.fromhex(c["iv"])
            cfg = cfgs.setdefault(key, pbschunk.CryptConfig(key))
            data = aesgcm_ref.golden_plaintext(c["len"], c["seed"])
            ct, tag = cfg.encrypt_host(iv, data)
            assert (ct, tag) == aesgcm_ref.cipher(key).encrypt(iv, data), c
            assert tag.hex() == c["tag"] and hashlib.sha256(ct).hexdigest() == c["ct_sha256"]
    finally:
        for cfg in cfgs.values():
            cfg.close()


def test_segmented_tag_equals_reference(pbschunk):
    """The kernels' GHASH decomposition (segments from the end, lane-strided Horner sums
    through the per-key H^256 table, lane powers, H^segment) run on the host."""
    S = pbschunk.GCM_SEGMENT_BYTES
    rng = np.random.default_rng(5)
    key = rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
    with pbschunk.CryptConfig(key) as cfg:
        for n in (0, 1, 16, 17, 4096 + 5, S - 16, S, S + 1, 2 * S + 15, 3 * S + 5):
            iv = rng.integers(0, 256, 16, dtype=np.uint8).tobytes()
            ct = rng.integers(0, 256, n, dtype=np.uint8)
            tag = (ctypes.c_uint8 * 16)()
            rc = pbschunk.lib().pbs_test_gcm_tag_segments_host(cfg.handle, iv, ct.ctypes.data if n else None, n, tag)
            assert rc == pbschunk.PBS_OK
            c = aesgcm_ref.cipher(key)
            assert bytes(tag) == c._tag(c.j0(iv), ct.tobytes()), n


def _frame(oracle, data):
    frame = oracle.zstd_twin_frame(data)
    assert len(frame) < len(data)
    return frame


def test_verifier_accepts_reference_blobs(oracle, fixture):
    data, g = fixture
    digest = bytes.fromhex(g["digest_enc"])
    plain = aesgcm_ref.blob_encode_encrypted(data, KEY, IV)
    assert plain[:8] == aesgcm_ref.ENCRYPTED_BLOB_MAGIC and len(plain) == len(data) + 44
    assert aesgcm_ref.blob_load_decode_encrypted(plain, KEY, digest) == data
    comp = aesgcm_ref.blob_encode_encrypted(_frame(oracle, data), KEY, IV, payload_is_zstd=True)
    assert comp[:8] == aesgcm_ref.ENCR_COMPR_BLOB_MAGIC and len(comp) < len(plain)
    assert aesgcm_ref.blob_load_decode_encrypted(comp, KEY, digest) == data
    # the unencrypted verifier refuses both
    for b in (plain, comp):
        with pytest.raises(ValueError):
            oracle.blob_load_decode(b)


def _flip(blob: bytes, pos: int, fix_crc: bool) -> bytes:
    b = bytearray(blob)
    b[pos] ^= 0x10
    if fix_crc:
        b[8:12] = struct.pack("<I", zlib.crc32(bytes(b[44:])))
    return bytes(b)


def test_verifier_rejects(oracle, fixture):
    data, g = fixture
    digest = bytes.fromhex(g["digest_enc"])
    for blob in (aesgcm_ref.blob_encode_encrypted(data, KEY, IV),
                 aesgcm_ref.blob_encode_encrypted(_frame(oracle, data), KEY, IV, payload_is_zstd=True)):
        with pytest.raises(ValueError, match="tag"):
            aesgcm_ref.blob_load_decode_encrypted(_flip(blob, 28 + 5, False), KEY, digest)
        with pytest.raises(ValueError, match="CRC"):
            aesgcm_ref.blob_load_decode_encrypted(_flip(blob, 44 + 100, False), KEY, digest)
        with pytest.raises(ValueError, match="tag"):
            aesgcm_ref.blob_load_decode_encrypted(_flip(blob, 44 + 100, True), KEY, digest)
        with pytest.raises(ValueError, match="tag"):
            aesgcm_ref.blob_load_decode_encrypted(blob, bytes([2]) * 32, digest)
        with pytest.raises(ValueError, match="digest"):
            aesgcm_ref.blob_load_decode_encrypted(blob, KEY, bytes.fromhex(g["digest_plain"]))
        with pytest.raises(ValueError, match="too small"):
            aesgcm_ref.blob_load_decode_encrypted(blob[:43], KEY, digest)
        with pytest.raises(ValueError, match="magic"):
            aesgcm_ref.blob_load_decode_encrypted(b"\0" * 8 + blob[8:], KEY, digest)


def test_null_config_and_bounds_are_argument_errors(pbschunk):
    lib = pbschunk.lib()
    offs = np.zeros(2, dtype=np.uint64)
    b = np.array([0, 16], dtype=np.uint64)
    for f in (lib.pbs_blob_encode_chunks_encrypted_device, lib.pbs_blob_encode_spans_encrypted_device):
        assert f(None, 16, 0, b.ctypes.data, 1, 0, None, None, None, 1 << 20, offs.ctypes.data, None, None, None,
                 None) == pbschunk.PBS_ERR_INVALID
    assert pbschunk.blob_stream_bound_encrypted([5, 10, 30]) == 2 * 44 + 25
    assert pbschunk.blob_stream_bound_encrypted([7]) == 0
    tag = (ctypes.c_uint8 * 16)()
    assert lib.pbs_aes256gcm_encrypt_host(None, IV, None, 0, None, tag) == pbschunk.PBS_ERR_INVALID
