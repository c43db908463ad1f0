"""GPU tests of the encrypted blob path (AES-256-GCM on the device, include/pbs_blob.h):
the reference's two encrypted blob tests (tests/blob_writer.rs:89-105) on the GPU encoder,
byte equality with the independent reference (tests/aesgcm_ref.py) over the lengths around
the GCM block, the workgroup row and the GHASH segment, the 32-bit counter wrap, library
IVs, the encrypted upload path and the argument errors.

Run on an MI355X:  python -m pytest tests -m gpu -x -q
"""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest

import aesgcm_ref
import gen_np

pytestmark = pytest.mark.gpu
KiB, MiB = 1024, 1024 * 1024
KEY = bytes([1]) * 32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TEST_DATA = np.array([i % 255 for i in range(100000)], dtype=np.uint8)


def _golden():
    with open(os.path.join(GOLDEN, "blob_writer_digests.json")) as f:
        return json.load(f)


def _iv(i: int) -> bytes:
    return hashlib.sha256(b"test iv %d" % i).digest()[:16]


@pytest.fixture(scope="module")
def torch_dev(gpu):
    import torch

    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def cfg(gpu):
    with gpu.CryptConfig(KEY) as c:
        yield c


def _dev(torch, host: np.ndarray, pad_front: int = 0):
    t = torch.empty(host.size + pad_front, dtype=torch.uint8, device="cuda")
    if host.size:
        t[pad_front:] = torch.from_numpy(host).to("cuda")
    return t, t.data_ptr() + pad_front


def _encode(gpu, torch, cfg, ptr, data_len, bounds=None, spans=None, base=0, compress=False, ivs=None, pad=0):
    """Encrypted blobs of the chunks, as a list of bytes; the blob buffer starts `pad` bytes
    into its allocation."""
    if spans is None:
        n = len(bounds) - 1
        cap = gpu.blob_stream_bound_encrypted(bounds)
    else:
        n = len(spans)
        cap = 44 * n + int(sum(int(e) - int(s) for s, e in spans))
    out = torch.zeros(cap + pad + 64, dtype=torch.uint8, device="cuda")
    if spans is None:
        offs, crcs, comp, t = gpu.blob_encode_chunks_device(ptr, data_len, bounds, out.data_ptr() + pad, cap, base=base,
                                                            compress=compress, crypt=cfg, ivs=ivs)
    else:
        offs, crcs, comp, t = gpu.blob_encode_spans_device(ptr, data_len, spans, out.data_ptr() + pad, cap, base=base,
                                                           compress=compress, crypt=cfg, ivs=ivs)
    img = out.cpu().numpy()
    assert not img[:pad].any() and not img[pad + int(offs[-1]):].any(), "wrote outside the blob stream"
    assert int(offs[0]) == 0 and int(offs[-1]) <= cap
    blobs = [img[pad + int(offs[i]):pad + int(offs[i + 1])].tobytes() for i in range(n)]
    for b, crc in zip(blobs, crcs):
        assert int.from_bytes(b[8:12], "little") == int(crc)
    return blobs, comp, t


@pytest.mark.parametrize("compress", [False, True])
@pytest.mark.parametrize("align", [0, 1, 3, 8, 15, 4093])
def test_reference_fixture(gpu, oracle, torch_dev, cfg, align, compress):
    """test_encrypted_blob_writer / test_encrypted_compressed_blob_writer: TEST_DATA as one
    chunk under the key [1; 32] verifies with TEST_DIGEST_ENC."""
    g = _golden()
    digest = bytes.fromhex(g["digest_enc"])
    assert cfg.id_key.hex() == g["id_key"]
    t, ptr = _dev(torch_dev, TEST_DATA, align)
    bounds = np.array([0, TEST_DATA.size], dtype=np.uint64)
    assert bytes(gpu.digest_chunks_device(ptr, TEST_DATA.size, bounds, key=cfg.id_key)[0]) == digest
    iv = _iv(align)
    blobs, comp, _ = _encode(gpu, torch_dev, cfg, ptr, TEST_DATA.size, bounds=bounds, compress=compress, ivs=[iv],
                             pad=align)
    blob = blobs[0]
    assert blob[12:28] == iv
    assert aesgcm_ref.blob_load_decode_encrypted(blob, KEY, digest) == TEST_DATA.tobytes()
    if not compress:
        assert comp[0] == 0
        assert blob == aesgcm_ref.blob_encode_encrypted(TEST_DATA.tobytes(), KEY, iv)
    else:
        assert comp[0] == 1 and blob[:8] == aesgcm_ref.ENCR_COMPR_BLOB_MAGIC
        cap = gpu.blob_stream_bound(bounds)
        out = torch_dev.empty(cap, dtype=torch_dev.uint8, device="cuda")
        offs, _, c2, _ = gpu.blob_encode_chunks_device(ptr, TEST_DATA.size, bounds, out.data_ptr(), cap)
        plain_blob = out.cpu().numpy()[:int(offs[1])].tobytes()
        assert c2[0] == 1 and plain_blob[:8] == oracle.COMPRESSED_BLOB_MAGIC
        assert aesgcm_ref.blob_decrypt_payload(blob, KEY) == plain_blob[12:]


@pytest.fixture(scope="module")
def shapes(gpu):
    """Chunks around the GCM block (16), the workgroup row (4096) and the GHASH segment S,
    with their IVs and reference blobs (compress off), computed once."""
    import corpus_gen

    S = gpu.GCM_SEGMENT_BYTES
    assert S == 65536
    lens = [0, 1, 15, 16, 17, 777, 4105, 65536, 100000, S - 16, S, S + 1, 2 * S + 15, 3 * S + 5]
    rng = np.random.default_rng(0xC0DE)
    chunks = []
    for i, n in enumerate(lens):
        if i == 7:
            c = np.zeros(n, dtype=np.uint8)  # 65536 zeros
        elif n == 100000:
            c = TEST_DATA.copy()
        elif n == 3 * S + 5:
            c = corpus_gen.text(n + 8192, 5)[:n]
        else:
            c = rng.integers(0, 256, n, dtype=np.uint8)
        assert c.size == n
        chunks.append(np.ascontiguousarray(c, dtype=np.uint8))
    ivs = [_iv(100 + i) for i in range(len(lens))]
    assert len(set(ivs)) == len(ivs)
    ref = [aesgcm_ref.blob_encode_encrypted(c.tobytes(), KEY, iv) for c, iv in zip(chunks, ivs)]
    return chunks, ivs, ref


def _verify_all(blobs, chunks):
    idk = aesgcm_ref.id_key(KEY)
    for b, c in zip(blobs, chunks):
        want = hashlib.sha256(c.tobytes() + idk).digest()
        assert aesgcm_ref.blob_load_decode_encrypted(b, KEY, want) == c.tobytes()


def test_shapes_bounds(gpu, torch_dev, cfg, shapes):
    chunks, ivs, ref = shapes
    base = (1 << 33) + 12345
    data = np.concatenate(chunks)
    bounds = (base + np.concatenate([[0], np.cumsum([c.size for c in chunks])])).astype(np.uint64)
    t, ptr = _dev(torch_dev, data, 5)
    blobs, comp, tm = _encode(gpu, torch_dev, cfg, ptr, data.size, bounds=bounds, base=base, ivs=ivs, pad=3)
    for i, (b, r) in enumerate(zip(blobs, ref)):
        assert b == r, f"chunk {i} ({chunks[i].size} bytes)"
    assert not comp.any() and tm["gcm_segments"] == sum((c.size + 65535) // 65536 for c in chunks)
    blobs, comp, _ = _encode(gpu, torch_dev, cfg, ptr, data.size, bounds=bounds, base=base, compress=True, ivs=ivs,
                             pad=1)
    assert comp[7] == 1 and comp[8] == 1 and comp[-1] == 1  # zeros, TEST_DATA, text
    for b, c in zip(blobs, comp):
        assert b[:8] == (aesgcm_ref.ENCR_COMPR_BLOB_MAGIC if c else aesgcm_ref.ENCRYPTED_BLOB_MAGIC)
    _verify_all(blobs, chunks)


def test_shapes_spans_reversed_with_gaps(gpu, torch_dev, cfg, shapes):
    chunks, ivs, ref = shapes
    base = (1 << 33) + 977
    parts, spans, pos = [], [], base
    rng = np.random.default_rng(9)
    for i, c in enumerate(chunks):
        gap = rng.integers(0, 256, 1 + (i * 7) % 23, dtype=np.uint8)
        parts += [gap, c]
        spans.append((pos + gap.size, pos + gap.size + c.size))
        pos += gap.size + c.size
    data = np.concatenate(parts)
    order = list(range(len(chunks)))[::-1]
    sp = np.array([spans[i] for i in order], dtype=np.uint64)
    t, ptr = _dev(torch_dev, data, 11)
    blobs, comp, _ = _encode(gpu, torch_dev, cfg, ptr, data.size, spans=sp, base=base, ivs=[ivs[i] for i in order],
                             pad=7)
    for k, i in enumerate(order):
        assert blobs[k] == ref[i], f"chunk {i} ({chunks[i].size} bytes)"
    blobs, comp, _ = _encode(gpu, torch_dev, cfg, ptr, data.size, spans=sp, base=base, compress=True,
                             ivs=[ivs[i] for i in order], pad=2)
    _verify_all(blobs, [chunks[i] for i in order])


def test_counter_wrap(gpu, torch_dev, cfg):
    """IVs whose J0 ends in 0xFFFFFFF0 / 0xFFFFFFFF (golden, from libcrypto): the counter
    wraps in its low 32 bits only, inside the first blocks of the chunk."""
    with open(os.path.join(GOLDEN, "aesgcm_vectors.json")) as f:
        cases = [c for c in json.load(f)["cases"] if "j0_low32" in c and c["key"] == KEY.hex()]
    assert {(c["j0_low32"], c["len"]) for c in cases} == {(w, n) for w in ("fffffff0", "ffffffff")
                                                          for n in (1024, 100000)}
    chunks = [np.frombuffer(aesgcm_ref.golden_plaintext(c["len"], c["seed"]), dtype=np.uint8) for c in cases]
    ivs = [bytes.fromhex(c["iv"]) for c in cases]
    data = np.concatenate(chunks)
    bounds = np.concatenate([[0], np.cumsum([c.size for c in chunks])]).astype(np.uint64)
    t, ptr = _dev(torch_dev, data, 9)
    blobs, _, _ = _encode(gpu, torch_dev, cfg, ptr, data.size, bounds=bounds, ivs=ivs, pad=5)
    for b, c, iv, chunk in zip(blobs, cases, ivs, chunks):
        assert b == aesgcm_ref.blob_encode_encrypted(chunk.tobytes(), KEY, iv), c
        assert b[28:44].hex() == c["tag"] and hashlib.sha256(b[44:]).hexdigest() == c["ct_sha256"]


def test_library_ivs(gpu, torch_dev, cfg):
    lens = [0, 5, 4096, 70000, 16, 33333]
    rng = np.random.default_rng(4)
    chunks = [rng.integers(0, 256, n, dtype=np.uint8) for n in lens]
    data = np.concatenate(chunks)
    bounds = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    t, ptr = _dev(torch_dev, data, 2)
    seen = []
    for _ in range(2):
        blobs, _, _ = _encode(gpu, torch_dev, cfg, ptr, data.size, bounds=bounds, ivs=None)
        seen += [b[12:28] for b in blobs]
        _verify_all(blobs, chunks)
    assert len(set(seen)) == 2 * len(lens)
    assert all(iv != bytes(16) for iv in seen)


@pytest.mark.parametrize("copies,spec", [(1, "1"), (2, "1"), (2, "0")])
@pytest.mark.parametrize("avg", [64 * KiB, 256 * KiB])
def test_upload_crypt(gpu, oracle, monkeypatch, cfg, avg, copies, spec):
    """pbs_upload_stream_host_crypt over a random head plus TEST_DATA x 40.  TEST_DATA has
    no cut candidates, so its chunks end at the maximum size and never line up with its
    100000-byte period: that stream alone has no repeated chunk.  `copies` 2 sends it twice;
    the chunker resyncs inside the second head and the chunks after it are known chunks.
    spec 1 encodes per piece beside the copies, 0 in the final pass after the pipeline."""
    monkeypatch.setenv("PBS_UPLOAD_SPEC", spec)
    one = np.concatenate([gen_np.gen_random(300 * KiB + 7, 77)] + [TEST_DATA] * 40)
    data = np.concatenate([one] * copies)
    ref_ends = oracle.chunk_feed(avg, data)
    if ref_ends.size == 0 or int(ref_ends[-1]) != data.size:
        ref_ends = np.append(ref_ends, np.uint64(data.size))
    bounds = np.concatenate([[0], ref_ends]).astype(np.uint64)
    idk = cfg.id_key
    chunks = [data[int(bounds[i]):int(bounds[i + 1])].tobytes() for i in range(ref_ends.size)]
    ref_dig = np.array([np.frombuffer(hashlib.sha256(c + idk).digest(), dtype=np.uint8) for c in chunks])
    out = gpu.upload_stream_host(data, avg, piece=1 * MiB + 3, crypt=cfg)
    assert np.array_equal(out["ends"], ref_ends)
    assert np.array_equal(out["digests"], ref_dig)
    ref_known = oracle.known_chunks(ref_dig, [])
    assert (int(ref_known.sum()) > 0) == (copies == 2)
    assert np.array_equal(out["known"], ref_known)
    offs = out["blob_offsets"]
    total = 0
    for i, c in enumerate(chunks):
        blob = out["blobs"][int(offs[i]):int(offs[i + 1])].tobytes()
        total += len(blob)
        if ref_known[i]:
            assert blob == b""
            continue
        assert aesgcm_ref.blob_load_decode_encrypted(blob, KEY, bytes(ref_dig[i])) == c
        assert (blob[:8] == aesgcm_ref.ENCR_COMPR_BLOB_MAGIC) == bool(out["compressed"][i])
    assert out["stats"]["size_compressed"] == total == int(offs[-1])
    assert out["stats"]["chunk_reused"] == int(ref_known.sum())
    ivs = [out["blobs"][int(offs[i]) + 12:int(offs[i]) + 28].tobytes() for i in range(len(chunks)) if not ref_known[i]]
    assert len(set(ivs)) == len(ivs)


def test_errors(gpu, torch_dev, cfg):
    data = gen_np.gen_random(50000, 3)
    bounds = np.array([0, 20000, 20000, 50000], dtype=np.uint64)
    t, ptr = _dev(torch_dev, data, 0)
    bound = gpu.blob_stream_bound_encrypted(bounds)
    assert bound == 3 * 44 + 50000
    out = torch_dev.full((bound + 4096,), 0xA5, dtype=torch_dev.uint8, device="cuda")
    offs = np.zeros(4, dtype=np.uint64)
    lib = gpu.lib()
    for f in (lib.pbs_blob_encode_chunks_encrypted_device, lib.pbs_blob_encode_spans_encrypted_device):
        rc = f(ctypes.c_void_p(ptr), data.size, 0, bounds.ctypes.data, 1, 0, None, None,
               ctypes.c_void_p(out.data_ptr()), bound, offs.ctypes.data, None, None, None, None)
        assert rc == gpu.PBS_ERR_INVALID  # PBS_ERR_ARG
    for compress in (False, True):
        with pytest.raises(gpu.ChunkerError) as e:
            gpu.blob_encode_chunks_device(ptr, data.size, bounds, out.data_ptr(), bound - 1, compress=compress,
                                          crypt=cfg, ivs=[_iv(i) for i in range(3)])
        assert e.value.code == gpu.PBS_ERR_CAPACITY
        torch_dev.cuda.synchronize()
        assert bool((out == 0xA5).all()), "a refused call wrote into the blob buffer"
    # and with the exact bound it fits, the guard behind it untouched
    gpu.blob_encode_chunks_device(ptr, data.size, bounds, out.data_ptr(), bound, compress=False, crypt=cfg,
                                  ivs=[_iv(i) for i in range(3)])
    img = out.cpu().numpy()
    assert (img[bound:] == 0xA5).all() and img[:8].tobytes() == aesgcm_ref.ENCRYPTED_BLOB_MAGIC
