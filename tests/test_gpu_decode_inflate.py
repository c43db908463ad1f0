"""GPU: the finished read path, pbs_blob_decode_inflate_device (csrc/pbs_inflate.hip), on the
compressed and mixed blobs of tests/dplanted.py (families f and g) and on the device encoder's
own output in all four modes.

The wanted chunk of a compressed blob is what libzstd inflates its frame to (the frame of an
encrypted one decrypted by tests/aesgcm_ref.py); the digests -- SHA-256(chunk), with id_key
appended for the encrypted kinds -- are hashlib's.  pbs_blob_decode_device must still hand the
frames back as before.

Run on an MI355X:  python -m pytest tests/test_gpu_decode_inflate.py -m gpu -x -q
"""
import hashlib
import struct
import zlib

import numpy as np
import pytest

import aesgcm_ref
import dplanted as d
import gplanted as g

pytestmark = pytest.mark.gpu

FILL = 0xA5
OK, NO_CONFIG, BAD_DIGEST, BAD_SIZE, BAD_FRAME = 0, 4, 6, 7, 8


@pytest.fixture(scope="module")
def torch_dev(gpu):
    import torch

    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def cfg(gpu):
    with gpu.CryptConfig(g.KEY1) as c:
        yield c


def chunk_of(oracle, it):
    return it.payload if it.kind in (0, 2) else oracle.zstd_decode_stream(it.payload, 1 << 17)


def digest_of(kind, chunk):
    return d.keyed_digest(chunk, g.KEY1) if kind >= 2 else d.plain_digest(chunk)


def run(gpu, torch, cfg, blobs, sizes, digests=None, sizes_exact=False, pad=5, out_pad=3):
    offs = np.concatenate([[0], np.cumsum([len(b) for b in blobs])]).astype(np.uint64)
    data = np.frombuffer(bytes(pad) + b"".join(blobs), np.uint8)
    src = torch.from_numpy(data.copy()).cuda()
    cap = int(sum(sizes))
    out = torch.full((out_pad + cap + 256,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    dg = None if digests is None else np.frombuffer(b"".join(digests), np.uint8)
    oo, lens, kinds, status, timing = gpu.blob_decode_inflate_device(
        src.data_ptr() + pad, offs, out.data_ptr() + out_pad, cap, np.array(sizes, np.uint64), crypt=cfg,
        expect_digests=dg, sizes_exact=sizes_exact)
    torch.cuda.synchronize()
    assert np.array_equal(src.cpu().numpy(), data), "the input was written"
    img = out.cpu().numpy()
    assert [int(x) for x in oo] == [int(x) for x in np.concatenate([[0], np.cumsum(sizes)])]
    assert (img[:out_pad] == FILL).all() and (img[out_pad + cap:] == FILL).all(), "bytes outside the slots were written"
    slots = [img[out_pad + int(oo[i]):out_pad + int(oo[i + 1])] for i in range(len(blobs))]
    return slots, lens, kinds, status, timing


def expect_all_good(items, chunks, slots, lens, kinds, status):
    for it, c, s, n, k, st in zip(items, chunks, slots, lens, kinds, status):
        assert (int(k), int(st)) == (it.kind, OK), (it.label, int(k), int(st))
        assert int(n) == len(c) and s[:len(c)].tobytes() == c, it.label
        assert (s[len(c):] == FILL).all(), it.label


@pytest.mark.parametrize("family", ["f", "g"])
def test_planted_blobs_inflate_to_their_chunks(gpu, torch_dev, cfg, oracle, family):
    items = d.stream(family, oracle)
    chunks = [chunk_of(oracle, it) for it in items]
    assert {it.kind for it in items} >= {1, 3}
    digests = [digest_of(it.kind, c) for it, c in zip(items, chunks)]
    # exact slots, digests of all kinds, sizes_exact
    slots, lens, kinds, status, timing = run(gpu, torch_dev, cfg, [it.blob for it in items], [len(c) for c in chunks],
                                             digests, sizes_exact=True)
    expect_all_good(items, chunks, slots, lens, kinds, status)
    assert timing["frames"] == sum(it.kind in (1, 3) for it in items) and timing["failed"] == 0
    # roomier slots, no digests: the bytes past out_lens keep their fill
    slots, lens, kinds, status, _ = run(gpu, torch_dev, cfg, [it.blob for it in items], [len(c) + 9 for c in chunks])
    expect_all_good(items, chunks, slots, lens, kinds, status)
    # the existing call still hands the frames back
    dec = d.gpu_decode(gpu, torch_dev, cfg, items)
    assert not d.mismatches(items, dec) and dec.input_unchanged and dec.outside_clean


@pytest.mark.parametrize("compress,encrypt", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_device_encoder_output_round_trips(gpu, torch_dev, cfg, oracle, compress, encrypt):
    import corpus_gen

    host = np.concatenate([corpus_gen.text(400_000, 3)[:390_000], np.zeros(100_000, np.uint8), oracle.gen_random(200_000, 9)])
    n = host.size
    bounds = np.array([0, 1, 70_000, 200_001, 390_000, 490_000, 490_016, 640_000, n], np.uint64)
    dev = torch_dev.from_numpy(host.copy()).cuda()
    cap = gpu.blob_stream_bound_encrypted(bounds) if encrypt else gpu.blob_stream_bound(bounds)
    blobs = torch_dev.empty(cap, dtype=torch_dev.uint8, device="cuda")
    offs, _, comp, _ = gpu.blob_encode_chunks_device(dev.data_ptr(), n, bounds, blobs.data_ptr(), cap, compress=bool(compress),
                                                     crypt=cfg if encrypt else None)
    assert bool(comp.any()) == bool(compress)
    chunks = [host[int(bounds[i]):int(bounds[i + 1])].tobytes() for i in range(bounds.size - 1)]
    digests = [digest_of(2 if encrypt else 0, c) for c in chunks]
    sizes = np.array([len(c) for c in chunks], np.uint64)
    out = torch_dev.full((n + 64,), FILL, dtype=torch_dev.uint8, device="cuda")
    oo, lens, kinds, status, timing = gpu.blob_decode_inflate_device(
        blobs.data_ptr(), offs, out.data_ptr(), n, sizes, crypt=cfg, expect_digests=np.frombuffer(b"".join(digests), np.uint8),
        sizes_exact=True)
    torch_dev.cuda.synchronize()
    img = out.cpu().numpy()
    where = [(i, int(lens[i]), int(status[i]), img[int(oo[i]):int(oo[i + 1])].tobytes() == chunks[i])
             for i in range(len(chunks))]
    assert not status.any(), where
    assert [int(k) for k in kinds] == [2 * encrypt + int(c) for c in comp]
    assert img[:n].tobytes() == host.tobytes() and (img[n:] == FILL).all()
    assert [int(x) for x in lens] == [len(c) for c in chunks]
    assert timing["frames"] == int(comp.sum())


def _four_kinds(oracle):
    import corpus_gen

    chunk = corpus_gen.text(150_000, 5).tobytes()
    blobs = [d.make_blob(oracle, k, chunk, g.KEY1, g._iv(9100 + k)) for k in range(4)]
    assert [d.kind_of(b) for b in blobs] == [0, 1, 2, 3]
    return chunk, blobs


def test_wrong_digest_on_each_kind(gpu, torch_dev, cfg, oracle):
    chunk, blobs = _four_kinds(oracle)
    good = [digest_of(k, chunk) for k in range(4)]
    for victim in range(4):
        digests = [d._flip(x, 17, 3) if k == victim else x for k, x in enumerate(good)]
        slots, lens, kinds, status, _ = run(gpu, torch_dev, cfg, blobs, [len(chunk)] * 4, digests, sizes_exact=True)
        assert [int(s) for s in status] == [BAD_DIGEST if k == victim else OK for k in range(4)]
        for k in range(4):
            if k == victim and k >= 2:
                assert not slots[k].any() and int(lens[k]) == 0, "an encrypted blob that failed left bytes in its slot"
            else:
                assert slots[k].tobytes() == chunk


def test_valid_tag_over_a_damaged_frame(gpu, torch_dev, cfg, oracle):
    chunk, blobs = _four_kinds(oracle)
    # the first flip from the middle of the frame on that libzstd refuses
    intact = blobs[1][12:]
    frame = next(f for f in (d._flip(intact, at, 4) for at in range(len(intact) // 2, len(intact)))
                 if judge_fails(oracle, f, len(chunk)))
    enc = aesgcm_ref.blob_encode_encrypted(bytes(frame), g.KEY1, g._iv(9200), True)
    plain = d.COMPRESSED_MAGIC + struct.pack("<I", zlib.crc32(bytes(frame))) + bytes(frame)
    both = [blobs[0], enc, blobs[2], plain, blobs[3]]
    kinds_w = [0, 3, 2, 1, 3]
    digests = [digest_of(k, chunk) for k in kinds_w]
    slots, lens, kinds, status, _ = run(gpu, torch_dev, cfg, both, [len(chunk)] * 5, digests)
    assert [int(k) for k in kinds] == kinds_w
    assert [int(s) for s in status] == [OK, BAD_FRAME, OK, BAD_FRAME, OK]
    assert not slots[1].any() and int(lens[1]) == 0, "kind 3 with a bad frame: the slot must be zero"
    for i in (0, 2, 4):
        assert slots[i].tobytes() == chunk


def judge_fails(oracle, frame, cap):
    try:
        oracle.zstd_decompress(frame, cap)
    except ValueError:
        return True
    return False


def test_overflow_rule_with_and_without_digests(gpu, torch_dev, cfg, oracle):
    chunk, blobs = _four_kinds(oracle)
    short = len(chunk) - 1
    for with_digests, want in ((True, BAD_DIGEST), (False, BAD_SIZE)):
        digests = [digest_of(k, chunk) for k in range(4)] * 2 if with_digests else None
        slots, lens, kinds, status, _ = run(gpu, torch_dev, cfg, blobs + blobs, [short] * 4 + [len(chunk)] * 4, digests)
        assert [int(s) for s in status] == [want] * 4 + [OK] * 4
        assert not slots[2].any() and not slots[3].any(), "encrypted blobs that failed: zero slots"
        assert slots[0].tobytes() == chunk[:short]  # an unencrypted blob keeps what was written
        for i in range(4, 8):
            assert slots[i].tobytes() == chunk
    # sizes_exact: a roomier slot is BAD_SIZE for the unencrypted kinds only (verify_unencrypted)
    slots, lens, kinds, status, _ = run(gpu, torch_dev, cfg, blobs, [len(chunk) + 1] * 4, None, sizes_exact=True)
    assert [int(s) for s in status] == [BAD_SIZE, BAD_SIZE, OK, OK]


def test_without_a_config(gpu, torch_dev, oracle):
    chunk, blobs = _four_kinds(oracle)
    digests = [digest_of(k, chunk) for k in range(4)]
    slots, lens, kinds, status, _ = run(gpu, torch_dev, None, blobs, [len(chunk)] * 4, digests, sizes_exact=True)
    assert [int(s) for s in status] == [OK, OK, NO_CONFIG, NO_CONFIG]
    assert slots[0].tobytes() == chunk and slots[1].tobytes() == chunk
    assert not slots[2].any() and not slots[3].any()
