"""GPU parity of the AES-256-GCM blob stage (csrc/pbs_crypt.hip) on the planted cases of
tests/gplanted.py: every tail length at every payload alignment, the ragged first segment on
the wave, row and segment boundaries, the counter wrap in every row position with J0's upper
words all ones, more items than two trips of the grid, four keys alive at once, and
compressed payloads -- through the chunks entry point, the spans entry point and a side
stream.

Every blob must equal the reference's (tests/aesgcm_ref.py; for compressed payloads the
oracle's frame encrypted by the reference) byte for byte, carry zlib's CRC of the ciphertext
in its header and in the returned array and the right magic and compressed flag; every byte
outside the blob stream stays as it was filled.  One encode call per family over all its
chunks back to back above 2^33.  test_gplanted_cpu.py proves on the CPU that each case holds
the feature it is named for.

Run on an MI355X:  python -m pytest tests/test_gpu_gplanted.py -m gpu -x -q
"""
import struct
import zlib

import numpy as np
import pytest

import aesgcm_ref
import gplanted as g

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_dev(gpu):
    import torch

    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def cfg(gpu):
    with gpu.CryptConfig(g.KEY1) as c:
        yield c


def _check(cs, exp, enc, zstd=None):
    """cs: the cases in the call's order; exp: their expected blobs; zstd: per case whether
    the payload is a zstd frame (None: compress off)."""
    assert len(enc.blobs) == len(cs) == len(exp)
    bad = []
    for i, (c, want, blob, crc, comp) in enumerate(zip(cs, exp, enc.blobs, enc.crcs, enc.comp)):
        if blob != want:
            a, b = np.frombuffer(blob, np.uint8), np.frombuffer(want, np.uint8)
            n = min(a.size, b.size)
            d = np.flatnonzero(a[:n] != b[:n])
            at = int(d[0]) if d.size else n
            msg = f"{c.label}: blob differs from the reference's at byte {at} ({g.where(len(want) - g.HDR, at)})"
            pay = d[d >= g.HDR]
            if at < g.HDR:  # (CRC and tag follow from the ciphertext: say where that goes wrong first)
                msg += (f", the ciphertext first at byte {int(pay[0])} ({g.where(len(want) - g.HDR, int(pay[0]))})"
                        if pay.size else ", the ciphertext not at all")
            bad.append(msg + f"; {d.size} bytes differ; {len(blob)} bytes, the reference's {len(want)}")
            continue
        z = bool(zstd[i]) if zstd is not None else False
        if struct.unpack("<I", blob[8:12])[0] != int(crc) or int(crc) != zlib.crc32(blob[g.HDR:]):
            bad.append(f"{c.label}: CRC field {blob[8:12].hex()}, returned {int(crc):#x}, zlib {zlib.crc32(blob[g.HDR:]):#x}")
        if blob[:8] != (aesgcm_ref.ENCR_COMPR_BLOB_MAGIC if z else aesgcm_ref.ENCRYPTED_BLOB_MAGIC) or bool(comp) != z:
            bad.append(f"{c.label}: magic {blob[:8].hex()}, comp flag {int(comp)}, payload is zstd: {z}")
    assert not bad, f"{len(bad)} of {len(cs)} cases:\n" + "\n".join(bad[:20])
    assert enc.outside_clean, "bytes outside the blob stream were written"


def _encode_chunks(gpu, torch, cfg, cs, pad=g.PAD, hip_stream=0, compress=False, src=None):
    data, bounds = g.layout_chunks([c.chunk for c in cs])
    t, ptr = src or g.gpu_upload(torch, data)
    return g.gpu_encode(gpu, torch, cfg, ptr, data.size, [c.iv for c in cs], bounds=bounds, pad=pad, compress=compress,
                        hip_stream=hip_stream)


def test_family_a_every_tail_at_every_alignment(gpu, torch_dev, cfg):
    """Lengths 0..600 in one call, at each of the 16 residues of the blob buffer's start: every
    (bytes in the last block, payload start mod 16) pair."""
    cs, exp = g.cases("a"), g.expected("a")
    data, _ = g.layout_chunks([c.chunk for c in cs])
    src = g.gpu_upload(torch_dev, data)
    for pad in g.TAIL_PADS:
        enc = _encode_chunks(gpu, torch_dev, cfg, cs, pad=pad, src=src)
        _check(cs, exp, enc)
        assert enc.timing["gcm_segments"] == 600


@pytest.mark.parametrize("family", ["b", "c"])
def test_family_chunks(gpu, torch_dev, cfg, family):
    cs = g.cases(family)
    enc = _encode_chunks(gpu, torch_dev, cfg, cs)
    _check(cs, g.expected(family), enc)
    assert enc.timing["gcm_segments"] == sum(g.segments(c.chunk.size) for c in cs)


def test_family_b_spans_reversed_with_gaps(gpu, torch_dev, cfg):
    cs, exp = g.cases("b"), g.expected("b")
    data, spans, order = g.layout_spans([c.chunk for c in cs])
    t, ptr = g.gpu_upload(torch_dev, data, pad=11)
    enc = g.gpu_encode(gpu, torch_dev, cfg, ptr, data.size, [cs[i].iv for i in order], spans=spans, pad=7)
    _check([cs[i] for i in order], [exp[i] for i in order], enc)


def test_family_c_on_a_side_stream(gpu, torch_dev, cfg):
    cs = g.cases("c")
    s = torch_dev.cuda.Stream()
    enc = _encode_chunks(gpu, torch_dev, cfg, cs, pad=9, hip_stream=s.cuda_stream)
    s.synchronize()
    _check(cs, g.expected("c"), enc)


def test_family_d_more_items_than_two_trips(gpu, torch_dev, cfg):
    """More than 2 * 3 * CUs segments in one call: every workgroup of gcm_ctr_ghash_kernel
    takes a second item and some a third; twice on one stream, so the scratch is reused."""
    ncu = torch_dev.cuda.get_device_properties(0).multi_processor_count
    cs, exp = g.cases("d", ncu), g.expected("d", ncu)
    data, _ = g.layout_chunks([c.chunk for c in cs])
    src = g.gpu_upload(torch_dev, data)
    for pad in (g.PAD, 12):
        enc = _encode_chunks(gpu, torch_dev, cfg, cs, pad=pad, src=src)
        assert enc.timing["gcm_segments"] > 2 * g.GROUPS_PER_CU * ncu
        assert enc.timing["gcm_segments"] == g.many_summary(cs)["segments"]
        _check(cs, exp, enc)


def test_family_e_four_keys_alive(gpu, torch_dev):
    """Four configs alive at once, used in alternating calls; then one closed, a config for a
    new key created, and calls under the new one and under a survivor."""
    by_key = {k: [(c, e) for c, e in zip(g.cases("e"), g.expected("e")) if c.key == k] for k in g.KEYS}
    assert all(len(v) == 8 for v in by_key.values())
    cfgs = {k: gpu.CryptConfig(k) for k in g.KEYS}
    try:
        for pad in (1, 14):
            for k in g.KEYS:
                cs, exp = zip(*by_key[k])
                _check(cs, exp, _encode_chunks(gpu, torch_dev, cfgs[k], cs, pad=pad))
        cfgs.pop(g.KEYS[1]).close()
        cfgs[g.SPARE_KEY] = gpu.CryptConfig(g.SPARE_KEY)
        _check(g.cases("e-spare"), g.expected("e-spare"), _encode_chunks(gpu, torch_dev, cfgs[g.SPARE_KEY], g.cases("e-spare")))
        cs, exp = zip(*by_key[g.KEYS[0]])
        _check(cs, exp, _encode_chunks(gpu, torch_dev, cfgs[g.KEYS[0]], cs))
    finally:
        for c in cfgs.values():
            c.close()


def test_family_f_compressed_payloads(gpu, oracle, torch_dev, cfg):
    """compress=True: the blobs equal the oracle's frames (or chunks, where the frame is no
    shorter) encrypted by the reference, and the flags those of the unencrypted encode."""
    cs = g.cases("f")
    exp = g.compressed_expected(oracle, cs)
    data, bounds = g.layout_chunks([c.chunk for c in cs])
    src = g.gpu_upload(torch_dev, data)
    enc = _encode_chunks(gpu, torch_dev, cfg, cs, compress=True, src=src)
    _check(cs, [b for b, _ in exp], enc, zstd=[z for _, z in exp])
    cap = gpu.blob_stream_bound(bounds)
    out = torch_dev.empty(cap, dtype=torch_dev.uint8, device="cuda")
    _, _, plain_comp, _ = gpu.blob_encode_chunks_device(src[1], data.size, bounds, out.data_ptr(), cap, base=g.BASE)
    assert [int(x) for x in enc.comp] == [int(x) for x in plain_comp] == [0, 0, 1, 1, 1]
    assert enc.timing["gcm_segments"] == sum(g.segments(len(b) - g.HDR) for b, _ in exp)
