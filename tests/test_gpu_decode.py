"""GPU parity of the read side (csrc/pbs_decode.hip: classify, per-blob CRC, payload copy,
AES-256-GCM open, digests, verdicts) on the planted blobs of tests/dplanted.py.

Every payload must equal the wanted one byte for byte, with out_offsets, kinds and status; the
input buffer stays as it was; every output byte outside [0, out_offsets[n]) keeps its fill,
the guard behind pbs_blob_decode_bound included; a failed encrypted blob leaves zeros; the
neighbours of a corrupted blob are untouched by it.  One decode call per family (family a: one
per pair of residues).  The blobs come from tests/aesgcm_ref.py and the oracle, the wanted
statuses are proved on the CPU by test_dplanted_cpu.py.  Bad blobs are data: no case hands the
library a bad pointer or offset.

Run on an MI355X:  python -m pytest tests/test_gpu_decode.py -m gpu -x -q
"""
import hashlib

import numpy as np
import pytest

import dplanted as d
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


def _check(items, dec):
    bad = d.mismatches(items, dec)
    assert not bad, f"{len(bad)} of {len(items)} items:\n" + "\n".join(bad[:20])
    assert dec.input_unchanged, "the input buffer was written"
    assert dec.outside_clean, "bytes outside [0, out_offsets[n]) were written"
    for it, pay in zip(items, dec.payloads):  # (implied by the byte equality; stated for the contract)
        if it.kind in (2, 3) and it.status != d.OK:
            assert not any(pay), f"{it.label}: unauthenticated bytes left in the output"
    assert dec.timing["failed"] == sum(it.status != d.OK for it in items)
    assert dec.timing["bytes_out"] == sum(len(it.payload) for it in items)


def test_family_a_every_tail_at_every_residue_triple(gpu, torch_dev, cfg):
    """Lengths 0..600 in one call, at each of the 16 residues of the blob stream's start and 8
    of the packed output's: every (length mod 16, source residue, destination residue)."""
    items = d.stream("a")
    data, _ = d.layout(items)
    for pad in g.TAIL_PADS:
        src = d.gpu_upload(torch_dev, data, pad)
        for out_pad in d.OUT_PADS:
            dec = d.gpu_decode(gpu, torch_dev, cfg, items, out_pad=out_pad, src=src)
            _check(items, dec)
            assert dec.timing["gcm_segments"] == 600


@pytest.mark.parametrize("family", ["b", "c"])
def test_family_open(gpu, torch_dev, cfg, family):
    items = d.stream(family)
    dec = d.gpu_decode(gpu, torch_dev, cfg, items)
    _check(items, dec)
    assert dec.timing["gcm_segments"] == sum(g.segments(len(it.payload)) for it in items)


def test_family_c_on_a_side_stream_without_expectations(gpu, torch_dev, cfg):
    items = d.stream("c")
    s = torch_dev.cuda.Stream()
    dec = d.gpu_decode(gpu, torch_dev, cfg, items, pad=11, out_pad=2, use_digests=False, use_sizes=False,
                       hip_stream=s.cuda_stream)
    s.synchronize()
    _check(items, dec)


def test_family_d_more_items_than_two_trips(gpu, torch_dev, cfg):
    """More than 2 * 3 * CUs segments in one call: every workgroup of gcm_open_kernel takes a
    second item and some a third; twice on one stream, so the scratch is reused."""
    ncu = torch_dev.cuda.get_device_properties(0).multi_processor_count
    items = d.stream("d", None, ncu)
    data, _ = d.layout(items)
    src = d.gpu_upload(torch_dev, data, 5)
    allocs = None
    for out_pad in (9, 12):
        dec = d.gpu_decode(gpu, torch_dev, cfg, items, out_pad=out_pad, src=src)
        assert dec.timing["gcm_segments"] > 2 * g.GROUPS_PER_CU * ncu
        assert dec.timing["gcm_segments"] == g.many_summary(g.cases("d", ncu))["segments"]
        _check(items, dec)
        if allocs is not None:
            assert gpu.debug_arena_allocs() == allocs, "the second call allocated device scratch"
        allocs = gpu.debug_arena_allocs()


def test_family_e_several_configs_alive(gpu, torch_dev):
    """Four configs alive at once, used in alternating calls; a blob opened under another
    key's config fails its tag and leaves zeros."""
    by_key = {k: [it for c, it in zip(g.cases("e"), d.stream("e")) if c.key == k] for k in g.KEYS}
    assert all(len(v) == 8 for v in by_key.values())
    cfgs = {k: gpu.CryptConfig(k) for k in g.KEYS}
    try:
        for pad in (1, 14):
            for k in g.KEYS:
                _check(by_key[k], d.gpu_decode(gpu, torch_dev, cfgs[k], by_key[k], pad=pad, out_pad=15 - pad))
        crossed = [d.bad(it.label + "/other-key", it, it.blob, d.BAD_TAG) for it in by_key[g.KEYS[0]]]
        _check(crossed, d.gpu_decode(gpu, torch_dev, cfgs[g.KEYS[3]], crossed))
        cfgs.pop(g.KEYS[1]).close()
        _check(by_key[g.KEYS[2]], d.gpu_decode(gpu, torch_dev, cfgs[g.KEYS[2]], by_key[g.KEYS[2]]))
    finally:
        for c in cfgs.values():
            c.close()


def test_family_f_compressed_payloads(gpu, oracle, torch_dev, cfg):
    """The frames handed back equal the oracle's; inflated (the caller's step) they give the
    chunks, whose digests the caller checks."""
    items = d.stream("f", oracle)
    dec = d.gpu_decode(gpu, torch_dev, cfg, items)
    _check(items, dec)
    chunks = [c.chunk.tobytes() for c in g.cases("f") for _ in (0, 1)]
    assert sorted({int(k) for k in dec.kinds}) == [0, 1, 2, 3]
    for it, pay, chunk in zip(items, dec.payloads, chunks):
        plain = oracle.blob_compressed(chunk)
        assert pay == plain[d.HDR:], it.label
        data = oracle.zstd_decompress(pay, len(chunk)) if it.kind in (1, 3) else pay
        assert data == chunk and hashlib.sha256(data).digest() == hashlib.sha256(chunk).digest(), it.label


def test_family_g_mixed_stream(gpu, oracle, torch_dev, cfg):
    items = d.stream("g", oracle)
    _check(items, d.gpu_decode(gpu, torch_dev, cfg, items))
    _check(items, d.gpu_decode(gpu, torch_dev, cfg, items, pad=0, out_pad=0))


def test_family_h_corruptions_between_intact_neighbours(gpu, oracle, torch_dev, cfg):
    items = d.stream("h", oracle)
    dec = d.gpu_decode(gpu, torch_dev, cfg, items)
    _check(items, dec)
    for i in range(0, len(items), 2):  # the neighbours of every corrupted blob
        assert int(dec.status[i]) == d.OK and dec.payloads[i] == items[i].payload, items[i].label
    assert {int(s) for s in dec.status} == set(range(8)) - {d.NO_CONFIG}


def test_family_h_without_a_config(gpu, oracle, torch_dev):
    items = d.stream("h-nocfg", oracle)
    dec = d.gpu_decode(gpu, torch_dev, None, items)
    _check(items, dec)
    assert dec.timing["gcm_segments"] == 0 and d.NO_CONFIG in {int(s) for s in dec.status}


@pytest.mark.parametrize("crypt,compress", [(False, False), (False, True), (True, False), (True, True)])
def test_round_trip_of_the_device_encoder(gpu, oracle, torch_dev, cfg, crypt, compress):
    """blob_encode_chunks_device (fixed IVs), then blob_decode_device: the stream comes back,
    status all OK, with the digests of digest_chunks_device as the expected ones."""
    import corpus_gen

    parts = [corpus_gen.text(150000, 3), g._bytes(77, 70001), np.zeros(0, np.uint8), np.zeros(70000, np.uint8),
             g._bytes(78, 13), corpus_gen.text(5000, 4)]
    data = np.concatenate(parts)
    bounds = np.concatenate([[0], np.cumsum([p.size for p in parts])]).astype(np.uint64)
    n = len(parts)
    t = torch_dev.from_numpy(data.copy()).to("cuda")
    c = cfg if crypt else None
    dig = gpu.digest_chunks_device(t.data_ptr(), data.size, bounds, key=c.id_key if crypt else None)
    cap = gpu.blob_stream_bound_encrypted(bounds) if crypt else gpu.blob_stream_bound(bounds)
    blobs = torch_dev.full((cap + 64,), 0x33, dtype=torch_dev.uint8, device="cuda")
    ivs = [g._iv(9000 + i) for i in range(n)] if crypt else None
    offs, _, comp, _ = gpu.blob_encode_chunks_device(t.data_ptr(), data.size, bounds, blobs.data_ptr() + 3, cap,
                                                     compress=compress, crypt=c, ivs=ivs)
    ocap = gpu.blob_decode_bound(offs)
    out = torch_dev.full((ocap + d.GUARD,), d.FILL_OUT, dtype=torch_dev.uint8, device="cuda")
    oo, kinds, status, _ = gpu.blob_decode_device(blobs.data_ptr() + 3, offs, out.data_ptr(), ocap, crypt=c,
                                                  expect_digests=dig, expect_sizes=[p.size for p in parts])
    torch_dev.cuda.synchronize()
    img = out.cpu().numpy()
    assert [int(s) for s in status] == [d.OK] * n
    assert [int(k) for k in kinds] == [2 * crypt + int(z) for z in comp]
    assert compress == bool(comp.any())
    for i, p in enumerate(parts):
        pay = img[int(oo[i]):int(oo[i + 1])].tobytes()
        if comp[i]:
            pay = oracle.zstd_decompress(pay, p.size)
            assert hashlib.sha256(pay + (c.id_key if crypt else b"")).digest() == dig[i].tobytes()
        assert pay == p.tobytes(), i
    assert (img[int(oo[-1]):] == d.FILL_OUT).all()


def test_capacity_one_below_the_bound(gpu, torch_dev, cfg):
    items = d.stream("c")
    data, offs = d.layout(items)
    t, lead = d.gpu_upload(torch_dev, data, 3)
    cap = gpu.blob_decode_bound(offs)
    assert cap == int(offs[-1]) - d.HDR * len(items)
    out = torch_dev.full((cap + 64,), d.FILL_OUT, dtype=torch_dev.uint8, device="cuda")
    with pytest.raises(gpu.ChunkerError) as e:
        gpu.blob_decode_device(t.data_ptr() + lead, offs, out.data_ptr(), cap - 1, crypt=cfg)
    assert e.value.code == gpu.PBS_ERR_CAPACITY
    torch_dev.cuda.synchronize()
    assert bool((out == d.FILL_OUT).all()), "the output was written before the capacity check"
    offs_, kinds, status, _ = gpu.blob_decode_device(0, [0], 0, 0)
    assert offs_.tolist() == [0] and kinds.size == 0 and status.size == 0


def test_mismatch_report_names_block_segment_row_and_lane():
    """The report the assertions above print, on a made-up difference (no GPU work)."""
    it = d.stream("b")[-1]
    n = len(it.payload)
    at = 16 * (1 + 4096 + 256 + 7) + 3  # segment 2 (first = 1), row 1, lane 7
    got = bytearray(it.payload)
    got[at] ^= 1
    dec = d.Decoded([bytes(got)], np.array([0, n]), np.array([2]), np.array([0]), True, True, {})
    (line,) = d.mismatches([it], dec)
    assert it.label in line and f"byte {at} " in line
    assert f"GCM block {at // 16} of 65537" in line and "segment 2 of 17, row 1, lane 7 " in line
    dec = d.Decoded([it.payload], np.array([0, n]), np.array([2]), np.array([d.BAD_TAG]), True, True, {})
    assert "BAD_TAG" in d.mismatches([it], dec)[0]
