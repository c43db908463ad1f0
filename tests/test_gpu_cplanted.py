"""GPU: the copy kernel of the read path on the stream of tests/cplanted.py -- kind-0 and kind-2
blobs whose lengths sit on the kernel's edges -- at every pad pair of cplanted.PADS, through
pbs_blob_decode_device (packed output) and pbs_blob_decode_inflate_device (slots: exact, 9 bytes
roomier, one cut under its payload).  Expected bytes are the payloads themselves; every byte
outside the slots and past out_lens inside them must keep its fill, and the input must stay as
it was.  One kind-2 blob has a flipped tag bit: zeros over its whole slot, intact neighbours.
test_cplanted_cpu.py proves that these pairs show every alignment.

Run on an MI355X:  python -m pytest tests/test_gpu_cplanted.py -m gpu -x -q
"""
import functools

import numpy as np
import pytest

import cplanted as c
import dplanted as d
import gplanted as g

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD = 256
OK, BAD_TAG, BAD_SIZE = d.OK, d.BAD_TAG, d.BAD_SIZE


@pytest.fixture(scope="module")
def torch_dev(gpu):
    import torch

    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def cfg(gpu):
    with gpu.CryptConfig(g.KEY1) as cc:
        yield cc


@pytest.fixture(scope="module")
def uploads(torch_dev, oracle):
    """in_pad -> (tensor, lead, untouched copy): the blob stream, uploaded once per residue"""
    data, _ = d.layout(c.items(oracle))
    out = {}
    for ip in c.IN_PADS:
        t, lead = d.gpu_upload(torch_dev, data, ip)
        out[ip] = (t, lead, t.clone())
    return out


@functools.lru_cache(maxsize=None)
def wanted(items, mode):
    """(slot sizes, out_lens, status, the slots' bytes back to back) of one inflate run of the
    items (a tuple); computed once per mode and left unchanged"""
    sizes = c.slot_sizes(mode)
    lens, status, img = [], [], []
    for i, (it, size) in enumerate(zip(items, sizes)):
        pay = np.frombuffer(it.payload, np.uint8)
        n = 0 if i == c.BAD_AT else min(pay.size, size)
        lens.append(n)
        status.append(BAD_TAG if i == c.BAD_AT else OK if pay.size <= size else BAD_SIZE)
        # (the bad blob: zeros over the whole slot, roomier or not)
        img.append(np.zeros(size, np.uint8) if i == c.BAD_AT else np.concatenate([pay[:n], np.full(size - n, FILL, np.uint8)]))
    return sizes, lens, status, np.concatenate(img)


def run_slots(gpu, torch, cfg, items, src, out_pad, mode, where):
    t, lead, before = src
    sizes, lens_w, status_w, img_w = wanted(tuple(items), mode)
    _, offs = d.layout(items)
    cap = int(sum(sizes))
    out = torch.full((32 + cap + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    olead = (-out.data_ptr()) % 16 + out_pad
    exact = mode == "exact"  # digests of every blob and verify_unencrypted's length in this mode
    dig = np.frombuffer(b"".join(it.digest for it in items), np.uint8) if exact else None
    torch.cuda.synchronize()
    oo, lens, kinds, status, _ = gpu.blob_decode_inflate_device(
        t.data_ptr() + lead, offs, out.data_ptr() + olead, cap, np.array(sizes, np.uint64), crypt=cfg, expect_digests=dig,
        sizes_exact=exact)
    torch.cuda.synchronize()
    img = out.cpu().numpy()
    assert torch.equal(t, before), f"{where}: the input was written"
    assert [int(x) for x in oo] == [int(x) for x in np.concatenate([[0], np.cumsum(sizes)])], where
    assert [int(k) for k in kinds] == list(c.PKINDS), where
    assert [int(s) for s in status] == status_w and [int(x) for x in lens] == lens_w, where
    assert (img[:olead] == FILL).all() and (img[olead + cap:] == FILL).all(), f"{where}: bytes outside the slots were written"
    got = img[olead:olead + cap]
    if not np.array_equal(got, img_w):
        at = int(np.flatnonzero(got != img_w)[0])
        i = int(np.searchsorted(np.cumsum(sizes), at, side="right"))
        pytest.fail(f"{where}: {items[i].label}: slot byte {at - int(oo[i])} of {sizes[i]} is {got[at]:#x}, wanted "
                    f"{img_w[at]:#x} (slot at residue {(out_pad + int(oo[i])) % 16}, out_len {lens_w[i]})")


@pytest.mark.parametrize("out_pad", c.OUT_PADS)
def test_copies_at_every_alignment(gpu, torch_dev, cfg, oracle, uploads, out_pad):
    items = c.items(oracle)
    for in_pad in c.IN_PADS:
        where = f"input pad {in_pad}, output pad {out_pad}"
        dec = d.gpu_decode(gpu, torch_dev, cfg, items, pad=in_pad, out_pad=out_pad, src=uploads[in_pad][:2])
        assert not d.mismatches(items, dec), where
        assert dec.input_unchanged and dec.outside_clean, where
        for mode in c.MODES:
            run_slots(gpu, torch_dev, cfg, items, uploads[in_pad], out_pad, mode, f"{where}, {mode} slots")
