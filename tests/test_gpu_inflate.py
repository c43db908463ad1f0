"""GPU parity of the zstd inflater (csrc/pbs_inflate.hip) on the frames of tests/iplanted.py.

Every frame's status and bytes must equal the host mirror's (the same format code run serially)
and obey libzstd's verdict (iplanted.check); the input stays as it was; every output byte outside
[slot start, slot start + out_lens) keeps its fill, the guard behind the last slot included, so a
bad frame cannot touch its neighbours.  Bad frames are data: no case hands the library a bad
pointer or offset.

Run on an MI355X:  python -m pytest tests/test_gpu_inflate.py -m gpu -x -q
"""
import numpy as np
import pytest

import iplanted as ip

pytestmark = pytest.mark.gpu

FILL = 0xA5
GROUPS_PER_CU = 4  # pbs_inflate.hip kGroupsPerCuMax: the launch keeps what is resident per CU, at most this


@pytest.fixture(scope="module")
def torch_dev(gpu):
    import torch

    torch.cuda.set_device(0)
    return torch


_mirror = {}


def mirror(gpu, it):
    """(bytes, status) of the host mirror, computed once per item."""
    key = (it.label, it.cap)
    if key not in _mirror:
        _mirror[key] = gpu.zstd_inflate_host(it.frame, it.cap)
    return _mirror[key]


def run(gpu, torch, items, pad=0, out_pad=0, hip_stream=0):
    data, foff, ooff, out_size = ip.layout(items, pad, out_pad)
    src = torch.from_numpy(data.copy()).cuda()
    out = torch.full((out_size,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    lens, status, timing = gpu.zstd_inflate_device(src.data_ptr(), foff, out.data_ptr(), ooff, hip_stream=hip_stream)
    torch.cuda.synchronize()
    assert np.array_equal(src.cpu().numpy(), data), "the input buffer was written"
    return out.cpu().numpy(), ooff, lens, status, timing


def verify(gpu, items, img, ooff, lens, status):
    wrong = []
    keep = np.ones(img.size, dtype=bool)  # bytes that must still hold the fill
    for i, it in enumerate(items):
        o, n = int(ooff[i]), int(lens[i])
        if n > it.cap:
            wrong.append(f"{it.label}: out_lens {n} above the slot {it.cap}")
            continue
        got = img[o:o + n].tobytes()
        keep[o:o + n] = False
        msg = ip.check(it, int(status[i]), got)
        if msg:
            wrong.append(msg)
        mb, ms = mirror(gpu, it)
        if (int(status[i]), got) != (ms, mb):
            wrong.append(f"{it.label}: status {status[i]} / {n} bytes, the host mirror has {ms} / {len(mb)}")
    assert not wrong, f"{len(wrong)} of {len(items)} items:\n" + "\n".join(wrong[:20])
    assert np.all(img[keep] == FILL), "bytes outside [slot start, slot start + out_lens) were written"


def test_whole_corpus_in_one_call(gpu, torch_dev):
    items = ip.interleaved()
    img, ooff, lens, status, timing = run(gpu, torch_dev, items, pad=3, out_pad=5)
    verify(gpu, items, img, ooff, lens, status)
    assert timing["frames"] == len(items)
    assert timing["failed"] == int(np.count_nonzero(status))
    assert timing["bytes_out"] == int(lens.sum())


def test_hand_frames_at_every_residue(gpu, torch_dev):
    """16 residues of the frames' start x 4 of the slots': every load and store alignment."""
    c = ip.corpus()
    items = [it for it in c["good"] if it.family == "hand"] + [it for it in c["bad"] if it.label.startswith("hand-")]
    for pad in range(16):
        for out_pad in range(4):
            img, ooff, lens, status, _ = run(gpu, torch_dev, items, pad=pad, out_pad=out_pad)
            verify(gpu, items, img, ooff, lens, status)


def test_more_frames_than_two_trips_of_the_grid_and_no_new_allocation(gpu, torch_dev):
    import random

    r = random.Random(5)
    src = ip.text(40_000, 41)
    items = []
    for i in range(4096):
        n = r.randint(100, 2000)
        at = r.randint(0, len(src) - n)
        data = src[at:at + n]
        items.append(ip.Item(f"small-{i}", ip.zstd_compress(data, level=1), n, data, ip.OK, "libzstd"))
    cus = torch_dev.cuda.get_device_properties(0).multi_processor_count
    assert len(items) > 2 * cus * GROUPS_PER_CU, "every workgroup must come back to the counter more than once"
    img, ooff, lens, status, timing = run(gpu, torch_dev, items, pad=1)
    verify(gpu, items, img, ooff, lens, status)
    assert cus <= timing["workgroups"] <= cus * GROUPS_PER_CU and 2 * timing["workgroups"] < len(items)
    before = gpu.debug_arena_allocs()
    img, ooff, lens, status, _ = run(gpu, torch_dev, items, pad=1)
    verify(gpu, items, img, ooff, lens, status)
    assert gpu.debug_arena_allocs() == before, "a repeated call allocated device memory"


def test_side_stream(gpu, torch_dev):
    items = ip.interleaved()[:120]
    s = torch_dev.cuda.Stream()
    img, ooff, lens, status, _ = run(gpu, torch_dev, items, pad=7, out_pad=1, hip_stream=s.cuda_stream)
    s.synchronize()
    verify(gpu, items, img, ooff, lens, status)


def test_one_16_mib_frame_beside_63_small_ones(gpu, torch_dev, oracle):
    """The largest chunk at the 4 MiB average: 128 blocks on one workgroup, offsets across many
    blocks, while the other workgroups finish the small frames."""
    big = oracle.gen_vmimage(16 << 20, 51).tobytes()
    frame = ip.zstd_compress(big, level=1, contentSizeFlag=0)
    assert oracle.zstd_decompress(frame, len(big)) == big
    small = [it for it in ip.corpus()["good"] if len(it.frame) < 8192]
    small = (small * (63 // len(small) + 1))[:63]
    assert len(small) == 63
    items = small[:31] + [ip.Item("big-16MiB", frame, len(big), big, ip.OK, "libzstd")] + small[31:]
    img, ooff, lens, status, _ = run(gpu, torch_dev, items, out_pad=2)
    verify(gpu, items, img, ooff, lens, status)
