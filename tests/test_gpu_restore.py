"""GPU: the restore path of include/pbs_restore.h (csrc/pbs_restore.hip) -- the digest lookup
against its host mirror, the segment copy kernel against numpy at every alignment pair, and
pbs_restore_range_device / restore_stream_device against the Python concatenation of the
chunks, with blobs made by tests/dplanted.py's make_blob and by the device encoder.

Run on an MI355X:  python -m pytest tests/test_gpu_restore.py -m gpu -x -q
"""
import hashlib
from typing import NamedTuple

import numpy as np
import pytest

import dplanted as d
import gplanted as g
import rplanted as r

pytestmark = pytest.mark.gpu

FILL = 0xA5
INVALID = -6
OK, BAD_CRC, NO_CONFIG, BAD_DIGEST, MISSING, NOT_REQUESTED = 0, 3, 4, 6, 10, 255


@pytest.fixture(scope="module")
def torch_dev(gpu):
    import torch

    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def cfg(gpu):
    with gpu.CryptConfig(g.KEY1) as c:
        yield c


def to_dev(torch, a: np.ndarray):
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


# ---- lookup -----------------------------------------------------------------------------------

def lookup_on_device(gpu, torch, index, store):
    di, ds = to_dev(torch, index.reshape(-1)), to_dev(torch, store.reshape(-1)) if store.size else None
    n, m = index.shape[0], store.shape[0]
    pos = torch.full((n,), 0x7FFFFFFF, dtype=torch.int32, device="cuda")
    first = torch.full((n,), 0x7FFFFFFF, dtype=torch.int32, device="cuda")
    assert di.data_ptr() % 16 == 0 and (ds is None or ds.data_ptr() % 16 == 0)
    nm, nu = gpu.digest_lookup_device(di.data_ptr(), n, ds.data_ptr() if m else 0, m, pos.data_ptr(), first.data_ptr())
    torch.cuda.synchronize()
    assert np.array_equal(di.cpu().numpy(), index.reshape(-1)), "the index digests were written"
    return pos.cpu().numpy().view(np.uint32), first.cpu().numpy().view(np.uint32), nm, nu


def test_lookup_planted_sets_match_the_host_mirror(gpu, torch_dev):
    index, store = r.planted_lookup_sets()
    want = gpu.digest_lookup_host(index, store)
    model = r.model_lookup(index, store)
    assert np.array_equal(want[0], model[0]) and np.array_equal(want[1], model[1]) and want[2:] == model[2:]
    got = lookup_on_device(gpu, torch_dev, index, store)
    assert np.array_equal(got[0], want[0]), np.flatnonzero(got[0] != want[0])
    assert np.array_equal(got[1], want[1]), np.flatnonzero(got[1] != want[1])
    assert got[2:] == want[2:]
    # an empty store: everything is missing, the grouping stays
    got = lookup_on_device(gpu, torch_dev, index, np.zeros((0, 32), np.uint8))
    assert (got[0] == r.MISSING).all() and np.array_equal(got[1], want[1]) and got[2] == index.shape[0]


def test_lookup_of_many_digests_uses_several_sort_tiles(gpu, torch_dev):
    n, m = 70_000, 50_000
    rng = np.random.default_rng(0x6D616E79)
    pool = rng.integers(0, 256, (110_000, 32), dtype=np.uint8)
    pool[100:140, :8] = pool[100, :8]        # forty digests in one prefix run, on both sides
    pool[200:204, :31] = pool[200, :31]
    pool[200:204, 31] = [1, 2, 3, 4]
    index = pool[rng.integers(0, 92_000, n)]                  # about 30 % of the entries repeat an earlier one
    index[rng.integers(0, n, 2000)] = pool[100:140][rng.integers(0, 40, 2000)]
    store = pool[rng.integers(20_000, 110_000, m)]            # unsorted, with duplicates; pool[:20000] is absent
    store[rng.integers(0, m, 300)] = pool[100:140:2][rng.integers(0, 20, 300)]
    want = gpu.digest_lookup_host(index, store)
    assert 0.27 < 1 - want[3] / n < 0.35 and 0 < want[2] < n
    got = lookup_on_device(gpu, torch_dev, index, store)
    assert np.array_equal(got[0], want[0]), np.flatnonzero(got[0] != want[0])[:10]
    assert np.array_equal(got[1], want[1]), np.flatnonzero(got[1] != want[1])[:10]
    assert got[2:] == want[2:]


# ---- the copy kernel --------------------------------------------------------------------------

ALIGNS = (0, 1, 7, 8, 15)
LENGTHS = (0, 1, 15, 16, 17, 31, 255, 4096, 65535, 65536, 65537, 131073)


def copy_segments():
    """(src_off, dst_off, lens): every alignment pair with every length, one 3 MiB segment, and
    one source fanned out to five destinations; offsets relative to 16-byte aligned bases, the
    destinations 48 or more bytes apart."""
    so, do, ln = [], [], []
    s = t = 0
    for sa in ALIGNS:
        for da in ALIGNS:
            for n in LENGTHS:
                so.append(s + sa)
                do.append(t + da)
                ln.append(n)
                s += (sa + n + 15) // 16 * 16 + 16
                t += (da + n + 15) // 16 * 16 + 48
    so.append(s + 3)
    do.append(t + 9)
    ln.append(3 << 20)
    s += (3 << 20) + 32
    t += (3 << 20) + 64
    for k, da in enumerate((0, 5, 8, 11, 15)):
        so.append(s + 13)
        do.append(t + da)
        ln.append(100_003)
        t += 100_003 + 15 + 48
    s += 100_003 + 32
    return np.array(so, np.uint64), np.array(do, np.uint64), np.array(ln, np.uint64), s, t


def test_copy_segments_every_alignment_and_length(gpu, torch_dev):
    so, do, ln, slen, dlen = copy_segments()
    src_host = np.random.default_rng(0x636F7079).integers(0, 256, slen, dtype=np.uint8)
    src = torch_dev.empty(slen + 16, dtype=torch_dev.uint8, device="cuda")
    dst = torch_dev.full((dlen + 16,), FILL, dtype=torch_dev.uint8, device="cuda")
    sl, dl = (-src.data_ptr()) % 16, (-dst.data_ptr()) % 16
    src[sl:sl + slen] = to_dev(torch_dev, src_host)
    before = src.clone()
    torch_dev.cuda.synchronize()
    gpu.copy_segments_device(src.data_ptr() + sl, dst.data_ptr() + dl, so, do, ln)
    torch_dev.cuda.synchronize()
    model = np.full(dlen + 16, FILL, np.uint8)
    for a, b, n in zip(so, do, ln):
        model[dl + int(b):dl + int(b) + int(n)] = src_host[int(a):int(a) + int(n)]
    img = dst.cpu().numpy()
    bad = np.flatnonzero(img != model)
    if bad.size:
        at = int(bad[0]) - dl
        k = int(np.searchsorted(do, at, side="right")) - 1
        pytest.fail(f"{bad.size} bytes differ, first at destination byte {at}: segment {k} (src +{int(so[k]) % 16}, "
                    f"dst +{int(do[k]) % 16}, {int(ln[k])} bytes) byte {at - int(do[k])}; got {img[bad[0]]:#x}, "
                    f"wanted {model[bad[0]]:#x}")
    assert torch_dev.equal(src, before), "the source was written"


def test_copy_segments_refuses_overlap(gpu, torch_dev):
    buf = torch_dev.full((4096,), FILL, dtype=torch_dev.uint8, device="cuda")
    src = to_dev(torch_dev, np.arange(4096, dtype=np.uint32).astype(np.uint8))
    cases = [
        ([0, 100], [10, 109], [100, 50]),        # two destinations share one byte
        ([0, 0], [500, 500], [1, 1]),            # the same destination twice
        ([0, 0, 0], [0, 2000, 1990], [1000, 10, 11]),   # the third reaches one byte into the second
    ]
    for so, do, ln in cases:
        with pytest.raises(gpu.ChunkerError) as e:
            gpu.copy_segments_device(src.data_ptr(), buf.data_ptr(), so, do, ln)
        assert e.value.code == INVALID
    with pytest.raises(gpu.ChunkerError) as e:   # a destination inside a source of the same buffer
        gpu.copy_segments_device(buf.data_ptr(), buf.data_ptr(), [0, 2000], [1000, 99], [100, 1])
    assert e.value.code == INVALID
    torch_dev.cuda.synchronize()
    assert bool((buf == FILL).all()), "a refused call wrote"
    # touching segments and empty ones anywhere are fine
    gpu.copy_segments_device(src.data_ptr(), buf.data_ptr(), [0, 100, 7], [10, 110, 50], [100, 50, 0])
    torch_dev.cuda.synchronize()
    img = buf.cpu().numpy()
    want = np.full(4096, FILL, np.uint8)
    want[10:110] = np.arange(100)
    want[110:160] = np.arange(100, 150)
    assert np.array_equal(img, want)


# ---- restore ----------------------------------------------------------------------------------

class Store(NamedTuple):
    ends: np.ndarray         # the index
    digests: np.ndarray
    chunks: list             # per index entry: the chunk's bytes
    status: list             # per index entry: the wanted status with the key
    blobs: np.ndarray        # the store's blob stream
    offsets: np.ndarray
    store_digests: np.ndarray
    compressed: set          # digests whose store blob holds a zstd frame
    encrypted: set           # digests whose store blob is encrypted


def _text(n, seed):
    import corpus_gen

    return corpus_gen.text(n + 64, seed)[:n].tobytes()


def _rand(n, seed):
    return np.random.default_rng([0x7273, seed]).integers(0, 256, n, dtype=np.uint8).tobytes()


@pytest.fixture(scope="module")
def store(oracle) -> Store:
    chunks = {  # name -> (kind asked of make_blob, bytes)
        "empty0": (0, b""), "one2": (2, _rand(1, 1)), "text1": (1, _text(4096, 2)), "zeros3": (3, bytes(4096)),
        "rand0": (0, _rand(70_000, 3)), "text1L": (1, _text(70_000, 4)), "rand2": (2, _rand(70_000, 5)),
        "text3": (3, _text(70_000, 6)), "zeros1": (1, bytes(200_001)), "text3L": (3, _text(200_001, 7)),
        "rand0L": (0, _rand(200_001, 8)), "rand2s": (2, _rand(4096, 9)), "one1": (1, _rand(1, 10)),
        "empty2": (2, b""), "flip0": (0, _rand(4096, 11)), "filed0": (0, _rand(70_000, 12)),
        "absent": (0, _rand(4096, 13)),
    }
    digest = {k: (d.keyed_digest(c, g.KEY1) if kind >= 2 else d.plain_digest(c)) for k, (kind, c) in chunks.items()}
    blob = {k: d.make_blob(oracle, kind, c, g.KEY1, g._iv(9100 + i)) for i, (k, (kind, c)) in enumerate(chunks.items())}
    assert {d.kind_of(b) for b in blob.values()} == {0, 1, 2, 3}
    blob["flip0"] = d._flip(blob["flip0"], d.HDR + 1000, 3)                       # a payload byte: the CRC is stale
    blob["filed0"] = d.make_blob(oracle, 0, _rand(70_000, 14), g.KEY1, g._iv(1))  # another chunk of the same length
    extras = [d.make_blob(oracle, k, _rand(3000 + k, 20 + k), g.KEY1, g._iv(9200 + k)) for k in (0, 1, 2)]
    filed = [(digest[k], blob[k]) for k in chunks if k != "absent"]
    filed += [(d.plain_digest(_rand(3000 + k, 20 + k) + b"x"), b) for k, b in zip((0, 1, 2), extras)]
    filed.append((digest["text1L"], blob["text1L"]))                              # a duplicate filing, later in the store
    order = np.random.default_rng(0x73746F72).permutation(len(filed))
    filed = [filed[int(i)] for i in order]
    names = ["rand0", "text1", "text1L", "text1L", "text1L", "empty0", "text3L", "one2", "zeros3", "rand2", "absent",
             "text3", "zeros1", "empty2", "rand0L", "rand2s", "one1", "flip0", "text1", "filed0", "rand0", "zeros3",
             "text3L", "one2", "absent", "rand2s", "text3", "flip0", "zeros1", "empty0", "rand2", "text1L", "one1",
             "filed0", "text1", "rand0L", "zeros3", "one2", "text3L", "rand0"]
    assert set(names) == set(chunks) and len(names) == 40
    want = {"absent": MISSING, "flip0": BAD_CRC, "filed0": BAD_DIGEST}
    return Store(np.cumsum([len(chunks[k][1]) for k in names]).astype(np.uint64),
                 np.frombuffer(b"".join(digest[k] for k in names), np.uint8).reshape(-1, 32),
                 [chunks[k][1] for k in names], [want.get(k, OK) for k in names],
                 np.frombuffer(b"".join(b for _, b in filed), np.uint8),
                 np.concatenate([[0], np.cumsum([len(b) for _, b in filed])]).astype(np.uint64),
                 np.frombuffer(b"".join(dg for dg, _ in filed), np.uint8).reshape(-1, 32),
                 {digest[k] for k in chunks if d.kind_of(blob[k]) in (1, 3)},
                 {digest[k] for k in chunks if d.kind_of(blob[k]) in (2, 3)})


@pytest.fixture(scope="module")
def store_dev(torch_dev, store):
    t = torch_dev.full((store.blobs.size + 64,), 0x5A, dtype=torch_dev.uint8, device="cuda")
    t[7:7 + store.blobs.size] = to_dev(torch_dev, store.blobs)     # (the store at an odd address)
    return t


def restore(gpu, torch, store, store_dev, crypt, offset, length, pad=3, **kw):
    """One call into a filled buffer; (output bytes, status, timing)."""
    before = store_dev.clone()
    n = int(store.ends[-1]) - offset if length is None else length
    out = torch.full((pad + n + 256,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    status, timing = gpu.restore_range_device((store.ends, store.digests), store_dev.data_ptr() + 7, store.offsets,
                                              store.store_digests, out.data_ptr() + pad, offset, length, crypt=crypt, **kw)
    torch.cuda.synchronize()
    assert torch.equal(store_dev, before), "the store was written"
    img = out.cpu().numpy()
    assert (img[:pad] == FILL).all() and (img[pad + n:] == FILL).all(), "bytes outside out_dev[0 .. len) were written"
    return img[pad:pad + n].tobytes(), status, timing


def expected(store, offset, length, no_config=False):
    """(bytes, status per entry, distinct present digests, distinct compressed ones) of a range."""
    py = [int(e) for e in store.ends]
    status = [NO_CONFIG if no_config and s == OK and store.digests[i].tobytes() in store.encrypted else s
              for i, s in enumerate(store.status)]
    archive = b"".join(c if s == OK else bytes(len(c)) for c, s in zip(store.chunks, status))
    want = [NOT_REQUESTED] * len(py)
    present = set()
    if length:
        i0, i1 = r.ref_chunk_from_offset(py, offset)[0], r.ref_chunk_from_offset(py, offset + length - 1)[0]
        want[i0:i1 + 1] = status[i0:i1 + 1]
        present = {store.digests[i].tobytes() for i in range(i0, i1 + 1) if status[i] != MISSING}
    # (a compressed blob reaches the inflater only when it loads and opens: none of the bad ones is compressed)
    frames = {x for x in present if x in store.compressed and not (no_config and x in store.encrypted)}
    return archive[offset:offset + length], want, len(present), len(frames)


def ranges(store):
    py = [0] + [int(e) for e in store.ends]
    total = py[-1]
    return [("whole", 0, total), ("empty-at-0", 0, 0), ("empty-at-end", total, 0),
            ("inside-one-chunk", py[6] + 1001, 50_001), ("mid-3-to-mid-9", py[3] + 33_333, py[9] + 35_001 - py[3] - 33_333),
            ("boundaries-2-to-6", py[2], py[7] - py[2]), ("boundary-to-end", py[30], total - py[30]),
            ("one-entry", py[14], py[15] - py[14]), ("last-byte", total - 1, 1), ("first-byte", 0, 1),
            ("over-failed-entries", py[16] + 1, py[20] - py[16] + 5)]


@pytest.mark.parametrize("which", range(11))
def test_restore_ranges(gpu, torch_dev, cfg, store, store_dev, which):
    name, offset, length = ranges(store)[which]
    want_bytes, want_status, uniq, frames = expected(store, offset, length)
    got, status, timing = restore(gpu, torch_dev, store, store_dev, cfg, offset, length, allow_bad=True)
    assert [int(s) for s in status] == want_status, name
    if got != want_bytes:
        a, b = np.frombuffer(got, np.uint8), np.frombuffer(want_bytes, np.uint8)
        at = int(np.flatnonzero(a != b)[0])
        i, within = r.ref_chunk_from_offset([int(e) for e in store.ends], offset + at)
        pytest.fail(f"{name}: output differs at byte {at}: entry {i} byte {within} of {len(store.chunks[i])}")
    assert (timing["unique"], timing["decode"]["frames"]) == (uniq, frames), name
    covering = [s for s in want_status if s != NOT_REQUESTED]
    assert timing["entries"] == len(covering) and timing["failed"] == sum(s != OK for s in covering)
    assert timing["missing"] == covering.count(MISSING) and timing["out_bytes"] == length


def test_restore_whole_archive_decodes_every_repeat_once(gpu, torch_dev, cfg, store, store_dev):
    total = int(store.ends[-1])
    _, status, timing = restore(gpu, torch_dev, store, store_dev, cfg, 0, None, allow_bad=True)
    present = {x.tobytes() for x, s in zip(store.digests, store.status) if s != MISSING}
    assert timing["unique"] == len(present) == 16 < timing["entries"] == 40
    assert timing["decoded_bytes"] == sum(len(c) for c in {x.tobytes(): c for x, c, s in
                                                             zip(store.digests, store.chunks, store.status) if s != MISSING}.values())
    assert timing["out_bytes"] == total and {int(s) for s in status} == {OK, BAD_CRC, BAD_DIGEST, MISSING}


def test_restore_past_the_end_is_invalid(gpu, torch_dev, cfg, store, store_dev):
    total = int(store.ends[-1])
    out = torch_dev.full((64,), FILL, dtype=torch_dev.uint8, device="cuda")
    for offset, length in ((total, 1), (total - 10, 11), (total + 1, 0), (0, total + 1)):
        with pytest.raises(gpu.ChunkerError) as e:
            gpu.restore_range_device((store.ends, store.digests), store_dev.data_ptr() + 7, store.offsets,
                                     store.store_digests, out.data_ptr(), offset, length, crypt=cfg, allow_bad=True)
        assert e.value.code == INVALID
    torch_dev.cuda.synchronize()
    assert bool((out == FILL).all())


def test_restore_raises_for_a_failed_entry_unless_allowed(gpu, torch_dev, cfg, store, store_dev):
    py = [0] + [int(e) for e in store.ends]
    with pytest.raises(gpu.ChunkerError):
        restore(gpu, torch_dev, store, store_dev, cfg, py[9], py[12] - py[9])       # entry 10 is absent
    got, status, _ = restore(gpu, torch_dev, store, store_dev, cfg, py[0], py[10])   # entries 0..9 are good
    assert got == b"".join(store.chunks[:10]) and [int(s) for s in status[:10]] == [OK] * 10


def test_restore_without_a_config(gpu, torch_dev, store, store_dev):
    total = int(store.ends[-1])
    want_bytes, want_status, uniq, frames = expected(store, 0, total, no_config=True)
    assert NO_CONFIG in want_status and OK in want_status
    got, status, timing = restore(gpu, torch_dev, store, store_dev, None, 0, total, allow_bad=True)
    assert [int(s) for s in status] == want_status
    assert got == want_bytes
    assert (timing["unique"], timing["decode"]["frames"]) == (uniq, frames)


# ---- round trip through the device encoder ----------------------------------------------------

@pytest.mark.parametrize("encrypt", [0, 1])
def test_stream_round_trip(gpu, torch_dev, cfg, encrypt):
    host = r.roundtrip_stream()
    n = host.size
    dev = to_dev(torch_dev, host)
    with gpu.Chunker(64 * 1024) as c:
        c.set_stream(torch_dev.cuda.current_stream().cuda_stream)
        ends = c.find_cuts_device(dev.data_ptr(), n, is_final=True)
    assert int(ends[-1]) == n
    bounds = np.concatenate([[0], ends]).astype(np.uint64)
    crypt = cfg if encrypt else None
    digests = gpu.digest_chunks_device(dev.data_ptr(), n, bounds, key=cfg.id_key if encrypt else None)
    cap = gpu.blob_stream_bound_encrypted(bounds) if encrypt else gpu.blob_stream_bound(bounds)
    blobs = torch_dev.empty(cap, dtype=torch_dev.uint8, device="cuda")
    offs, _, comp, _ = gpu.blob_encode_chunks_device(dev.data_ptr(), n, bounds, blobs.data_ptr(), cap, compress=True,
                                                     crypt=crypt)
    assert comp.any()
    image, csum = gpu.didx_build(ends, digests, bytes(range(16)), 1_700_000_000)
    index = gpu.DynamicIndexReader(image)
    assert index.compute_csum() == (csum, n) and index.index_csum == csum
    out = torch_dev.full((n + 64,), FILL, dtype=torch_dev.uint8, device="cuda")
    torch_dev.cuda.synchronize()
    status, timings = gpu.restore_stream_device(index, blobs.data_ptr(), offs, digests, out.data_ptr(), crypt=crypt,
                                                window=r.ROUNDTRIP_WINDOW)
    torch_dev.cuda.synchronize()
    img = out.cpu().numpy()
    assert (status == OK).all() and (img[n:] == FILL).all()
    assert np.array_equal(img[:n], host)
    assert hashlib.sha256(img[:n].tobytes()).digest() == hashlib.sha256(host.tobytes()).digest()
    windows = r.stream_windows(ends, r.ROUNDTRIP_WINDOW)
    assert len(windows) == len(timings) > 1
    for (i, j), t in zip(windows, timings):
        assert (t["entries"], t["unique"]) == (j - i + 1, len({digests[k].tobytes() for k in range(i, j + 1)}))
        assert t["failed"] == 0 and t["out_bytes"] == int(bounds[j + 1] - bounds[i])
    assert sum(t["unique"] for t in timings) < sum(t["entries"] for t in timings) == ends.size
    gpu.blob_encode_release()
