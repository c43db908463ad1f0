"""The fixed-size chunk path on the GPU (include/pbs_fixed.h): the dirty map kernel at the
positions where its tiling can go wrong, the digests of a resident image with a dirty map, the
upload of an image from host memory and the restore of a range."""
import hashlib

import numpy as np
import pytest

import dplanted as d
import fplanted as f
import gplanted as g

pytestmark = pytest.mark.gpu

NOT_POW2, INVALID = -1, -6
OK, BAD_SIZE, MISSING, NOT_REQUESTED = 0, 7, 10, 255
KiB, MiB = 1 << 10, 1 << 20
FILL = 0xA5
GUARD = 64
OFFSETS = ((0, 0), (1, 0), (0, 8), (3, 13))


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


# ---- the dirty map ------------------------------------------------------------------------------

class Pair:
    """Two images of `size` bytes at byte offsets (po, co) inside larger device buffers."""

    def __init__(self, torch, host: np.ndarray, po: int, co: int):
        self.torch, self.size, self.po, self.co = torch, host.size, po, co
        self.prev = torch.full((po + host.size + 32,), 0x3C, dtype=torch.uint8, device="cuda")
        self.cur = torch.full((co + host.size + 32,), 0xC3, dtype=torch.uint8, device="cuda")
        img = to_dev(torch, host)
        self.prev[po:po + host.size] = img
        self.cur[co:co + host.size] = img
        self.prev0, self.cur0 = self.prev.clone(), self.cur.clone()

    def run(self, gpu, c: int):
        """(flags, n_dirty); the flag buffer is filled and guarded."""
        torch = self.torch
        n = f.count(self.size, c)
        flags = torch.full((n + GUARD,), FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        cnt = gpu.fixed_dirty_device(self.prev.data_ptr() + self.po, self.cur.data_ptr() + self.co, self.size, c,
                                     flags.data_ptr())
        torch.cuda.synchronize()
        out = flags.cpu().numpy()
        assert (out[n:] == FILL).all(), "bytes after dirty_dev[0 .. n) were written"
        return out[:n], cnt


@pytest.mark.parametrize("r_name", ("0", "1", "15", "16", "17", "C-1"))
@pytest.mark.parametrize("c", (4 * KiB, 64 * KiB, 1 * MiB))
def test_dirty_one_flipped_byte(gpu, torch_dev, c, r_name):
    r = c - 1 if r_name == "C-1" else int(r_name)
    size = 5 * c + r
    host, _ = f.image_pair(size, r)
    flips = f.flip_positions(size, c)
    n = f.count(size, c)
    for po, co in OFFSETS:
        pair = Pair(torch_dev, host, po, co)
        flags, cnt = pair.run(gpu, c)
        assert cnt == 0 and not flags.any(), "equal images"
        cur_host = host.copy()
        for label, at in flips.items():
            for bit in (0x01, 0x80):
                pair.cur[co + at] ^= bit
                cur_host[at] ^= bit
                flags, cnt = pair.run(gpu, c)
                want, want_cnt = gpu.fixed_dirty_host(host, cur_host, c)
                pair.cur[co + at] ^= bit
                cur_host[at] ^= bit
                where = f"C {c} r {r} offsets ({po}, {co}) {label} byte {at} ^ {bit:#x}"
                assert np.array_equal(flags, want) and cnt == want_cnt == 1, (where, flags.tolist())
                assert flags[at // c] == 1 and int(flags.sum()) == 1 and flags.size == n, where
        assert torch_dev.equal(pair.prev, pair.prev0) and torch_dev.equal(pair.cur, pair.cur0), "an image was written"


@pytest.mark.parametrize("c", (4 * KiB, 64 * KiB, 1 * MiB))
def test_dirty_all_different_and_mixed(gpu, torch_dev, c):
    size = 5 * c + 17
    host, _ = f.image_pair(size, 5)
    for po, co in OFFSETS:
        pair = Pair(torch_dev, host, po, co)
        pair.cur[co:co + size] ^= 0xFF
        flags, cnt = pair.run(gpu, c)
        assert flags.tolist() == [1] * 6 and cnt == 6
        # every byte of chunks 1 and 4 and the last chunk's last byte
        pair.cur[co:co + size] = pair.prev[po:po + size]
        cur_host = host.copy()
        for lo, hi in ((c, 2 * c), (4 * c, 5 * c), (size - 1, size)):
            pair.cur[co + lo:co + hi] ^= 0x10
            cur_host[lo:hi] ^= 0x10
        flags, cnt = pair.run(gpu, c)
        want, want_cnt = gpu.fixed_dirty_host(host, cur_host, c)
        assert flags.tolist() == want.tolist() == [0, 1, 0, 0, 1, 1] and cnt == want_cnt == 3
        assert torch_dev.equal(pair.prev, pair.prev0), "the previous image was written"


def test_dirty_many_chunks_counts_on_the_device(gpu, torch_dev):
    c, n = 4 * KiB, 3001  # more flags than one counting workgroup holds
    host, _ = f.image_pair(n * c - 5, 8)
    pair = Pair(torch_dev, host, 5, 2)
    cur_host = host.copy()
    for i in range(0, n, 7):
        at = i * c + (i * 37) % (c - 5)
        pair.cur[2 + at] ^= 0x04
        cur_host[at] ^= 0x04
    flags, cnt = pair.run(gpu, c)
    want, want_cnt = gpu.fixed_dirty_host(host, cur_host, c)
    assert np.array_equal(flags, want) and cnt == want_cnt == len(range(0, n, 7))


def test_dirty_chunk_size_errors(gpu, torch_dev):
    a = torch_dev.zeros(1 << 16, dtype=torch_dev.uint8, device="cuda")
    fl = torch_dev.full((64,), FILL, dtype=torch_dev.uint8, device="cuda")
    for c, code in ((2048, INVALID), (12288, NOT_POW2), (0, NOT_POW2)):
        with pytest.raises(gpu.ChunkerError) as e:
            gpu.fixed_dirty_device(a.data_ptr(), a.data_ptr(), 1 << 16, c, fl.data_ptr())
        assert e.value.code == code, c
    torch_dev.cuda.synchronize()
    assert (fl.cpu().numpy() == FILL).all()


# ---- digests of a resident image ---------------------------------------------------------------

def ref_digests(data: np.ndarray, c: int, key=None) -> np.ndarray:
    k = bytes(key) if key else b""
    out = [hashlib.sha256(data[s:s + c].tobytes() + k).digest() for s in range(0, data.size, c)]
    return np.frombuffer(b"".join(out), np.uint8).reshape(-1, 32)


@pytest.mark.parametrize("keyed", (False, True))
@pytest.mark.parametrize("tail", ("5C+1", "3C"))
@pytest.mark.parametrize("c", (4 * KiB, 64 * KiB, 1 * MiB))
def test_fixed_digests(gpu, torch_dev, c, tail, keyed):
    """(1 MiB beside the sizes the issue names: from there the chunks go through the hybrid split.)"""
    size = 5 * c + 1 if tail == "5C+1" else 3 * c
    key = bytes(range(100, 132)) if keyed else None
    data = np.random.default_rng([0x646967, c, size]).integers(0, 256, size, dtype=np.uint8)
    buf = torch_dev.zeros(size + 3, dtype=torch_dev.uint8, device="cuda")
    buf[3:] = to_dev(torch_dev, data)  # (an odd base address)
    ptr = buf.data_ptr() + 3
    want = ref_digests(data, c, key)
    n = want.shape[0]
    dig, csum, t = gpu.fixed_digests_device(ptr, size, c, key=key)
    assert np.array_equal(dig, want) and csum == hashlib.sha256(want.tobytes()).digest()
    assert (t["hashed_chunks"], t["hashed_bytes"]) == (n, size)
    # a dirty map with previous digests that are no digests of anything: the clean entries come
    # back verbatim -- they were not hashed
    prev = f.digests_of(n, 77)
    for dirty in ([1, 0] * 3, [0, 0, 1, 1, 0, 1], [0] * 6, [1] * 6):
        dirty = np.array(dirty[:n], dtype=np.uint8)
        dig, csum, t = gpu.fixed_digests_device(ptr, size, c, key=key, dirty=dirty, prev_digests=prev)
        exp = np.where(dirty[:, None] != 0, want, prev)
        assert np.array_equal(dig, exp), dirty.tolist()
        assert csum == hashlib.sha256(exp.tobytes()).digest()
        assert t["hashed_chunks"] == int(dirty.sum())
        assert t["hashed_bytes"] == sum(min(c, size - i * c) for i in np.flatnonzero(dirty))
    with pytest.raises(gpu.ChunkerError) as e:
        gpu.fixed_digests_device(ptr, size, c, dirty=np.ones(n, np.uint8))
    assert e.value.code == INVALID
    assert np.array_equal(buf[3:].cpu().numpy(), data), "the image was written"


def test_fixed_digests_chunk_size_errors(gpu, torch_dev):
    a = torch_dev.zeros(1 << 16, dtype=torch_dev.uint8, device="cuda")
    for c, code in ((2048, INVALID), (12288, NOT_POW2)):
        with pytest.raises(gpu.ChunkerError) as e:
            gpu.fixed_digests_device(a.data_ptr(), 1 << 16, c)
        assert e.value.code == code


# ---- upload ------------------------------------------------------------------------------------

UC = 64 * KiB
ULEN = 5 * UC + UC // 2


@pytest.fixture(scope="module")
def image():
    """Six chunks: text, text (= chunk 3), zeros, the same text as chunk 1, text, half a chunk of text."""
    import corpus_gen

    t = corpus_gen.text(5 * UC, 21)  # (about n bytes)
    assert t.size >= 4 * UC
    parts = [t[:UC], t[UC:2 * UC], np.zeros(UC, np.uint8), t[UC:2 * UC], t[2 * UC:3 * UC], t[3 * UC:3 * UC + UC // 2]]
    data = np.ascontiguousarray(np.concatenate(parts))
    assert data.size == ULEN
    return data


def known_model(digests, known, dirty=None):
    """backup_writer.rs:690-697: known iff in the previous index's set or an earlier (hashed) chunk."""
    seen = {bytes(k) for k in known}
    out = []
    for i, dg in enumerate(digests):
        if dirty is not None and not dirty[i]:
            out.append(1)
            continue
        out.append(1 if bytes(dg) in seen else 0)
        seen.add(bytes(dg))
    return np.array(out, dtype=np.uint8)


def check_upload(gpu, out, data, want_dig, want_known, key, crypt, compress, hashed=None):
    n = want_dig.shape[0]
    ends = np.minimum((np.arange(n, dtype=np.uint64) + 1) * np.uint64(UC), np.uint64(data.size))
    assert np.array_equal(out["ends"], ends), "ends is the grid"
    assert np.array_equal(out["digests"], want_dig)
    assert np.array_equal(out["known"], want_known)
    assert out["csum"] == hashlib.sha256(want_dig.tobytes()).digest()
    assert out["fidx"] == f.model_image(want_dig, data.size, UC, bytes(16), 0)
    offs = out["blob_offsets"]
    assert offs[0] == 0 and offs.size == n + 1
    total = 0
    for i in range(n):
        blob = out["blobs"][int(offs[i]):int(offs[i + 1])].tobytes()
        if want_known[i]:
            assert blob == b"" and not out["compressed"][i], f"known chunk {i} has a blob"
            continue
        chunk = data[i * UC:min((i + 1) * UC, data.size)].tobytes()
        payload, kind, status = gpu.blob_decode_host(blob, crypt=crypt)
        assert status == OK and (kind >= 2) == (crypt is not None), (i, kind, status)
        assert bool(out["compressed"][i]) == (kind in (1, 3)) and (compress or kind in (0, 2))
        if kind in (1, 3):
            payload, zst = gpu.zstd_inflate_host(payload, len(chunk))
            assert zst == 0
        assert payload == chunk, f"chunk {i} does not decode to itself"
        assert hashlib.sha256(payload + (key or b"")).digest() == want_dig[i].tobytes()
        total += len(blob)
    if compress and not want_known.all():
        assert any(out["compressed"][i] for i in range(n) if not want_known[i]), "text and zeros compress"
    st = out["stats"]
    sizes = [min(UC, data.size - i * UC) for i in range(n)]
    assert (st["chunk_count"], st["chunk_reused"], st["size"]) == (n, int(want_known.sum()), data.size)
    assert st["size_reused"] == sum(s for s, k in zip(sizes, want_known) if k)
    assert st["size_compressed"] == total == int(offs[-1])
    assert out["timing"]["dirty_chunks"] == (n if hashed is None else hashed)


@pytest.mark.parametrize("encrypt", (False, True))
@pytest.mark.parametrize("with_known", (False, True))
@pytest.mark.parametrize("compress", (True, False))
@pytest.mark.parametrize("piece", (UC, 3 * UC // 2, 1 << 30))
def test_upload_fixed(gpu, torch_dev, cfg, image, piece, compress, with_known, encrypt):
    crypt = cfg if encrypt else None
    key = cfg.id_key if encrypt else None
    want = ref_digests(image, UC, key)
    assert want[1].tobytes() == want[3].tobytes()
    known = [want[4].tobytes(), bytes(range(32))] if with_known else []
    out = gpu.upload_fixed_host(image, UC, known=known, piece=piece, compress=compress, crypt=crypt)
    want_known = known_model(want, known)
    assert want_known.tolist() == [0, 0, 0, 1, 1 if with_known else 0, 0]
    check_upload(gpu, out, image, want, want_known, key, crypt, compress)
    assert out["timing"]["copied_bytes"] == ULEN


@pytest.mark.parametrize("encrypt", (False, True))
@pytest.mark.parametrize("piece", (UC, 3 * UC // 2, 1 << 30))
def test_upload_fixed_with_a_dirty_map(gpu, torch_dev, cfg, image, piece, encrypt):
    """The clean chunks' host bytes are NOT what prev_digests describe (those are no digests of
    anything): a clean chunk that was read or hashed would show."""
    crypt = cfg if encrypt else None
    key = cfg.id_key if encrypt else None
    real = ref_digests(image, UC, key)
    n = real.shape[0]
    prev = f.digests_of(n, 31)
    pieces = [(s, min(s + piece, ULEN)) for s in range(0, ULEN, piece)]
    for dirty in ([0, 1, 0, 1, 0, 1], [0] * 6, [0, 0, 1, 0, 0, 0], [1] * 6, [0, 0, 0, 0, 0, 1]):
        dirty = np.array(dirty, dtype=np.uint8)
        want = np.where(dirty[:, None] != 0, real, prev)
        # chunk 3 holds chunk 1's bytes: it is known only when chunk 1 was hashed before it, never
        # through chunk 1's previous digest; `known` lists one previous and one real digest
        for known in ([], [prev[0].tobytes(), real[5].tobytes()]):
            out = gpu.upload_fixed_host(image, UC, known=known, piece=piece, dirty=dirty, prev_digests=prev, crypt=crypt)
            want_known = known_model(want, known, dirty)
            check_upload(gpu, out, image, want, want_known, key, crypt, True, hashed=int(dirty.sum()))
            touched = sum(hi - lo for lo, hi in pieces
                          if any(dirty[i] for i in range(n) if i * UC < hi and min((i + 1) * UC, ULEN) > lo))
            assert out["timing"]["copied_bytes"] == touched, (dirty.tolist(), piece)
    if piece == UC:
        assert touched == UC // 2  # the last run: one dirty chunk, one piece


def test_upload_fixed_after_the_pipeline(gpu, torch_dev, image, monkeypatch):
    """PBS_UPLOAD_SPEC=0: the known test and the encoding after the pipeline, with and without a map."""
    monkeypatch.setenv("PBS_UPLOAD_SPEC", "0")
    real = ref_digests(image, UC)
    out = gpu.upload_fixed_host(image, UC, piece=UC)
    check_upload(gpu, out, image, real, known_model(real, []), None, None, True)
    prev = f.digests_of(6, 32)
    dirty = np.array([0, 1, 0, 1, 1, 0], dtype=np.uint8)
    want = np.where(dirty[:, None] != 0, real, prev)
    out = gpu.upload_fixed_host(image, UC, piece=UC, dirty=dirty, prev_digests=prev)
    check_upload(gpu, out, image, want, known_model(want, [], dirty), None, None, True, hashed=3)


def test_upload_fixed_errors(gpu, image):
    for c, code in ((3 * UC, NOT_POW2), (0, NOT_POW2), (2048, INVALID)):
        with pytest.raises(gpu.ChunkerError) as e:
            gpu.upload_fixed_host(image, c)
        assert e.value.code == code, c
    with pytest.raises(gpu.ChunkerError) as e:
        gpu.upload_fixed_host(image, UC, dirty=np.ones(6, np.uint8))
    assert e.value.code == INVALID
    out = gpu.upload_fixed_host(b"", UC)
    assert out["ends"].size == 0 and out["stats"]["chunk_count"] == 0


def test_upload_stream_host_is_unchanged(gpu, oracle, image):
    """The dynamic twin on the same buffer: one call against the oracle's cuts."""
    avg = 64 * KiB
    ref_ends = oracle.chunk_feed(avg, image)
    if ref_ends.size == 0 or int(ref_ends[-1]) != image.size:
        ref_ends = np.append(ref_ends, np.uint64(image.size))
    bounds = np.concatenate([[0], ref_ends]).astype(np.uint64)
    ref_dig = oracle.chunk_digests(image, bounds)
    out = gpu.upload_stream_host(image, avg, piece=UC)
    assert np.array_equal(out["ends"], ref_ends) and np.array_equal(out["digests"], ref_dig)
    assert np.array_equal(out["known"], oracle.known_chunks(ref_dig, []))
    img, csum = oracle.didx_image(ref_ends, ref_dig, bytes(16), 0)
    assert out["didx"] == img and out["csum"] == csum


# ---- restore -----------------------------------------------------------------------------------

RC = 64 * KiB
RSIZE = 5 * RC + 1


@pytest.fixture(scope="module")
def archive(oracle):
    """Six entries over four blob kinds: entry 3 names entry 1's digest again, entry 2's blob is
    missing, and the last entry's blob holds RC bytes instead of 1."""
    import corpus_gen

    rng = np.random.default_rng(0x66727374)
    text = corpus_gen.text(3 * RC, 5)  # (about n bytes: more than the two chunks taken)
    chunks = [rng.integers(0, 256, RC, dtype=np.uint8).tobytes(), text[:RC].tobytes(),
              rng.integers(0, 256, RC, dtype=np.uint8).tobytes(), None, text[RC:2 * RC].tobytes(), b"\x5a"]
    chunks[3] = chunks[1]
    kinds = [2, 1, 0, 1, 3, 0]
    assert [len(c) for c in chunks] == [RC] * 5 + [1]
    digest = [d.keyed_digest(c, g.KEY1) if k >= 2 else d.plain_digest(c) for c, k in zip(chunks, kinds)]
    # the last entry names a chunk of RC bytes, which the store holds: its digest verifies, its
    # length is not the clipped one
    long_last = rng.integers(0, 256, RC, dtype=np.uint8).tobytes()
    digest[5] = d.plain_digest(long_last)
    blobs = {0: d.make_blob(oracle, 2, chunks[0], g.KEY1, g._iv(1)), 1: d.make_blob(oracle, 1, chunks[1], g.KEY1, g._iv(2)),
             4: d.make_blob(oracle, 3, chunks[4], g.KEY1, g._iv(4)),
             5: d.make_blob(oracle, 0, long_last, g.KEY1, g._iv(5))}
    extra = d.make_blob(oracle, 0, chunks[2], g.KEY1, g._iv(3))        # entry 2's blob, filed under another digest
    filed = [(digest[5], blobs[5]), (digest[1], blobs[1]), (hashlib.sha256(b"elsewhere").digest(), extra),
             (digest[4], blobs[4]), (digest[0], blobs[0])]
    assert {d.kind_of(b) for _, b in filed} == {0, 1, 2, 3}
    status = [OK, OK, MISSING, OK, OK, BAD_SIZE]
    return {"chunks": chunks, "digests": np.frombuffer(b"".join(digest), np.uint8).reshape(-1, 32), "status": status,
            "blobs": np.frombuffer(b"".join(b for _, b in filed), np.uint8),
            "offsets": np.concatenate([[0], np.cumsum([len(b) for _, b in filed])]).astype(np.uint64),
            "store_digests": np.frombuffer(b"".join(dg for dg, _ in filed), np.uint8).reshape(-1, 32)}


@pytest.mark.parametrize("name,offset,length", [("whole", 0, RSIZE), ("two-boundaries", RC - 100, RC + 200),
                                                ("last-byte", RSIZE - 1, 1), ("good-part", 3 * RC + 5, 2 * RC - 5)])
def test_restore_fixed_range(gpu, torch_dev, cfg, archive, name, offset, length):
    """Outputs and statuses against the dynamic call with the explicit ends and against the Python
    concatenation.  The last entry's store blob decodes to RC bytes and its digest verifies: the
    entry is 1 byte long, so it is BAD_SIZE (the restore looks at such a blob a second time in a
    slot of the longest chunk's length), with zeros for its byte."""
    torch = torch_dev
    store = torch.full((archive["blobs"].size + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    store[7:7 + archive["blobs"].size] = to_dev(torch, archive["blobs"])
    before = store.clone()
    image = gpu.fidx_build(archive["digests"], RSIZE, RC, bytes(range(16)), 9)[0]
    reader = gpu.FixedIndexReader(image)
    assert reader.index_count() == 6 and image[:8] == f.FIDX_MAGIC

    def call(fn, index):
        out = torch.full((3 + length + 256,), FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        status, timing = fn(index, store.data_ptr() + 7, archive["offsets"], archive["store_digests"], out.data_ptr() + 3,
                            offset, length, crypt=cfg, allow_bad=True)
        torch.cuda.synchronize()
        img = out.cpu().numpy()
        assert (img[:3] == FILL).all() and (img[3 + length:] == FILL).all(), "bytes outside out_dev[0 .. len) were written"
        return img[3:3 + length].tobytes(), [int(s) for s in status], timing

    got, status, timing = call(gpu.restore_fixed_range_device, reader)
    # the Python concatenation, zeros where the status is not OK
    sizes = [min(RC, RSIZE - i * RC) for i in range(6)]
    flat = b"".join(c if s == OK else bytes(n) for c, s, n in zip(archive["chunks"], archive["status"], sizes))
    i0, i1 = offset // RC, (offset + length - 1) // RC
    want_status = [archive["status"][i] if i0 <= i <= i1 else NOT_REQUESTED for i in range(6)]
    print(f"{name}: status {status}, wanted {want_status}")
    assert status == want_status, name
    assert got == flat[offset:offset + length], name
    # the dynamic call with the explicit ends
    got2, status2, timing2 = call(gpu.restore_range_device, (reader.ends(), reader.digests))
    assert (got2, status2) == (got, status), name
    for k in ("entries", "unique", "missing", "failed", "out_bytes"):
        assert timing[k] == timing2[k], k
    assert timing["failed"] == sum(s not in (OK, NOT_REQUESTED) for s in want_status)
    assert torch.equal(store, before), "the store was written"
    if name == "good-part":
        st, _ = gpu.restore_fixed_range_device(reader, store.data_ptr() + 7, archive["offsets"], archive["store_digests"],
                                               torch.empty(length, dtype=torch.uint8, device="cuda").data_ptr(), offset,
                                               length, crypt=cfg)
        assert [int(s) for s in st] == want_status


def test_restore_fixed_errors(gpu, torch_dev, cfg, archive):
    torch = torch_dev
    store = to_dev(torch, archive["blobs"])
    out = torch.empty(RSIZE + 16, dtype=torch.uint8, device="cuda")
    args = (store.data_ptr(), archive["offsets"], archive["store_digests"], out.data_ptr())
    for index, offset, length, code in (((archive["digests"], RSIZE, RC), 0, RSIZE + 1, INVALID),   # past the end
                                        ((archive["digests"], RSIZE, RC), RSIZE, 1, INVALID),
                                        ((archive["digests"][:5], RSIZE, RC), 0, 1, INVALID),        # a wrong count
                                        ((archive["digests"], RSIZE, 3 * RC), 0, 1, NOT_POW2),
                                        ((archive["digests"], RSIZE, 2048), 0, 1, INVALID)):
        with pytest.raises(gpu.ChunkerError) as e:
            gpu.restore_fixed_range_device(index, *args, offset, length, crypt=cfg, allow_bad=True)
        assert e.value.code == code, (offset, length)


@pytest.mark.parametrize("kind", (0, 1, 2, 3))
def test_restore_over_long_chunk_is_bad_size_only_when_its_digest_verifies(gpu, oracle, torch_dev, cfg, kind):
    """A dynamic index of two entries (RC and 10 bytes).  The second entry's store blob decodes to
    RC bytes: BAD_SIZE where it is the chunk the index names (read_chunk verifies the whole chunk,
    CachedChunk::new then refuses its length), BAD_DIGEST where it is filed under another digest."""
    import corpus_gen

    torch = torch_dev
    first = np.random.default_rng(41).integers(0, 256, RC, dtype=np.uint8).tobytes()
    long_chunk = corpus_gen.text(2 * RC, 42)[:RC].tobytes()
    assert len(long_chunk) == RC
    dg = (lambda c: d.keyed_digest(c, g.KEY1)) if kind >= 2 else d.plain_digest
    blobs = [d.make_blob(oracle, 0, first, g.KEY1, g._iv(1)), d.make_blob(oracle, kind, long_chunk, g.KEY1, g._iv(2))]
    assert d.kind_of(blobs[1]) == kind
    store = to_dev(torch, np.frombuffer(b"".join(blobs), np.uint8))
    offsets = np.array([0, len(blobs[0]), len(blobs[0]) + len(blobs[1])], dtype=np.uint64)
    ends = np.array([RC, RC + 10], dtype=np.uint64)
    other = hashlib.sha256(b"another chunk").digest()
    for named, want in ((dg(long_chunk), BAD_SIZE), (other, 6)):
        digests = np.frombuffer(d.plain_digest(first) + named, np.uint8).reshape(-1, 32)
        out = torch.full((RC + 10 + 16,), FILL, dtype=torch.uint8, device="cuda")
        status, timing = gpu.restore_range_device((ends, digests), store.data_ptr(), offsets, digests, out.data_ptr(),
                                                  crypt=cfg, allow_bad=True)
        torch.cuda.synchronize()
        img = out.cpu().numpy()
        assert [int(s) for s in status] == [OK, want]
        assert img[:RC].tobytes() == first and not img[RC:RC + 10].any() and (img[RC + 10:] == FILL).all()
        assert timing["failed"] == 1
