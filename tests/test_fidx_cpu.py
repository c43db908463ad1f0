"""The fixed index (.fidx) on the host: image, parser, position helpers, check_chunk_alignment,
FixedChunkStream, FixedIndexWriter / FixedIndexReader and the dirty map's host mirror
(include/pbs_fixed.h, proxmox-backup_amd/csrc/pbs_fidx.cpp).  No GPU."""
import hashlib
import struct

import numpy as np
import pytest

import fplanted as f

NOT_POW2, CAPACITY, INVALID = -1, -5, -6
UUID = bytes(range(1, 17))
CTIME = 1700000123
MIB4 = 4 << 20


def sizes():
    out = []
    for c in (1, 4096, MIB4):
        for k in (1, 2, 5):
            for size in (k * c, k * c + 1, k * c - 1):
                if size > 0:
                    out.append((size, c))
    return sorted(set(out))


@pytest.mark.parametrize("size,c", sizes())
def test_image_equals_the_layout_and_parses_back(pbschunk, size, c):
    n = f.count(size, c)
    dig = f.digests_of(n, size % 97)
    image, csum = pbschunk.fidx_build(dig, size, c, UUID, CTIME)
    want = f.model_image(dig, size, c, UUID, CTIME)
    assert image == want and len(image) == pbschunk.fidx_size(n) == 4096 + 32 * n
    assert csum == hashlib.sha256(dig.tobytes()).digest() == want[32:64]
    assert pbschunk.fidx_count(size, c) == n
    uuid, ctime, hc, cc, psize, pcs, pdig = pbschunk.fidx_parse(want)
    assert (uuid, ctime, hc, cc, psize, pcs) == (UUID, CTIME, csum, csum, size, c)
    assert np.array_equal(pdig, dig)
    # a flipped digest byte: the computed checksum moves, the header's stays; nothing is compared
    bad = bytearray(want)
    bad[4096 + 32 * (n - 1) + 5] ^= 1
    _, _, hc, cc, *_ = pbschunk.fidx_parse(bytes(bad))
    assert hc == csum and cc == hashlib.sha256(bytes(bad[4096:])).digest() != csum


def test_negative_ctime_round_trips(pbschunk):
    image, _ = pbschunk.fidx_build(f.digests_of(1), 10, 4096, UUID, -5)
    assert image[24:32] == struct.pack("<q", -5) and pbschunk.fidx_parse(image)[1] == -5


def parse_code(pbschunk, image, cap=None):
    with pytest.raises(pbschunk.ChunkerError) as e:
        pbschunk.fidx_parse(image, cap)
    return e.value.code, e.value.n


def test_parse_errors(pbschunk):
    size, c = 5 * 4096 + 1, 4096
    dig = f.digests_of(6)
    good = f.model_image(dig, size, c, UUID, CTIME)
    assert parse_code(pbschunk, good[:4095])[0] == INVALID                      # "index too small"
    assert parse_code(pbschunk, good[:4096] + bytes(31))[0] == INVALID         # a ragged body
    assert parse_code(pbschunk, bytes([good[0] ^ 1]) + good[1:])[0] == INVALID  # "got unknown magic number"
    assert parse_code(pbschunk, good[:7] + bytes([good[7] ^ 0x80]) + good[8:])[0] == INVALID
    assert parse_code(pbschunk, good + bytes(32))[0] == INVALID                 # one entry too many
    assert parse_code(pbschunk, good[:-32])[0] == INVALID                       # one too few
    zero_size = good[:64] + struct.pack("<Q", 0) + good[72:4096]
    assert parse_code(pbschunk, zero_size)[0] == INVALID                        # no zero-length mapping
    zero_cs = good[:72] + struct.pack("<Q", 0) + good[80:]
    assert parse_code(pbschunk, zero_cs)[0] == INVALID                          # the reference divides by it
    three = f.model_image(f.digests_of(f.count(size, 3)), size, 3, UUID, CTIME)
    assert parse_code(pbschunk, three)[0] == NOT_POW2                           # (the documented deviation)
    assert parse_code(pbschunk, good, cap=5) == (CAPACITY, 6)                   # under capacity still sets n
    assert parse_code(pbschunk, good, cap=0) == (CAPACITY, 6)


def test_position_helpers(pbschunk):
    c = 4096
    for size in (5 * c, 5 * c + 1, 5 * c - 1, 1):
        n = f.count(size, c)
        assert pbschunk.fidx_chunk_info(size, c, n - 1) == ((n - 1) * c, size)  # the last one is clipped
        assert pbschunk.fidx_chunk_info(size, c, n) is None
        if n > 1:
            assert pbschunk.fidx_chunk_info(size, c, 0) == (0, c) and pbschunk.fidx_chunk_info(size, c, 1) == (c, min(2 * c, size))
        for off in (0, c - 1, c, size - 1):
            want = None if off >= size else (off // c, off % c)
            assert pbschunk.fidx_chunk_from_offset(size, c, off) == want, (size, off)
        assert pbschunk.fidx_chunk_from_offset(size, c, size) is None          # :206-208
        assert pbschunk.fidx_chunk_from_offset(size, c, size + 1) is None
    with pytest.raises(pbschunk.ChunkerError) as e:
        pbschunk.fidx_chunk_from_offset(100, 3, 0)
    assert e.value.code == NOT_POW2


# (size, chunk_size, end offset, chunk_len) -> the index, or None where the reference bails
C = 4096
ALIGNMENT_CASES = [
    ((5 * C, C, 1, 2), None),                 # :365 offset < chunk_len: "got chunk with small offset"
    ((5 * C, C, 5 * C + 1, 1), None),         # :371 offset > size: "chunk data exceeds size"
    ((5 * C, C, 6 * C, C), None),             # :371 a whole chunk past the end
    ((5 * C, C, 2 * C - 1, C - 1), None),     # :376 short chunk that does not end the image
    ((5 * C + 9, C, 5 * C, C - 1), None),     # :376 ... nor one that ends the last full chunk
    ((5 * C, C, 5 * C, C + 1), None),         # :377 chunk_len > chunk_size, even at the end
    ((5 * C, C, 5 * C, 0), None),             # :378 chunk_len == 0 at the end
    ((5 * C, C, 2 * C, 0), None),             # :376 chunk_len == 0 elsewhere (!= chunk_size)
    ((5 * C, C, 2 * C + 1, C), None),         # :387 pos & (chunk_size - 1) != 0: "got unaligned chunk"
    ((5 * C, C, C, C), 0),                    # :391 the first chunk
    ((5 * C, C, 3 * C, C), 2),                # :391 a middle chunk
    ((5 * C, C, 5 * C, C), 4),                # :391 a full last chunk of an exact multiple
    ((5 * C + 9, C, 5 * C + 9, 9), 5),        # quirk 1: a short last chunk is legal with offset == size ...
    ((5 * C + 9, C, 5 * C + 8, 8), None),     # :376 ... and only then
    ((5 * C + 9, C, 5 * C + 9, C), None),     # quirk 2: a full-length "last" chunk of a ragged image passes
                                              # the length clause (:376-378) and fails :387 as unaligned
    ((5 * C + 9, C, 5 * C + 9, 10), None),    # :387 a short last chunk from the wrong start
    ((9, C, 9, 9), 0),                        # an image shorter than one chunk
]


@pytest.mark.parametrize("args,want", ALIGNMENT_CASES)
def test_check_chunk_alignment_clause_by_clause(pbschunk, args, want):
    model = f.model_chunk_alignment(*args)
    assert (model if isinstance(model, int) else None) == want, "the transcription disagrees with the written value"
    if want is None:
        with pytest.raises(pbschunk.ChunkerError) as e:
            pbschunk.fidx_check_chunk_alignment(*args)
        assert e.value.code == INVALID
    else:
        assert pbschunk.fidx_check_chunk_alignment(*args) == want


def test_quirk_two_fails_as_unaligned_not_as_length():
    assert f.model_chunk_alignment(5 * C + 9, C, 5 * C + 9, C) == "unaligned"


@pytest.mark.parametrize("c", (16, 4096))
def test_fixed_chunk_stream(pbschunk, c):
    for total in (0, 1, c - 1, c, c + 1, 3 * c, 3 * c + 5):
        data = np.random.default_rng([7, total]).integers(0, 256, total, dtype=np.uint8).tobytes()
        want = [data[i:i + c] for i in range(0, total, c)]
        assert all(want) and (total % c or all(len(x) == c for x in want))  # no empty last chunk
        for piece in (1, 7, c - 1, c, c + 1, max(total, 1)):
            if piece == 1 and total > 20000:
                continue
            s = pbschunk.FixedChunkStream(c)
            got = list(s.chunks(data[i:i + piece] for i in range(0, total, piece)))
            assert got == want, (total, piece)
    assert list(pbschunk.FixedChunkStream(c).chunks([])) == [] and pbschunk.FixedChunkStream(c).finish() == []


def test_writer_out_of_order_equals_in_order(pbschunk):
    c, size = 4096, 7 * 4096 + 33
    n = f.count(size, c)
    dig = f.digests_of(n, 3)
    ends = [min((i + 1) * c, size) for i in range(n)]
    want, want_csum = pbschunk.fidx_build(dig, size, c, UUID, CTIME)
    for order in (range(n), reversed(range(n)), np.random.default_rng(5).permutation(n)):
        w = pbschunk.FixedIndexWriter(size, c, UUID, CTIME)
        for i in order:
            i = int(i)
            assert w.add_chunk(ends[i], ends[i] - i * c, dig[i].tobytes()) == i
        assert w.close() == want_csum and w.image() == want
    assert want == f.model_image(dig, size, c, UUID, CTIME)


def test_writer_clone_and_patch(pbschunk, tmp_path):
    c, size = 4096, 6 * 4096
    dig = f.digests_of(6, 4)
    prev = pbschunk.FixedIndexReader(pbschunk.fidx_build(dig, size, c, UUID, CTIME)[0])
    w = pbschunk.FixedIndexWriter(size, c, bytes(16), 5)
    w.clone_data_from(prev)
    patched = dig.copy()
    patched[1], patched[4] = 0x11, 0x44
    w.add_digest(4, patched[4].tobytes())
    w.add_digest(1, patched[1].tobytes())
    path = tmp_path / "disk.img.fidx"
    csum = w.close(str(path))
    assert (w.image(), csum) == pbschunk.fidx_build(patched, size, c, bytes(16), 5)
    r = pbschunk.FixedIndexReader(str(path))
    assert (r.index_count(), r.index_bytes(), r.chunk_size, r.uuid, r.ctime) == (6, size, c, bytes(16), 5)
    assert r.index_csum == csum == r.compute_csum()[0] and r.compute_csum()[1] == size
    assert r.index_digest(4) == patched[4].tobytes() and r.index_digest(6) is None
    assert r.chunk_info(5) == (5 * c, size, patched[5].tobytes()) and r.chunk_info(6) is None
    assert r.chunk_from_offset(size - 1) == (5, c - 1) and r.chunk_from_offset(size) is None


def test_writer_errors(pbschunk):
    c = 4096
    prev = pbschunk.FixedIndexReader(pbschunk.fidx_build(f.digests_of(6), 6 * c, c)[0])
    w = pbschunk.FixedIndexWriter(5 * c, c, UUID, CTIME)
    with pytest.raises(ValueError):
        w.clone_data_from(prev)                        # "index sizes not equal"
    with pytest.raises(IndexError):
        w.add_digest(5, bytes(32))                     # "index out of range"
    with pytest.raises(pbschunk.ChunkerError):
        w.add_chunk(5 * c + 1, 1, bytes(32))
    w.close()
    with pytest.raises(RuntimeError):
        w.close()                                      # "cannot close already closed index file."
    with pytest.raises(RuntimeError):
        w.add_digest(0, bytes(32))
    with pytest.raises(pbschunk.ChunkerError):
        pbschunk.FixedIndexWriter(5 * c, 3, UUID, CTIME)


def test_dirty_mirror_equals_the_model(pbschunk):
    for label, prev, cur in f.planted_dirty_sets(4096):
        flags, n_dirty = pbschunk.fixed_dirty_host(prev, cur, 4096)
        want = f.model_dirty(prev, cur, 4096)
        assert np.array_equal(flags, want) and n_dirty == int(want.sum()), label
        if "/x" in label:
            assert n_dirty == 1, label
    # a chunk size that is no power of two is the mirror's business too
    a, b = f.image_pair(1000, 1)
    b[999] ^= 1
    flags, n_dirty = pbschunk.fixed_dirty_host(a, b, 300)
    assert flags.tolist() == [0, 0, 0, 1] and n_dirty == 1
