"""Garbage collection on the host (include/pbs_gc.h, pbs_gc_*_host; no GPU): the host mirror
against the Python model of tests/gcplanted.py on every planted case, the argument rules, and
garbage_collection(..., device=False) on a real chunk store under tmp_path."""
import numpy as np
import pytest

import gcplanted as G

P1 = 1_700_000_000
TIMES = [(P1, P1), (P1, P1 - 200_000)]  # oldest_writer == phase1_start; oldest_writer < phase1_start - 86400
SIZES_M = [0, 1, 2, 31, 32, 33, 255, 256, 257, 4096, 4097, 70000]


def strided(rows, stride, lead=8):
    """The digests `stride` bytes apart in a poisoned buffer, the first one 8- but not 16-byte
    aligned.  Returns (buffer, address of digest 0)."""
    n = rows.shape[0]
    buf = np.full(lead + 16 + n * stride + 64, 0xEE, dtype=np.uint8)
    off = (-buf.ctypes.data) % 16 + 8
    view = np.lib.stride_tricks.as_strided(buf[off:], shape=(n, 32), strides=(stride, 1))
    view[:] = rows
    return buf, buf.ctypes.data + off


def check_against_model(p, files, index, phase1_start, oldest_writer, pieces=1, stride=32):
    listing = G.sim_listing(files)
    paths = listing[0]
    model = G.model_gc(files, [("a.didx", index, 12345)], phase1_start, oldest_writer, now=phase1_start + 7)
    rows = G.digest_rows(index) if index else np.zeros((0, 32), dtype=np.uint8)
    buf, addr = strided(rows, stride)
    before = buf.copy()
    with p.GarbageCollector(listing, device=False) as gc:
        n = rows.shape[0]
        cuts = [n * k // pieces for k in range(pieces + 1)]
        missing = []
        for k in range(pieces):
            pos, nm = gc.mark(addr + cuts[k] * stride, stride, cuts[k + 1] - cuts[k], index_bytes=12345 if k == 0 else None)
            assert nm == pos.size
            missing += [int(x) + cuts[k] for x in pos]
        assert np.array_equal(buf, before), "the index was written"
        assert missing == [pos for _, pos in model["warnings"]]
        touched = gc.touched()
        assert {paths[j] for j in np.flatnonzero(touched)} == model["touched"]
        sizes, atimes = G.sim_sizes_atimes(files, paths)
        actions, status = gc.sweep(sizes, atimes, phase1_start, oldest_writer)
        assert status == model["status"]
        assert {paths[j] for j in np.flatnonzero(actions == G.REMOVE)} == model["removed"]
        assert {paths[j] for j in np.flatnonzero(actions == G.PENDING)} == model["pending"]
        assert set(np.unique(actions)) <= {G.KEEP, G.PENDING, G.REMOVE}
    return model


@pytest.mark.parametrize("m", SIZES_M)
def test_mirror_equals_model(pbschunk, m):
    files, index = G.planted(m, seed=m + 1)
    for phase1_start, oldest_writer in TIMES:
        G.plant_times(files, index, phase1_start, oldest_writer)
        model = check_against_model(pbschunk, files, index, phase1_start, oldest_writer)
    if m >= 4096:  # every class holds bad and non-bad files, and the sums pass 2^32
        s = model["status"]
        for k in ("disk-chunks", "removed-chunks", "pending-chunks", "removed-bad", "still-bad"):
            assert s[k] > 0, k
        assert min(s["disk-bytes"], s["removed-bytes"], s["pending-bytes"]) > 1 << 40


@pytest.mark.parametrize("stride,pieces", [(40, 1), (48, 3), (32, 3)])
def test_mirror_strides_and_pieces(pbschunk, stride, pieces):
    files, index = G.planted(4097, seed=5)
    G.plant_times(files, index, *TIMES[1])
    check_against_model(pbschunk, files, index, *TIMES[1], pieces=pieces, stride=stride)


def test_home_slot_is_the_documented_formula(pbschunk):
    rng = np.random.default_rng(3)
    for L in (1, 6, 13, 18, 33, 63):
        for _ in range(50):
            d = rng.bytes(32)
            assert pbschunk.gc_home_slot(d, L) == G.home_slot(d, L)


def test_mirror_argument_rules(pbschunk):
    p = pbschunk
    files, index = G.planted(64, seed=9)
    listing = G.sim_listing(files)
    rows = G.digest_rows(index)
    buf, addr = strided(rows, 32)
    gc = p.GarbageCollector(listing, device=False)
    for bad_stride in (0, 24, 31, 36, 44):
        with pytest.raises(p.ChunkerError) as e:
            gc.mark(addr, bad_stride, 4, index_bytes=1)
        assert e.value.code == p.PBS_ERR_INVALID
    for shift in (1, 4):
        with pytest.raises(p.ChunkerError) as e:
            gc.mark(addr + shift, 32, 4, index_bytes=1)
        assert e.value.code == p.PBS_ERR_INVALID
    with pytest.raises(p.ChunkerError) as e:
        gc.sweep(np.zeros(64, np.uint64), np.zeros(64, np.int64), P1, P1 + 1)
    assert e.value.code == p.PBS_ERR_INVALID
    _, status = gc.sweep(np.zeros(64, np.uint64), np.zeros(64, np.int64), P1, P1)
    assert status["index-file-count"] == 0 and status["index-data-bytes"] == 0, "a rejected mark counted"
    assert not gc.touched().any()
    # cap: 0, n_missing - 1, n_missing
    _, nm = gc.mark(addr, 32, rows.shape[0], index_bytes=77, cap=0)
    assert nm > 2
    full, _ = gc.mark(addr, 32, rows.shape[0], cap=nm)
    part, nm2 = gc.mark(addr, 32, rows.shape[0], cap=nm - 1)
    assert nm2 == nm and full.size == nm and np.array_equal(part, full[:-1]) and np.all(np.diff(full.astype(np.int64)) > 0)
    _, status = gc.sweep(np.zeros(64, np.uint64), np.zeros(64, np.int64), P1, P1)
    assert status["index-file-count"] == 1 and status["index-data-bytes"] == 77
    with pytest.raises(p.ChunkerError):
        p.GarbageCollector((None, listing[1], np.full(64, 4, np.uint8)), device=False)
    gc.close()
    for call in (lambda: gc.mark(addr, 32, 1), lambda: gc.touched(), lambda: gc.mark_index(b"\0" * 4096),
                 lambda: gc.sweep(np.zeros(64, np.uint64), np.zeros(64, np.int64), P1, P1)):
        with pytest.raises(p.ChunkerError) as e:
            call()
        assert e.value.code == p.PBS_ERR_INVALID
    gc.close()  # (twice: nothing)


def test_mirror_index_images(pbschunk):
    p = pbschunk
    files, index = G.planted(700, seed=11)
    G.plant_times(files, index, *TIMES[0])
    listing = G.sim_listing(files)
    (didx, a, abytes), (fidx, b, bbytes) = G.index_images(p, index)
    model = G.model_gc(files, [("a.didx", a, abytes), ("b.fidx", b, bbytes)], *TIMES[0], now=P1)
    with p.GarbageCollector(listing, device=False) as gc:
        for bad in (didx[:4095], didx + b"\0", b"\1" + didx[1:], fidx[:-1], b"\1" + fidx[1:], fidx[:4096]):
            with pytest.raises(p.ChunkerError) as e:
                gc.mark_index(bad)
            assert e.value.code == p.PBS_ERR_INVALID
        assert not gc.touched().any(), "a bad image left marks"
        pa = gc.mark_index(didx)
        pb = gc.mark_index(fidx, cap=0)
        assert pb.size == 0
        assert [("a.didx", int(x)) for x in pa] == [w for w in model["warnings"] if w[0] == "a.didx"]
        assert gc.n_missing == sum(1 for w in model["warnings"] if w[0] == "b.fidx")
        sizes, atimes = G.sim_sizes_atimes(files, listing[0])
        _, status = gc.sweep(sizes, atimes, *TIMES[0])
        assert status == model["status"]


def test_garbage_collection_on_a_real_store_host(pbschunk, tmp_path):
    G.run_real_store(pbschunk, tmp_path, device=False)
