"""Garbage collection on the GPU (include/pbs_gc.h): the device must equal the host mirror exactly
on touched, actions, status, n_missing and the missing lists, on the planted stores of
tests/gcplanted.py (the mirror itself is checked against the model in test_gc_cpu.py)."""
import functools

import numpy as np
import pytest

import gcplanted as G

pytestmark = pytest.mark.gpu

P1 = 1_700_000_000
TIMES = [(P1, P1), (P1, P1 - 200_000)]  # oldest_writer == phase1_start; oldest_writer < phase1_start - 86400
POISON = 0xEE


@pytest.fixture(scope="module")
def torch_dev(gpu):
    import torch

    torch.cuda.set_device(0)
    yield torch
    gpu.gc_release()


@functools.lru_cache(maxsize=None)
def case(m):
    """(listing, index rows, sizes/atimes per TIMES entry) of the planted store of m files."""
    files, index = G.planted(m, seed=m + 1)
    listing = G.sim_listing(files)
    plans = []
    for phase1_start, oldest_writer in TIMES:
        G.plant_times(files, index, phase1_start, oldest_writer)
        plans.append(G.sim_sizes_atimes(files, listing[0]))
    rows = G.digest_rows(index) if index else np.zeros((0, 32), np.uint8)
    return listing, rows, plans


@functools.lru_cache(maxsize=None)
def long_index():
    """70 000 entries over the store of 4097 files: its planted index repeated, and from entry
    10 000 on one present digest 5 000 times."""
    _, rows, _ = case(4097)
    reps = -(-70000 // rows.shape[0])
    out = np.tile(rows, (reps, 1))[:70000].copy()
    out[10000:15000] = rows[0]
    return out


def host_strided(rows, stride):
    n = rows.shape[0]
    buf = np.full(16 + 8 + n * stride + 64, POISON, dtype=np.uint8)
    off = (-buf.ctypes.data) % 16 + 8
    np.lib.stride_tricks.as_strided(buf[off:], shape=(n, 32), strides=(stride, 1))[:] = rows
    return buf, buf.ctypes.data + off


def dev_strided(torch, rows, stride):
    """The digests `stride` bytes apart in a poisoned device buffer, digest 0 at an address that is
    8- but not 16-byte aligned.  Returns (tensor, its host image, address of digest 0)."""
    n = rows.shape[0]
    img = np.full(8 + n * stride + 64, POISON, dtype=np.uint8)
    np.lib.stride_tricks.as_strided(img[8:], shape=(n, 32), strides=(stride, 1))[:] = rows
    t = torch.from_numpy(img.copy()).cuda()
    assert t.data_ptr() % 16 == 0
    return t, img, t.data_ptr() + 8


def mark_all(gc, addr, stride, n, pieces=1, cap=None):
    cuts = [n * k // pieces for k in range(pieces + 1)]
    missing, total = [], 0
    for k in range(pieces):
        pos, nm = gc.mark(addr + cuts[k] * stride, stride, cuts[k + 1] - cuts[k],
                          index_bytes=4242 if k == 0 else None, cap=cap)
        missing += [int(x) + cuts[k] for x in pos]
        total += nm
    return missing, total


def outcome(gc, plans):
    """touched, and actions + status of one sweep per TIMES entry, on the same handle."""
    out = [gc.touched()]
    for (sizes, atimes), (phase1_start, oldest_writer) in zip(plans, TIMES):
        out += list(gc.sweep(sizes, atimes, phase1_start, oldest_writer))
    return out


def same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if isinstance(x, np.ndarray):
            assert np.array_equal(x, y)
        else:
            assert x == y


def compare(p, torch, listing, rows, plans, stride=32, pieces=1):
    t, img, addr = dev_strided(torch, rows, stride)
    hbuf, haddr = host_strided(rows, stride)
    n = rows.shape[0]
    with p.GarbageCollector(listing, device=True) as dev, p.GarbageCollector(listing, device=False) as host:
        assert dev.table_log2 == G.table_log2(len(listing[0]))
        got, want = mark_all(dev, addr, stride, n, pieces), mark_all(host, haddr, stride, n, pieces)
        assert got[1] == want[1] and got[0] == want[0]
        assert got[0] == sorted(got[0])
        torch.cuda.synchronize()
        assert np.array_equal(t.cpu().numpy(), img), "the index was written"
        same(outcome(dev, plans), outcome(host, plans))
        return want


@pytest.mark.parametrize("m", [0, 1, 2, 31, 32, 33, 255, 256, 257, 4096, 4097, 70000])
def test_table_of_every_size(gpu, torch_dev, m):
    listing, rows, plans = case(m)
    assert len(listing[0]) == m
    missing, nm = compare(gpu, torch_dev, listing, rows, plans)
    assert nm >= 2
    if m >= 4096:  # the planted groups are all there
        L = G.table_log2(m)
        d = listing[1]
        homes = [G.home_slot(bytes(x), L) for x in d]
        assert sum(h >= (1 << L) - 4 for h in homes) >= 8, "no cluster wraps"
        _, counts = np.unique(d[:, :8], axis=0, return_counts=True)
        assert counts.max() >= 300
        assert (listing[2] == 1).sum() > 12 and (listing[2] == 2).sum() >= 1 and (listing[2] == 3).sum() >= 1
        # the documented hash is the exported one
        for x, h in list(zip(d, homes))[:64]:
            assert gpu.gc_home_slot(bytes(x), L) == h


@pytest.mark.parametrize("n,stride", [(0, 32), (1, 40), (63, 40), (64, 48), (65, 32), (255, 40), (256, 40), (257, 48),
                                      (70000, 32), (70000, 40), (70000, 48)])
def test_mark_of_every_length_and_stride(gpu, torch_dev, n, stride):
    listing, _, plans = case(4097)
    compare(gpu, torch_dev, listing, long_index()[:n], plans, stride=stride)


def test_mark_in_three_pieces_equals_one_call(gpu, torch_dev):
    listing, _, plans = case(4097)
    rows = long_index()[:20001]
    one = compare(gpu, torch_dev, listing, rows, plans, stride=40, pieces=1)
    three = compare(gpu, torch_dev, listing, rows, plans, stride=40, pieces=3)
    assert one == three
    t, _, addr = dev_strided(torch_dev, rows, 40)
    with gpu.GarbageCollector(listing) as a, gpu.GarbageCollector(listing) as b:
        mark_all(a, addr, 40, rows.shape[0], pieces=1)
        mark_all(b, addr, 40, rows.shape[0], pieces=3)
        same(outcome(a, plans), outcome(b, plans))  # (the status holds the file and byte counters)
        assert a.sweep(*plans[0], *TIMES[0])[1]["index-file-count"] == 1


def test_missing_list_capacities(gpu, torch_dev):
    listing, _, _ = case(4097)
    rows = long_index()
    t, _, addr = dev_strided(torch_dev, rows, 40)
    with gpu.GarbageCollector(listing) as gc:
        full, nm = gc.mark(addr, 40, 70000)
        assert nm == full.size > 1000 and np.all(np.diff(full.astype(np.int64)) > 0)
        assert len({int(x) // 256 for x in full}) > 100, "the list does not cross blocks"
        for cap in (0, nm - 1, nm):
            pos, nm2 = gc.mark(addr, 40, 70000, cap=cap)
            assert nm2 == nm and np.array_equal(pos, full[:cap])


def test_index_images(gpu, torch_dev):
    p = gpu
    listing, rows, plans = case(4097)
    index = [bytes(r) for r in rows]
    (didx, _, _), (fidx, _, _) = G.index_images(p, index)
    with p.GarbageCollector(listing, device=True) as dev, p.GarbageCollector(listing, device=False) as host:
        for bad in (didx[:4095], didx + b"\0", b"\1" + didx[1:], fidx[:-1], b"\1" + fidx[1:], fidx[:4096]):
            with pytest.raises(p.ChunkerError) as e:
                dev.mark_index(bad)
            assert e.value.code == p.PBS_ERR_INVALID
        assert not dev.touched().any(), "a bad image left marks"
        assert dev.sweep(*plans[0], *TIMES[0])[1]["index-file-count"] == 0
        for img in (didx, fidx):
            got, want = dev.mark_index(img), host.mark_index(img)
            assert np.array_equal(got, want) and dev.n_missing == host.n_missing > 0
        same(outcome(dev, plans), outcome(host, plans))


def named(k, fill=0x11):
    return bytes([0xAB, k]) + bytes([fill]) * 30


def test_bad_rule(gpu, torch_dev):
    """Store entries by hand; `touched` spelled out."""
    store = [(named(1), 0), (named(1), G.BAD), (named(1), G.BAD),         # referenced, chunk present
             *[(named(2), G.BAD)] * 10,                                      # referenced, no chunk
             (named(3), G.BAD),                                              # not referenced
             (named(4), G.FOREIGN), (named(4), G.BAD),                       # referenced; the foreign file is no chunk
             (named(5), G.BAD | G.FOREIGN),                                  # referenced, foreign
             (named(6), 0)]                                                  # not referenced
    want = [1, 0, 0] + [1] * 10 + [0] + [0, 1] + [0] + [0]
    listing = (None, G.digest_rows([d for d, _ in store]), np.array([f for _, f in store], np.uint8))
    rows = G.digest_rows([named(1), named(2), named(4), named(5), named(7)])
    t, _, addr = dev_strided(torch_dev, rows, 32)
    hbuf, haddr = host_strided(rows, 32)
    for device, a in ((True, addr), (False, haddr)):
        with gpu.GarbageCollector(listing, device=device) as gc:
            pos, nm = gc.mark(a, 32, 5, index_bytes=0)
            assert list(pos) == [1, 2, 3, 4] and nm == 4  # only digest 1 has its chunk
            assert list(gc.touched()) == want


def test_sweep_boundaries(gpu, torch_dev):
    """Every class at its exact boundary, bad and not, by hand; then other times on the same handle."""
    for phase1_start, oldest_writer in TIMES:
        lo = min(phase1_start - 86400, oldest_writer) - 300
        atimes = [lo - 1, lo, oldest_writer - 1, oldest_writer]
        want_act = [G.REMOVE, G.PENDING, G.PENDING, G.KEEP]
        store, sizes, at, act = [], [], [], []
        k = 0
        for flag in (0, G.BAD):
            for a, w in zip(atimes, want_act):
                for size in (0, 1 << 40):
                    store.append((named(k, 0x22), flag))
                    sizes.append(size)
                    at.append(a)
                    act.append(w)
                    k += 1
        for flag in (0, G.BAD):  # vanished: nowhere
            store.append((named(k, 0x22), flag))
            sizes.append(G.VANISHED)
            at.append(lo - 1)
            act.append(G.KEEP)
            k += 1
        touched_from = k
        for _ in range(5):  # named by the index, ancient: must stay
            store.append((named(k, 0x22), 0))
            sizes.append(1 << 40)
            at.append(1000)
            act.append(G.KEEP)
            k += 1
        listing = (None, G.digest_rows([d for d, _ in store]), np.array([f for _, f in store], np.uint8))
        rows = listing[1][touched_from:].copy()
        t, _, addr = dev_strided(torch_dev, rows, 32)
        with gpu.GarbageCollector(listing) as gc:
            gc.mark(addr, 32, rows.shape[0], index_bytes=99)
            actions, status = gc.sweep(sizes, at, phase1_start, oldest_writer)
            assert list(actions) == act
            assert status == {
                "index-file-count": 1, "index-data-bytes": 99,
                "disk-bytes": (1 + 1 + 5) << 40, "disk-chunks": 2 + 5,
                "removed-bytes": 2 << 40, "removed-chunks": 2, "removed-bad": 2,
                "pending-bytes": 4 << 40, "pending-chunks": 4, "still-bad": 4}
            with pytest.raises(gpu.ChunkerError) as e:
                gc.sweep(sizes, at, phase1_start, phase1_start + 1)
            assert e.value.code == gpu.PBS_ERR_INVALID
            # far in the future everything unnamed goes; the marks persist
            actions, status = gc.sweep(sizes, at, phase1_start + 10**7, phase1_start + 10**7)
            assert list(actions[touched_from:]) == [G.KEEP] * 5 and status["disk-chunks"] == 5
            assert status["removed-chunks"] == 8 and status["removed-bad"] == 8 and status["removed-bytes"] == 8 << 40


def test_handles(gpu, torch_dev):
    p = gpu
    la, ra, pa = case(257)
    lb, rb, pb = case(4096)
    ta, _, aa = dev_strided(torch_dev, ra, 32)
    tb, _, ab = dev_strided(torch_dev, rb, 32)
    a, b = p.GarbageCollector(la), p.GarbageCollector(lb)
    with p.GarbageCollector(la, device=False) as ha, p.GarbageCollector(lb, device=False) as hb:
        mark_all(a, aa, 32, ra.shape[0])
        assert not b.touched().any()
        mark_all(b, ab, 32, rb.shape[0])
        hbuf_a, haddr_a = host_strided(ra, 32)
        hbuf_b, haddr_b = host_strided(rb, 32)
        mark_all(ha, haddr_a, 32, ra.shape[0])
        mark_all(hb, haddr_b, 32, rb.shape[0])
        a.mark(aa, 32, 0, index_bytes=7)  # an empty index counts as a file
        ha.mark(haddr_a, 32, 0, index_bytes=7)
        same(outcome(a, pa), outcome(ha, pa))
        same(outcome(b, pb), outcome(hb, pb))
        a.close()
        same(outcome(b, pb), outcome(hb, pb))
    for call in (lambda: a.mark(aa, 32, 1), lambda: a.touched(), lambda: a.sweep(*pa[0], *TIMES[0]),
                 lambda: a.mark_index(b"\0" * 4096)):
        with pytest.raises(p.ChunkerError) as e:
            call()
        assert e.value.code == p.PBS_ERR_INVALID
    assert a.table_log2 == 0
    for bad_stride, shift in ((24, 0), (36, 0), (32, 4), (40, 1)):
        with pytest.raises(p.ChunkerError) as e:
            b.mark(ab + shift, bad_stride, 4)
        assert e.value.code == p.PBS_ERR_INVALID
    b.close()
    a.close()
    p.gc_release()  # no handle alive
    p.gc_release()
    with p.GarbageCollector(la) as c:  # and the work areas come back
        mark_all(c, aa, 32, ra.shape[0])


def test_garbage_collection_on_a_real_store_device(gpu, torch_dev, tmp_path):
    G.run_real_store(gpu, tmp_path, device=True)
