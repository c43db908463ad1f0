"""The growing digest table that the sync job and the backup session share (csrc/grow_table_dev.h):
a SyncWorker and a BackupSession, device and host mirror of each, start from one listing and take
the same digest batches.  After every batch all four must agree on the entry count, the table's L
and the digest list in order -- a new digest at the position of its lowest row -- and each device
handle's own per-entry arrays must equal its mirror's.

The listing has m = 33 entries and no reserve, so the begin table is the smallest one.  Batch 1
(257 rows) crosses one 256-lane block edge and makes the table grow.  Batch 2 (600 rows) makes the
entry arrays grow a second time with appended entries in them; the table, which batch 1 rebuilt a
factor of two above its need, still holds it.  Batch 3 (1200 rows) makes the table grow again,
this time over appended entries."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M = 33


def _fresh(rng, n):
    """n distinct digests that no earlier call returned (the first 8 bytes count up)."""
    rows = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    lo = _fresh.next
    _fresh.next += n
    rows[:, :8] = np.arange(lo, lo + n, dtype=">u8").view(np.uint8).reshape(n, 8)
    return rows


def _batches():
    rng = np.random.default_rng(0x67726F77)
    _fresh.next = 1
    listing = _fresh(rng, M)

    # batch 1: 257 rows
    b1 = _fresh(rng, 257)
    b1[256] = b1[0]        # one new digest on both sides of the block edge
    b1[255] = b1[254]      # another new digest twice, both below the edge
    b1[1] = listing[5]     # a listed digest
    b1[2] = b1[1]          # ... and again
    new1 = np.delete(b1, [1, 2, 255, 256], axis=0)

    # batch 2: 600 rows, a quarter from batch 1's new digests, a quarter listed, the rest new
    kind = rng.permutation(np.repeat([0, 1, 2], [150, 150, 300]))
    for want in (255, 256, 511, 512):  # the repeats are new digests
        if kind[want] != 2:
            other = next(i for i in np.flatnonzero(kind == 2) if i not in (255, 256, 511, 512))
            kind[want], kind[other] = kind[other], kind[want]
    b2 = np.zeros((600, 32), np.uint8)
    b2[kind == 0] = new1[rng.integers(0, len(new1), size=int((kind == 0).sum()))]
    b2[kind == 1] = listing[rng.integers(0, M, size=int((kind == 1).sum()))]
    b2[kind == 2] = _fresh(rng, int((kind == 2).sum()))
    b2[256] = b2[255]
    b2[512] = b2[511]

    # batch 3: 1200 rows, every third one a digest seen before
    b3 = _fresh(rng, 1200)
    seen = np.concatenate([listing, b1, b2])
    b3[::3] = seen[rng.integers(0, len(seen), size=400)]
    return rng, listing, [b1, b2, b3]


def _append_order(have, batch):
    """`have` and then the digests of `batch` that are not in it, each once, in row order."""
    known = {r.tobytes() for r in have}
    out = list(have)
    for r in batch:
        if r.tobytes() not in known:
            known.add(r.tobytes())
            out.append(r)
    return np.asarray(out, np.uint8).reshape(-1, 32)


def test_four_handles_grow_alike(gpu):
    import torch

    torch.cuda.set_device(0)
    rng, listing, batches = _batches()
    file_sizes = rng.integers(1, 4 << 20, size=M).astype(np.uint64)
    kinds = np.where(rng.integers(0, 2, size=M) == 0, gpu.BLOB_KIND_UNCOMPRESSED, gpu.BLOB_KIND_COMPRESSED).astype(np.uint8)
    try:
        with gpu.SyncWorker((None, listing), reserve=0) as sd, \
                gpu.SyncWorker((None, listing), reserve=0, device=False) as sm, \
                gpu.BackupSession((listing, file_sizes, kinds), reserve=0) as bd, \
                gpu.BackupSession((listing, file_sizes, kinds), reserve=0, device=False) as bm:
            handles = dict(sync_device=sd, sync_mirror=sm, backup_device=bd, backup_mirror=bm)
            l_begin = sm.table_log2
            assert {h.table_log2 for h in handles.values()} == {l_begin}
            want = listing
            logs = [l_begin]
            for b, batch in enumerate(batches):
                n = len(batch)
                sizes = rng.integers(1, 4 << 20, size=n).astype(np.uint32)  # (a repeated digest: another size per row)
                for w in (sd, sm):
                    w.plan(batch, sizes.astype(np.uint64))
                    w.abort_index()  # (an aborted plan keeps its appended entries)
                for s in (bd, bm):
                    assert s.register_previous(batch, sizes) == 0
                want = _append_order(want, batch)
                s_dev, s_mir = sd.listing(), sm.listing()
                b_dev, b_mir = bd.listing(), bm.listing()
                got = dict(sync_device=s_dev[0], sync_mirror=s_mir[0], backup_device=b_dev["digests"],
                           backup_mirror=b_mir["digests"])
                for name, h in handles.items():
                    assert h.count == sm.count == len(want), (b, name, h.count, sm.count, len(want))
                    assert h.table_log2 == sm.table_log2, (b, name, h.table_log2, sm.table_log2)
                    assert np.array_equal(got[name], want), (b, name, "digest list")
                assert np.array_equal(s_dev[1], s_mir[1]), (b, "sync present")
                for key in ("present", "known", "known_size"):
                    assert np.array_equal(b_dev[key], b_mir[key]), (b, "backup " + key)
                assert b_mir["known"][M:].all() and b_mir["known"].sum() > len(want) - M, (b, "known")
                logs.append(sm.table_log2)
            # what the batches are there for: the table grew at batch 1 and at batch 3
            assert logs[1] > logs[0] and logs[2] == logs[1] and logs[3] > logs[2], logs
    finally:
        gpu.sync_release()
        gpu.backup_release()
