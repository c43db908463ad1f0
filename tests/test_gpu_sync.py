"""The sync job on the GPU (include/pbs_sync.h): the device handle must equal the host mirror and
the model of the reference exactly -- verdicts, both lists, kinds and status per submitted blob,
the result struct, the listing with its present bytes, the entry count and the table's L -- on the
planted cases of tests/splanted.py, by hand and through pull_index over a resident source."""
import numpy as np
import pytest

import splanted as s
import vplanted as v

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_dev(gpu):
    import torch

    torch.cuda.set_device(0)
    yield torch
    gpu.sync_release()
    gpu.verify_release()
    gpu.blob_encode_release()


def _host(arr):
    return arr, None


def _uploader(torch):
    """Blobs into device memory, the first one 3 bytes past a 16-byte boundary."""
    def upload(arr):
        t = torch.zeros(arr.size + 19, dtype=torch.uint8, device="cuda")
        lead = (-t.data_ptr()) % 16 + 3
        if arr.size:
            t[lead:lead + arr.size] = torch.from_numpy(arr.copy()).cuda()
        torch.cuda.synchronize()
        return t.data_ptr() + lead, t
    return upload


def _device(gpu):
    return lambda listing, reserve: gpu.SyncWorker(listing, reserve=reserve)


def _mirror(gpu):
    return lambda listing, reserve: gpu.SyncWorker(listing, reserve=reserve, device=False)


@pytest.mark.parametrize("how", ["hand", "image"])
def test_device_equals_the_model_and_the_mirror(gpu, oracle, torch_dev, how):
    """plan (or plan_index) / submit / finish on every planted case, against the model; the mirror
    on the same cases must give the model's answers too (so device == mirror == model)."""
    up = _uploader(torch_dev)
    bad = []
    for c in s.cases(oracle):
        want = s.expected(oracle, c)
        bad += [("device",) + x for x in s.run_case(_device(gpu), c, want, up, how=how)]
        bad += [("mirror",) + x for x in s.run_case(_mirror(gpu), c, want, _host, how=how)]
    assert not bad, bad[:10]


@pytest.mark.parametrize("budget", ["one", "two", "all"])
def test_pull_index_on_a_resident_source(gpu, oracle, torch_dev, budget):
    """pull_index over the source store in device memory at budgets of one blob a batch, about two,
    and everything in one: identical outcomes, the model's."""
    up = _uploader(torch_dev)
    bad = []
    for c in s.cases(oracle):
        rows, blobs, off = s.remote_stream(c)
        ptr, keep = up(blobs)
        bad += s.run_case(_device(gpu), c, s.expected(oracle, c), up, how="pull", budget={"one": 1, "two": 700, "all": 0}[budget],
                          remote=(rows, ptr, off))
        del keep
    assert not bad, bad[:10]


@pytest.mark.parametrize("batch", [1, 2])
def test_submit_in_batches(gpu, oracle, torch_dev, batch):
    for label in ("planted/m33/n257/seed1", "growth"):
        c = s.case(oracle, label)
        assert s.run_case(_device(gpu), c, s.expected(oracle, c), _uploader(torch_dev), batch=batch) == []


def _big_indexes():
    """m = 2^16 listed digests and three indexes of n = 2^18: about half the entries repeat within
    the index, a quarter name listed chunks, a quarter are new (and the later indexes name chunks
    of the earlier ones)."""
    rng = np.random.default_rng(0x62696773)
    m, n = 1 << 16, 1 << 18
    store = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    out, pool = [], store
    for _ in range(3):
        fresh = rng.integers(0, 256, (n // 4, 32), dtype=np.uint8)
        base = np.concatenate([fresh, pool[rng.integers(0, pool.shape[0], n // 4)]])
        rows = np.concatenate([base, base[rng.integers(0, base.shape[0], n // 2)]])
        out.append(np.ascontiguousarray(rows[rng.permutation(n)]))
        pool = np.concatenate([pool, fresh])
    return store, out


def test_many_workgroups_equal_the_mirror(gpu, torch_dev):
    """One size that fills many workgroups: the full verdict array, both lists, the listing and L
    against the mirror through three indexes and one new_group on the same handles.  Nothing is
    submitted: the plans are aborted, so every appended entry stays absent and claimed."""
    store, indexes = _big_indexes()
    sizes = np.full(indexes[0].shape[0], 4096, dtype=np.uint64)
    with gpu.SyncWorker((None, store)) as w, gpu.SyncWorker((None, store), device=False) as hw:
        assert w.table_log2 == hw.table_log2 == 17
        for step, rows in enumerate(indexes):
            if step == 2:
                w.new_group()
                hw.new_group()
            got, want = w.plan(rows, sizes), hw.plan(rows, sizes)
            for name, a, b in zip(("verdict", "fetch_store", "fetch_entry", "touch_store"), got, want):
                assert np.array_equal(a, b), (step, name, a.size, b.size, np.flatnonzero(a[:min(a.size, b.size)] != b[:min(a.size, b.size)])[:4])
            assert (np.bincount(got[0], minlength=3) > (rows.shape[0] // 8 if step == 0 else 0)).all()
            assert (w.count, w.table_log2) == (hw.count, hw.table_log2)
            w.abort_index()
            hw.abort_index()
        assert w.table_log2 == 21  # (2 (2^16 + 2^18) > 2^17: table_log2_for(2^16 + 2^18) + 1, and no growth after)
        (dg, pr), (hdg, hpr) = w.listing(), hw.listing()
        assert np.array_equal(dg, hdg) and np.array_equal(pr, hpr) and pr.sum() == store.shape[0]


def test_two_live_handles_are_independent(gpu, oracle, torch_dev):
    gpu.sync_release()  # with none alive
    a, b = s.case(oracle, "growth"), s.case(oracle, "two-groups")
    up = _uploader(torch_dev)
    ea, eb = s.expected(oracle, a), s.expected(oracle, b)
    with gpu.SyncWorker(s.listing(a)) as wa, gpu.SyncWorker(s.listing(b)) as wb:
        ixa, ixb = a.steps[0], b.steps[0]
        wa.plan(v.digest_rows(ixa.digests), ixa.sizes)  # a's plan stays open, and grows a's table
        got = s.by_hand(wb, b, ixb, up)                 # b's index inside a's
        assert s.outcome_diff(got, eb[0]) == []
        gpu.sync_release()                              # with two alive and one plan open
        wa.abort_index()
        assert (wa.count, wa.table_log2) == (ea[0]["count"], ea[0]["table_log2"])
        wa.new_group()
        got = s.by_hand(wa, a, ixa, up)
        want = dict(ea[0])
        want["result"] = dict(want["result"], appended=0)  # (the aborted plan appended them)
        assert s.outcome_diff(got, want) == []
        assert s.outcome_diff(s.by_hand(wb, b, b.steps[1], up), eb[1]) == []
    gpu.sync_release()


def test_abort_and_argument_errors_on_the_device(gpu, oracle, torch_dev):
    c = s.case(oracle, "two-groups")
    ix, e = c.steps[0], s.expected(oracle, c)[0]
    dg = v.digest_rows(ix.digests)
    blobs = [c.remote[ix.digests[i]] for i in e["fetch_entry"]]
    off = np.concatenate([[0], np.cumsum([len(b) for b in blobs])]).astype(np.uint64)
    ptr, keep = _uploader(torch_dev)(np.frombuffer(b"".join(blobs), np.uint8))
    INVALID = gpu.PBS_ERR_INVALID

    def code(f, *a, **k):
        with pytest.raises(gpu.ChunkerError) as err:
            f(*a, **k)
        return err.value.code

    w = gpu.SyncWorker(s.listing(c))
    assert code(w.finish) == INVALID and code(w.lists) == INVALID and code(w.submit, ptr, off) == INVALID
    w.plan(dg, ix.sizes)
    assert code(w.plan, dg, ix.sizes) == INVALID and code(w.plan_index, e["image"]) == INVALID
    assert code(w.new_group) == INVALID and code(w.finish) == INVALID
    assert code(w.submit, ptr, np.concatenate([off, [off[-1]]])) == INVALID
    w.submit(ptr, off[:2])
    w.abort_index()                                                    # mid-plan: claims, entries and the insert stay
    assert w.count == 5 and list(w.listing()[1]) == [1, 1, 1, 1, 0]
    assert list(w.plan(dg, ix.sizes)[0]) == [s.DUP] * 4
    w.finish()
    for bad in (e["image"][:4095], e["image"][:-1], b"\0" + e["image"][1:]):
        assert code(w.plan_index, bad) == INVALID
    assert w.plan_index(e["image"], (e["honest"][0] + 1, None))[0] == v.WRONG_SIZE
    assert w.plan_index(e["image"], (None, bytes(32)))[0] == v.WRONG_CSUM
    assert code(w.finish) == INVALID and w.count == 5
    w.new_group()
    assert list(w.plan_index(e["image"], e["honest"])[1]) == [s.EXISTS, s.FETCH, s.EXISTS, s.DUP]
    w.close()
    for f, a in ((w.listing, ()), (w.plan, (dg, ix.sizes)), (w.finish, ()), (w.abort_index, ()), (w.new_group, ()),
                 (w.submit, (ptr, off))):
        assert code(f, *a) == INVALID
    assert w.count == 0 and w.table_log2 == 0


def test_pull_snapshot_on_the_device(gpu, oracle, torch_dev, tmp_path):
    s.check_pull_snapshot(gpu, oracle, tmp_path, device=True)
