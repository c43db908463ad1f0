"""The verify job on the GPU (include/pbs_verify.h): the device handle must equal the host mirror
exactly -- results, states, both lists, the todo lists, kinds and status per submitted blob -- on
the planted cases of tests/vplanted.py (the mirror itself is checked against the model of the
reference in test_verify_cpu.py)."""
import numpy as np
import pytest

import vplanted as v

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_dev(gpu):
    import torch

    torch.cuda.set_device(0)
    yield torch
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


_mirror = {}


def mirror_by_hand(gpu, oracle, case):
    """The host mirror's outcome of every index of a case by plan / submit / finish: computed once."""
    if case.label not in _mirror:
        outs = []
        with gpu.VerifyWorker(v.listing(case), device=False) as w:
            for ix, e in zip(case.indexes, v.expected(oracle, case)):
                outs.append(None if e["result"]["index_check"] else v.by_hand(w, case, ix, _host))
        _mirror[case.label] = outs
    return _mirror[case.label]


def test_device_by_hand_equals_the_mirror(gpu, oracle, torch_dev):
    """plan / submit / finish on every planted case."""
    up = _uploader(torch_dev)
    bad = []
    for case in v.cases(oracle):
        with gpu.VerifyWorker(v.listing(case)) as w:
            for ix, want in zip(case.indexes, mirror_by_hand(gpu, oracle, case)):
                if want is None:
                    continue
                got = v.by_hand(w, case, ix, up)
                bad += [(case.label, ix.name) + x for x in v.outcome_diff(got, want)]
    assert not bad, bad[:10]


def test_device_whole_index_equals_the_mirror(gpu, oracle, torch_dev):
    """pbs_verify_index_device against pbs_verify_index_host on every planted case, the store
    resident in device memory, the manifest's checks included."""
    up = _uploader(torch_dev)
    bad = []
    for case in v.cases(oracle):
        blobs, off = v.store_stream(case)
        ptr, keep = up(blobs)
        with gpu.VerifyWorker(v.listing(case)) as w, gpu.VerifyWorker(v.listing(case), device=False) as hw:
            for ix, e in zip(case.indexes, v.expected(oracle, case, resident=True)):
                info = v.resolve_info(ix, e["honest"])
                outs = []
                for worker, store in ((w, (ptr, off)), (hw, (blobs, off))):
                    res, cs, mp = worker.verify_index(e["image"], ix.mode, info=info, store=store)
                    outs.append(dict(result=res, corrupt_store=[int(x) for x in cs], missing_pos=[int(x) for x in mp],
                                     states=worker.states()))
                bad += [(case.label, ix.name) + x for x in v.outcome_diff(outs[0], outs[1])]
                bad += [(case.label, ix.name, "model") + x for x in v.outcome_diff(outs[0], e)]
        del keep
    assert not bad, bad[:10]


@pytest.mark.parametrize("budget", ["one", "two", "all"])
def test_budgets_give_identical_outcomes(gpu, oracle, torch_dev, budget):
    """budget_bytes that force one blob per batch (every blob is larger than a budget of 1 byte and
    is processed all the same), about two, and everything in one."""
    case = next(c for c in v.cases(oracle) if c.label == "planted/m65/n257/seed1/mode0")
    ix, e = case.indexes[0], v.expected(oracle, case, resident=True)[0]
    blobs, off = v.store_stream(case)
    ptr, keep = _uploader(torch_dev)(blobs)
    with gpu.VerifyWorker(v.listing(case)) as w:
        res, cs, mp = w.verify_index(e["image"], ix.mode, store=(ptr, off), budget={"one": 1, "two": 1300, "all": 0}[budget])
        got = dict(result=res, corrupt_store=[int(x) for x in cs], missing_pos=[int(x) for x in mp], states=w.states())
    assert v.outcome_diff(got, e) == []


@pytest.mark.parametrize("batch", [1, 2])
def test_submit_in_batches(gpu, oracle, torch_dev, batch):
    case = next(c for c in v.cases(oracle) if c.label == "planted/m65/n257/seed1/mode0")
    with gpu.VerifyWorker(v.listing(case)) as w:
        got = v.by_hand(w, case, case.indexes[0], _uploader(torch_dev), batch=batch)
    assert v.outcome_diff(got, mirror_by_hand(gpu, oracle, case)[0]) == []


def test_plan_order_at_the_boundaries(gpu, oracle, torch_dev):
    """todo_store ascending in store position, todo_entry the lowest occurrence, at every boundary
    m and n; an aborted plan changes nothing."""
    for case in v.cases(oracle):
        if not case.label.startswith("planted/"):
            continue
        ix = case.indexes[0]
        first, low = {}, {}
        for pos, dg in enumerate(ix.digests):
            first.setdefault(dg, pos)
        for j, (dg, _) in enumerate(case.store):
            low.setdefault(dg, j)
        with gpu.VerifyWorker(v.listing(case)) as w:
            ts, te = w.plan(v.digest_rows(ix.digests) if ix.digests else np.zeros((0, 32), np.uint8), ix.sizes, ix.mode)
            w.abort_index()
            assert (w.states() == v.UNKNOWN).all()
        ts, te = [int(x) for x in ts], [int(x) for x in te]
        assert ts == sorted(set(ts)), case.label
        assert ts == sorted({low[dg] for dg in ix.digests if dg in low}), case.label
        assert all(low[ix.digests[t]] == j and first[ix.digests[t]] == t for j, t in zip(ts, te)), case.label


def test_all_encrypted_store_needs_no_output_scratch(gpu, oracle, torch_dev):
    case = next(c for c in v.cases(oracle) if c.label == "all-encrypted")
    ix = case.indexes[0]
    blobs, off = v.store_stream(case)
    ptr, keep = _uploader(torch_dev)(blobs)
    with gpu.VerifyWorker(v.listing(case)) as w:
        ts, _ = w.plan(v.digest_rows(ix.digests), ix.sizes, ix.mode)
        assert list(ts) == list(range(len(case.store)))
        kinds, status = w.submit(ptr, off)
        t = w.timing
        assert t["scratch_bytes"] == 0 and t["encrypted"] == t["decoded"] == t["blobs"] == len(case.store)
        assert (kinds >= 2).all() and (status == 0).all()
        res, cs, mp = w.finish(len(ix.digests))
        assert res["ok"] == 1 and res["newly_verified"] == len(case.store) and cs.size == 0 and mp.size == 0
        assert (w.states() == v.VERIFIED).all()
    # the same blobs under an index of mode NONE: scratch is still not needed
    mm = next(c for c in v.cases(oracle) if c.label == "mismatch/encrypted-chunks-none-index")
    b2, o2 = v.store_stream(mm)
    p2, keep2 = _uploader(torch_dev)(b2)
    with gpu.VerifyWorker(v.listing(mm)) as w:
        w.plan(v.digest_rows(mm.indexes[0].digests), mm.indexes[0].sizes, v.MODE_NONE)
        w.submit(p2, o2)
        assert w.timing["scratch_bytes"] == 0
        res, _, _ = w.finish()
        assert res["mode_mismatch"] == 5 and res["errors"] == 5 and (w.states() == v.VERIFIED).all()


def test_two_live_handles_are_independent(gpu, oracle, torch_dev):
    gpu.verify_release()  # with none alive
    a = next(c for c in v.cases(oracle) if c.label == "planted/m65/n257/seed1/mode0")
    b = next(c for c in v.cases(oracle) if c.label == "mismatch/mixed")
    up = _uploader(torch_dev)
    with gpu.VerifyWorker(v.listing(a)) as wa, gpu.VerifyWorker(v.listing(b)) as wb:
        ixa, ixb = a.indexes[0], b.indexes[0]
        tsa, _ = wa.plan(v.digest_rows(ixa.digests), ixa.sizes, ixa.mode)
        tsb, _ = wb.plan(v.digest_rows(ixb.digests), ixb.sizes, ixb.mode)  # b's plan inside a's
        bb, ob = v.store_stream(b)
        pb, keepb = up(bb)
        wb.submit(pb, ob)
        resb, _, _ = wb.finish(len(ixb.digests))
        assert v.result_diff(resb, v.expected(oracle, b)[0]["result"]) == []
        gpu.verify_release()  # with two alive and one plan open
        assert (wa.states() == v.UNKNOWN).all()
        wa.abort_index()
        got = v.by_hand(wa, a, ixa, up)
        assert v.outcome_diff(got, mirror_by_hand(gpu, oracle, a)[0]) == []
        assert np.array_equal(wb.states(), v.expected(oracle, b)[0]["states"])
    gpu.verify_release()


def test_argument_errors_on_the_device(gpu, oracle, torch_dev):
    case = next(c for c in v.cases(oracle) if c.label == "mismatch/mixed")
    ix = case.indexes[0]
    blobs, off = v.store_stream(case)
    ptr, keep = _uploader(torch_dev)(blobs)

    def code(f, *a, **k):
        with pytest.raises(gpu.ChunkerError) as e:
            f(*a, **k)
        return e.value.code

    w = gpu.VerifyWorker(v.listing(case))
    assert code(w.finish) == gpu.PBS_ERR_INVALID
    assert code(w.submit, ptr, off) == gpu.PBS_ERR_INVALID
    w.plan(v.digest_rows(ix.digests), ix.sizes, ix.mode)
    assert code(w.plan, v.digest_rows(ix.digests), ix.sizes, ix.mode) == gpu.PBS_ERR_INVALID
    assert code(w.finish) == gpu.PBS_ERR_INVALID
    assert code(w.submit, ptr, np.concatenate([off, [off[-1]]])) == gpu.PBS_ERR_INVALID
    w.submit(ptr, off)
    res, _, _ = w.finish()
    assert v.result_diff(res, v.expected(oracle, case)[0]["result"]) == []
    w.close()
    assert code(w.states) == gpu.PBS_ERR_INVALID and code(w.finish) == gpu.PBS_ERR_INVALID


def test_verify_snapshot_on_the_device(gpu, oracle, torch_dev, tmp_path):
    """verify_snapshot(device=True) on the real store of the CPU test: the same per-file results."""
    base = str(tmp_path / "store")
    snap, what = v.build_snapshot(oracle, gpu, base)
    listing = gpu.list_chunk_store(base)
    with gpu.VerifyWorker(listing, device=False) as hw, gpu.VerifyWorker(listing) as w:
        want = gpu.verify_snapshot(base, snap, hw)
        got = gpu.verify_snapshot(base, snap, w, batch_bytes=20000)
        assert got == want and got[0] == "failed"
        assert np.array_equal(w.states(), hw.states())
        assert gpu.verify_snapshot(base, snap, w) == gpu.verify_snapshot(base, snap, hw)
