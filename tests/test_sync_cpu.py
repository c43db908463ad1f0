"""The sync job on the CPU: the planted inputs of tests/splanted.py, and the host mirror
(pbs_sync_*_host) and the Python front end (SyncWorker(device=False), pull_snapshot) against the
model of the reference.

Expected values come from the model of splanted.py, the oracle, tests/aesgcm_ref.py and hashlib --
never from the library under test.  No GPU is used.
"""
import numpy as np
import pytest

import dplanted as d
import splanted as s
import vplanted as v


def _host(arr):
    return arr, None


def _mirror(pbschunk):
    return lambda listing, reserve: pbschunk.SyncWorker(listing, reserve=reserve, device=False)


def test_constants_match_the_library(pbschunk):
    p = pbschunk
    assert (p.SYNC_DUP, p.SYNC_EXISTS, p.SYNC_FETCH) == (s.DUP, s.EXISTS, s.FETCH)
    assert p.SYNC_ST_LOAD_FAILED == s.LOAD_FAILED and p.SYNC_NONE == s.NONE
    assert tuple(k for k, _ in p.SyncResult._fields_)[:len(s.RESULT_KEYS)] == s.RESULT_KEYS


def test_planted_cases_cover_the_edges(pbschunk, oracle):
    cs = {c.label: c for c in s.cases(oracle)}
    assert {len(c.steps[0].digests) for c in cs.values() if c.label.startswith("planted/m33/")} == set(s.N_SET)
    assert {len(c.listing) for c in cs.values() if c.label.startswith("planted/")} >= set(s.M_SET)
    ix = cs["planted/m33/n257/seed1"].steps[0]
    assert ix.digests[63] == ix.digests[64] and ix.digests[255] == ix.digests[256] and ix.digests[0] == ix.digests[-1]
    # every status of a submitted blob, all four kinds good, encrypted blobs verified by CRC alone
    e = s.expected(oracle, cs["planted/m33/n1000/seed1"])[0]
    assert set(e["status"]) == {d.OK, d.TOO_SMALL, d.BAD_MAGIC, d.BAD_CRC, v.BAD_FRAME, d.BAD_DIGEST, d.BAD_SIZE,
                                s.LOAD_FAILED}
    assert {k for k, st in zip(e["kinds"], e["status"]) if st == d.OK} == {0, 1, 2, 3}
    assert v.specials_hold(oracle) == []
    # the capacity rule around the minimum table of 64 slots
    L = {(m, n): s.expected(oracle, cs[f"planted/m{m}/n{n}/seed2"])[0]["table_log2"] for m in s.M_SET for n in (1, 65)}
    assert [L[m, 1] for m in s.M_SET] == [6, 6, 6, 8, 7] and [L[m, 65] for m in s.M_SET] == [9, 9, 9, 9, 9]
    # one digest a thousand times: one claiming entry, the lowest
    for label, verdict in (("repeat1000/absent", s.FETCH), ("repeat1000/present", s.EXISTS)):
        e = s.expected(oracle, cs[label])[0]
        assert e["verdict"] == [verdict] + [s.DUP] * 999
        assert e["fetch_entry"] == ([0] if verdict == s.FETCH else []) and e["result"]["appended"] == (verdict == s.FETCH)
    # the chain: one prefix, home slot capacity - 3 by the library's own hash, half listed and half new
    c = cs["chain300"]
    digs = c.steps[0].digests
    assert len({x[:8] for x in digs}) == 1 and len(set(digs)) == 300
    assert pbschunk.gc_home_slot(digs[0], s.CHAIN_L) == (1 << s.CHAIN_L) - 3
    e = s.expected(oracle, c)[0]
    assert e["table_log2"] == s.CHAIN_L and e["verdict"] == [s.EXISTS, s.FETCH] * 150
    assert e["fetch_store"] == list(range(150, 300)) and e["result"]["inserted"] == 75
    # a digest at three listing positions: the lowest is the chunk
    e = s.expected(oracle, cs["triple"])[0]
    assert e["touch_store"] == [3, 1, 0] and e["verdict"] == [s.FETCH, s.EXISTS, s.EXISTS, s.DUP, s.EXISTS]
    # growth: 40 entries in 128 slots, then 100 more do not fit 1/2: 2^(8 + 1 + 1)
    g = s.expected(oracle, cs["growth"])
    assert s.begin_log2(40, 0) == 7 and g[0]["table_log2"] == 10 and g[1]["table_log2"] == 10
    assert g[0]["count"] == 140 and g[0]["result"]["load_failed"] == 11 and g[1]["result"]["dup"] > 30
    assert g[3]["result"]["appended"] == 0 and g[3]["result"]["fetch"] > 0  # what could not be fetched is asked for again
    # two groups
    t = s.expected(oracle, cs["two-groups"])
    assert t[0]["verdict"] == [s.FETCH, s.FETCH, s.EXISTS, s.DUP] and t[0]["status"] == [d.OK, d.BAD_CRC]
    assert t[1]["verdict"] == [s.DUP] * 4 + [s.FETCH]
    assert t[3]["verdict"] == [s.EXISTS, s.FETCH, s.EXISTS, s.DUP] and t[3]["fetch_store"] == t[0]["fetch_store"][1:]
    assert t[3]["result"]["appended"] == 0 and t[3]["result"]["first_failed"] == 0
    assert [x["index_check"] for x in t[4:]] == [v.WRONG_SIZE, v.WRONG_CSUM] and t[5]["present"] == t[3]["present"]


@pytest.mark.parametrize("how", ["hand", "image"])
def test_host_mirror_equals_the_model(pbschunk, oracle, how):
    """plan (or plan_index) / submit / finish of the mirror on every planted case: verdicts, both
    lists, kinds and status per blob, the result struct, the listing and table_log2."""
    bad = []
    for c in s.cases(oracle):
        bad += s.run_case(_mirror(pbschunk), c, s.expected(oracle, c), _host, how=how)
    assert not bad, bad[:10]


@pytest.mark.parametrize("batch", [1, 2])
def test_host_mirror_in_batches(pbschunk, oracle, batch):
    for label in ("planted/m33/n257/seed1", "growth"):
        c = s.case(oracle, label)
        assert s.run_case(_mirror(pbschunk), c, s.expected(oracle, c), _host, batch=batch) == []


@pytest.mark.parametrize("budget", [0, 1, 700])
def test_host_mirror_pull_index_equals_the_model(pbschunk, oracle, budget):
    """pull_index over a resident source at three budgets: one blob a batch, about two, all."""
    bad = []
    for c in s.cases(oracle):
        bad += s.run_case(_mirror(pbschunk), c, s.expected(oracle, c), _host, how="pull", budget=budget,
                          remote=s.remote_stream(c))
    assert not bad, bad[:10]


def test_abort_keeps_claims_and_appended_entries(pbschunk, oracle):
    c = s.case(oracle, "growth")
    ix = c.steps[0]
    e = s.expected(oracle, c)[0]
    with pbschunk.SyncWorker(s.listing(c), device=False) as w:
        vd, fs, fe, ts = w.plan(v.digest_rows(ix.digests), ix.sizes)
        again = w.lists()
        assert [list(x) for x in again] == [list(fs), list(fe), list(ts)]
        blobs = [c.remote[ix.digests[int(i)]] for i in fe[:3]]
        off = np.concatenate([[0], np.cumsum([len(b) for b in blobs])])
        w.submit(np.frombuffer(b"".join(blobs), np.uint8), off)
        w.abort_index()
        dg, pr = w.listing()
        assert w.count == 140 and [bytes(r) for r in dg] == e["digests"]
        assert list(pr) == [1] * 43 + [0] * 97                      # the three inserts stay
        vd2, fs2, _, _ = w.plan(v.digest_rows(ix.digests), ix.sizes)
        assert (vd2 == s.DUP).all() and fs2.size == 0               # every claim stays
        w.finish()
        w.new_group()
        vd3, fs3, fe3, _ = w.plan(v.digest_rows(ix.digests), ix.sizes)
        assert list(vd3) == [s.EXISTS] * 3 + [s.FETCH] * 97 and list(fs3) == list(range(43, 140)) and w.count == 140
        w.abort_index()


def test_argument_errors(pbschunk, oracle):
    p = pbschunk
    INVALID = p.PBS_ERR_INVALID
    c = s.case(oracle, "two-groups")
    ix, e = c.steps[0], s.expected(oracle, c)[0]
    dg = v.digest_rows(ix.digests)
    blobs = [c.remote[ix.digests[i]] for i in e["fetch_entry"]]
    raw = np.frombuffer(b"".join(blobs), np.uint8)
    off = np.concatenate([[0], np.cumsum([len(b) for b in blobs])]).astype(np.uint64)

    def code(f, *a, **k):
        with pytest.raises(p.ChunkerError) as err:
            f(*a, **k)
        return err.value.code

    w = p.SyncWorker(s.listing(c), device=False)
    assert code(w.finish) == INVALID and code(w.lists) == INVALID      # no plan
    assert code(w.submit, raw, off[:2]) == INVALID
    w.plan(dg, ix.sizes)
    assert code(w.plan, dg, ix.sizes) == INVALID                       # plan during plan
    assert code(w.plan_index, e["image"]) == INVALID
    assert code(w.new_group) == INVALID                                # an index is open
    assert code(w.finish) == INVALID                                   # early finish
    assert code(w.submit, raw, np.concatenate([off, [off[-1]]])) == INVALID   # oversubmit: three of two
    assert code(w.submit, raw, np.array([5, 3], np.uint64)) == INVALID
    w.submit(raw, off[:2])
    assert code(w.finish) == INVALID                                   # one of two submitted
    w.submit(raw[int(off[1]):], off[1:] - off[1])
    assert s.outcome_diff(dict(e, result=w.finish()), e) == []
    assert code(w.finish) == INVALID                                   # finished already
    w.abort_index()                                                    # no plan: nothing
    before = w.listing()
    img = e["image"]
    for bad in (img[:4095], img[:-1], b"\0" + img[1:]):                # truncated, ragged, wrong magic
        assert code(w.plan_index, bad) == INVALID
    for info, want in (((e["honest"][0] + 1, e["honest"][1]), v.WRONG_SIZE), ((e["honest"][0], bytes(32)), v.WRONG_CSUM)):
        assert w.plan_index(img, info)[0] == want                      # nothing is claimed, no plan is open
        assert code(w.finish) == INVALID
    assert w.count == 5 and all(np.array_equal(a, b) for a, b in zip(before, w.listing()))
    w.new_group()
    assert list(w.plan_index(img, e["honest"])[1]) == [s.EXISTS, s.FETCH, s.EXISTS, s.DUP]
    w.close()
    w.close()
    for f, a in ((w.listing, ()), (w.plan, (dg, ix.sizes)), (w.finish, ()), (w.abort_index, ()), (w.new_group, ()),
                 (w.lists, ()), (w.submit, (raw, off)), (w.plan_index, (img,))):
        assert code(f, *a) == INVALID                                  # a dead handle
    assert w.count == 0 and w.table_log2 == 0


def test_count_plus_n_at_the_limit(pbschunk):
    """count + n < 2^32 - 16: the limit is checked before any array is read."""
    import ctypes

    L, h = pbschunk.lib(), ctypes.c_void_p(None)
    one = np.zeros(32, np.uint8)
    assert L.pbs_sync_begin_host(one.ctypes.data, 1, 0, ctypes.byref(h), None) == pbschunk.PBS_OK
    nf, nt, lim = ctypes.c_size_t(0), ctypes.c_size_t(0), (1 << 32) - 16
    for n, want in ((lim - 1, pbschunk.PBS_ERR_INVALID), (lim, pbschunk.PBS_ERR_INVALID)):
        assert L.pbs_sync_plan_host(h, one.ctypes.data, one.ctypes.data, n, None, None, None, 0, ctypes.byref(nf), None, 0,
                                    ctypes.byref(nt), None) == want
    assert L.pbs_sync_begin_host(one.ctypes.data, 1, lim - 1, ctypes.byref(ctypes.c_void_p(None)), None) == pbschunk.PBS_ERR_INVALID
    assert L.pbs_sync_plan_host(h, None, None, 0, None, None, None, 0, ctypes.byref(nf), None, 0, ctypes.byref(nt), None) == pbschunk.PBS_OK
    L.pbs_sync_end_host(h)


def test_pull_snapshot_on_a_real_store(pbschunk, oracle, tmp_path):
    s.check_pull_snapshot(pbschunk, oracle, tmp_path, device=False)
