"""The verify job on the CPU: the planted inputs of tests/vplanted.py proved with the reference
functions, and the host mirror (pbs_verify_*_host, pbs_verify_blob_host) and the Python front end
(VerifyWorker(device=False), verify_blob, bad_chunk_path, verify_snapshot) against the model.

Expected values come from the model of vplanted.py, the oracle, tests/aesgcm_ref.py, zlib and
hashlib -- never from the library under test.  No GPU is used.
"""
import hashlib
import os

import numpy as np
import pytest

import dplanted as d
import gplanted as g
import vplanted as v


def _host(arr):
    return arr, None


def test_constants_match_the_library(pbschunk):
    p = pbschunk
    assert (p.VERIFY_UNKNOWN, p.VERIFY_VERIFIED, p.VERIFY_CORRUPT) == (v.UNKNOWN, v.VERIFIED, v.CORRUPT)
    assert (p.VERIFY_MODE_NONE, p.VERIFY_MODE_ENCRYPT) == (v.MODE_NONE, v.MODE_ENCRYPT)
    assert p.VERIFY_ST_LOAD_FAILED == v.LOAD_FAILED and not 0 <= v.LOAD_FAILED <= 10
    assert (p.VERIFY_INDEX_OK, p.VERIFY_INDEX_WRONG_SIZE, p.VERIFY_INDEX_WRONG_CSUM) == (0, v.WRONG_SIZE, v.WRONG_CSUM)
    assert p.BLOB_ST_BAD_FRAME == v.BAD_FRAME
    assert tuple(k for k, _ in p.VerifyResult._fields_) == v.RESULT_KEYS
    assert p.verify_crypt_mode("encrypt") == v.MODE_ENCRYPT
    assert p.verify_crypt_mode("none") == p.verify_crypt_mode("sign-only") == v.MODE_NONE  # manifest.rs:39-44
    with pytest.raises(ValueError):
        p.verify_crypt_mode("sign")


def test_planted_statuses_hold_by_the_reference(oracle):
    """Every special blob has the status it is planted for, by the reference functions alone, and
    every status is there."""
    assert v.specials_hold(oracle) == []
    have = {st for *_, st in v.specials(oracle)}
    assert have == {d.OK, d.TOO_SMALL, d.BAD_MAGIC, d.BAD_CRC, v.BAD_FRAME, d.BAD_DIGEST, d.BAD_SIZE, v.LOAD_FAILED}
    lens = {len(b) for _, _, b, _, _, st in v.specials(oracle) if st == d.TOO_SMALL}
    assert lens == {0, 11, 43}


def test_planted_cases_cover_the_edges(oracle):
    cs = {c.label: c for c in v.cases(oracle)}
    for m in v.BOUNDARY:
        assert any(len(c.store) == m for c in cs.values()), m
        assert any(len(c.indexes[0].digests) == m for c in cs.values()), m
    c = cs["planted/m300/n257/seed2/mode0"]
    ix = c.indexes[0]
    assert ix.digests[255] == ix.digests[256] and ix.digests[0] == ix.digests[-1]
    e = v.expected(oracle, c)[0]
    # the representative is the LOWEST occurrence
    first = {}
    for pos, dg in enumerate(ix.digests):
        first.setdefault(dg, pos)
    low = {}
    for j, (dg, _) in enumerate(c.store):
        low.setdefault(dg, j)
    assert e["todo_store"] == sorted(e["todo_store"])
    assert all(low[ix.digests[t]] == j and first[ix.digests[t]] == t for j, t in zip(e["todo_store"], e["todo_entry"]))
    # a digest twice in the store: only the lowest position has a state
    dup = [j for j, (dg, _) in enumerate(c.store) if low[dg] != j]
    assert len(dup) == 2 and all(e["states"][j] == v.UNKNOWN for j in dup)
    assert sorted(int(e["states"][low[c.store[j][0]]]) for j in dup) == [v.VERIFIED, v.CORRUPT]
    # the same digest with two sizes: the first one's decides
    sized = {}
    for dg, s in zip(ix.digests, ix.sizes):
        sized.setdefault(dg, []).append(s)
    two = {dg: s for dg, s in sized.items() if len(set(s)) == 2}
    assert len(two) == 2
    got = sorted((s[0] < s[1], int(e["states"][low[dg]])) for dg, s in two.items())
    assert got == [(False, v.CORRUPT), (True, v.VERIFIED)]
    # clusters that wrap the table's end
    L = v.gcplanted.table_log2(len(c.store))
    assert sum(v.gcplanted.home_slot(dg, L) >= (1 << L) - 4 for dg, _ in c.store) >= 4
    # a mismatching chunk that is otherwise good ends VERIFIED, and the index fails
    mm = v.expected(oracle, cs["mismatch/encrypted-chunks-none-index"])[0]
    assert (mm["states"] == v.VERIFIED).all() and mm["result"]["errors"] == 5 and not mm["result"]["ok"]
    # the sequence: nothing is loaded for what the first index verified; every occurrence of what
    # it found corrupt counts; the wrong infos change nothing
    s = v.expected(oracle, cs["sequence"])
    assert s[1]["result"]["skipped_verified"] > 100 and s[1]["result"]["loaded"] == 8
    assert s[1]["result"]["errors"] == s[1]["result"]["skipped_corrupt"] + s[1]["result"]["missing"] > 10
    assert [x["result"]["index_check"] for x in s] == [0, 0, v.WRONG_SIZE, v.WRONG_CSUM]
    assert np.array_equal(s[2]["states"], s[1]["states"]) and np.array_equal(s[3]["states"], s[1]["states"])


def test_host_mirror_by_hand_equals_the_model(pbschunk, oracle):
    """plan / submit / finish of the mirror on every planted case: results field by field, the
    todo lists, kinds and status per blob, corrupt_store, missing_pos and the states."""
    bad = []
    for case in v.cases(oracle):
        want = v.expected(oracle, case)
        with pbschunk.VerifyWorker(v.listing(case), device=False) as w:
            for ix, e in zip(case.indexes, want):
                if e["result"]["index_check"]:
                    continue  # (the manifest's check belongs to verify_index)
                got = v.by_hand(w, case, ix, _host)
                bad += [(case.label, ix.name) + x for x in v.outcome_diff(got, e)]
    assert not bad, bad[:10]


@pytest.mark.parametrize("batch", [1, 2, 7])
def test_host_mirror_in_batches(pbschunk, oracle, batch):
    case = next(c for c in v.cases(oracle) if c.label == "planted/m65/n257/seed1/mode0")
    with pbschunk.VerifyWorker(v.listing(case), device=False) as w:
        got = v.by_hand(w, case, case.indexes[0], _host, batch=batch)
    assert v.outcome_diff(got, v.expected(oracle, case)[0]) == []


@pytest.mark.parametrize("budget", [0, 1, 20000])
def test_host_mirror_whole_index_equals_the_model(pbschunk, oracle, budget):
    """pbs_verify_index_host over the .didx images, the store resident: the manifest's check
    included, at three batch budgets."""
    bad = []
    for case in v.cases(oracle):
        want = v.expected(oracle, case, resident=True)
        blobs, off = v.store_stream(case)
        with pbschunk.VerifyWorker(v.listing(case), device=False) as w:
            for ix, e in zip(case.indexes, want):
                res, cs, mp = w.verify_index(e["image"], ix.mode, info=v.resolve_info(ix, e["honest"]),
                                             store=(blobs, off), budget=budget)
                got = dict(result=res, corrupt_store=[int(x) for x in cs], missing_pos=[int(x) for x in mp],
                           states=w.states())
                bad += [(case.label, ix.name) + x for x in v.outcome_diff(got, e)]
    assert not bad, bad[:10]


def test_whole_index_on_a_fixed_index(pbschunk, oracle):
    """A .fidx image: chunk_info's sizes, the last chunk clipped to the archive's size."""
    cs_, size = 4096, 2 * 4096 + 5
    data = d._chunk(77, size, True)
    chunks = [data[i * cs_:(i + 1) * cs_] for i in range(3)]
    digs = [d.plain_digest(c) for c in chunks]
    blobs = [d.make_blob(oracle, i % 2, c, g.KEY1, g._iv(1)) for i, c in enumerate(chunks)]
    image, csum = pbschunk.fidx_build(v.digest_rows(digs), size, cs_)
    assert hashlib.sha256(b"".join(digs)).digest() == csum
    off = np.concatenate([[0], np.cumsum([len(b) for b in blobs])]).astype(np.uint64)
    raw = np.frombuffer(b"".join(blobs), np.uint8)
    with pbschunk.VerifyWorker((None, v.digest_rows(digs)), device=False) as w:
        res, _, _ = w.verify_index(image, "none", info=(size, csum), store=(raw, off))
        assert res["ok"] == 1 and res["loaded"] == 3 and res["decoded_bytes"] == size
        res, _, _ = w.verify_index(image, "none", info=(size + 1, csum), store=(raw, off))
        assert (res["ok"], res["index_check"]) == (0, v.WRONG_SIZE)
        res, _, _ = w.verify_index(image, "none", info=(size, bytes(32)), store=(raw, off))
        assert (res["ok"], res["index_check"]) == (0, v.WRONG_CSUM)
        res, _, _ = w.verify_index(image, "none", info=(size, csum), store=(raw, off))
        assert res["ok"] == 1 and res["loaded"] == 0 and res["skipped_verified"] == 3
    # the clipped chunk under a full-size blob is not the chunk the index names
    long_last = d.make_blob(oracle, 0, data[2 * cs_:] + b"x", g.KEY1, g._iv(1))
    blobs2 = blobs[:2] + [long_last]
    off2 = np.concatenate([[0], np.cumsum([len(b) for b in blobs2])]).astype(np.uint64)
    with pbschunk.VerifyWorker((None, v.digest_rows(digs)), device=False) as w:
        res, corrupt, _ = w.verify_index(image, "none", store=(np.frombuffer(b"".join(blobs2), np.uint8), off2))
        assert res["ok"] == 0 and list(corrupt) == [2] and res["errors"] == 1


def test_verify_blob(pbschunk, oracle):
    p = pbschunk
    cases = []
    text = d._chunk(5, 9000, True)
    for kind in range(4):
        raw = d.make_blob(oracle, kind, text if kind in (1, 3) else b"config", g.KEY1, g._iv(kind))
        assert d.kind_of(raw) == kind
        cases.append((f"good{kind}", raw, len(raw), hashlib.sha256(raw).digest()))
    good1 = cases[1][1]
    cases.append(("wrong-size", good1, len(good1) + 1, hashlib.sha256(good1).digest()))
    cases.append(("wrong-csum", good1, len(good1), bytes(32)))
    for name, raw in (("bad-crc", d._flip(good1, 40, 1)), ("bad-crc-enc", d._flip(cases[2][1], 46, 1)),
                      ("bad-magic", d._flip(good1, 1, 1)), ("short", good1[:11]), ("empty", b""),
                      ("enc-43", cases[2][1][:43]),
                      ("bad-frame", d._with_crc(d._flip(good1, d.HDR, 0))), ("cut-frame", d._with_crc(good1[:-9]))):
        cases.append((name, raw, len(raw), hashlib.sha256(raw).digest()))
    names = {"": p.VERIFY_BLOB_OK, "wrong size": p.VERIFY_BLOB_WRONG_SIZE, "wrong index checksum": p.VERIFY_BLOB_WRONG_CSUM,
             "load": p.VERIFY_BLOB_LOAD, "decode": p.VERIFY_BLOB_DECODE}
    seen = set()
    for name, raw, size, csum in cases:
        want = names[v.model_verify_blob(oracle, raw, size, csum)]
        seen.add(want)
        assert p.verify_blob(raw, (size, csum)) == want, name
    assert seen == set(names.values())
    # the order: the size is looked at before the checksum, the checksum before the blob
    assert p.verify_blob(b"", (1, bytes(32))) == p.VERIFY_BLOB_WRONG_SIZE
    assert p.verify_blob(b"x", (1, bytes(32))) == p.VERIFY_BLOB_WRONG_CSUM


@pytest.mark.parametrize("existing", [0, 3, 9, 10])
def test_bad_chunk_path(pbschunk, tmp_path, existing):
    """rename_corrupted_chunk's counter (verify.rs:79-88): the first free of .0.bad .. .8.bad, and
    .9.bad whether it exists or not."""
    path = str(tmp_path / ("ab" * 32))
    for k in range(existing):
        open(f"{path}.{k}.bad", "wb").close()
    assert pbschunk.bad_chunk_path(path) == f"{path}.{min(existing, 9)}.bad"


def test_argument_errors(pbschunk, oracle):
    p = pbschunk
    INVALID = p.PBS_ERR_INVALID
    case = next(c for c in v.cases(oracle) if c.label == "mismatch/mixed")
    ix = case.indexes[0]
    dg = v.digest_rows(ix.digests)
    blobs, off = v.store_stream(case)

    def code(f, *a, **k):
        with pytest.raises(p.ChunkerError) as e:
            f(*a, **k)
        return e.value.code

    w = p.VerifyWorker(v.listing(case), device=False)
    assert code(w.finish) == INVALID                                   # no plan
    assert code(w.submit, blobs, off[:2]) == INVALID                   # no plan
    assert code(w.plan, dg, ix.sizes, 2) == INVALID                    # no such mode
    ts, _ = w.plan(dg, ix.sizes, ix.mode)
    assert list(ts) == [0, 1, 2, 3]
    assert code(w.plan, dg, ix.sizes, ix.mode) == INVALID              # plan during plan
    assert code(w.verify_index, v.expected(oracle, case)[0]["image"], ix.mode, store=(blobs, off)) == INVALID
    assert code(w.finish) == INVALID                                   # early finish
    w.abort_index()
    assert (w.states() == v.UNKNOWN).all()
    ts, _ = w.plan(dg, ix.sizes, ix.mode)
    assert code(w.submit, blobs, np.concatenate([off, [off[-1]]])) == INVALID      # oversubmit: five of four
    assert code(w.submit, blobs, np.array([5, 3], np.uint64)) == INVALID           # descending offsets
    w.submit(blobs, off[:3])
    assert code(w.finish) == INVALID                                   # two of four submitted
    w.submit(blobs[int(off[2]):], off[2:] - off[2])
    res, _, _ = w.finish(len(ix.digests))
    assert v.result_diff(res, v.expected(oracle, case)[0]["result"]) == []
    assert code(w.finish) == INVALID                                   # finished already
    w.abort_index()                                                    # no plan: nothing
    img = v.expected(oracle, case)[0]["image"]
    assert code(w.verify_index, img[:4095], ix.mode, store=(blobs, off)) == INVALID
    assert code(w.verify_index, img[:-1], ix.mode, store=(blobs, off)) == INVALID
    assert code(w.verify_index, b"\0" + img[1:], ix.mode, store=(blobs, off)) == INVALID
    before = w.states().copy()
    w.close()
    w.close()
    for f, a in ((w.states, ()), (w.plan, (dg, ix.sizes, ix.mode)), (w.finish, ()), (w.abort_index, ()),
                 (w.submit, (blobs, off))):
        assert code(f, *a) == INVALID                                  # a dead handle
    assert (before != v.UNKNOWN).all()
    with pytest.raises(ValueError):
        p.VerifyWorker(v.listing(case), device=False).verify_index(img, 0, store=(blobs, off[:-1]))


def test_verify_snapshot_on_a_real_store(pbschunk, oracle, tmp_path):
    p = pbschunk
    base = str(tmp_path / "store")
    snap, what = v.build_snapshot(oracle, p, base)
    listing = p.list_chunk_store(base)
    with p.VerifyWorker(listing, device=False) as w:
        verdict, files = p.verify_snapshot(base, snap, w)
        assert verdict == "failed"
        by = {name: (err, res) for name, err, res in files}
        assert list(by) == ["qemu-server.conf.blob", "root.pxar.didx", "drive-scsi0.img.fidx"]
        assert by["qemu-server.conf.blob"] == (None, None)
        err, res = by["root.pxar.didx"]
        assert err == "chunks could not be verified"
        # one corrupt chunk (once in the index), one absent (once): two errors; 38 good ones
        assert (res["errors"], res["newly_corrupt"], res["missing"], res["newly_verified"]) == (2, 1, 1, 38)
        assert res["entries"] == 45 and res["loaded"] == 39
        err, res = by["drive-scsi0.img.fidx"]
        assert err is None and res["ok"] == 1 and res["loaded"] == 4 and res["decoded_bytes"] == 3 * 4096 + 100
        assert os.path.exists(what["corrupt_path"])  # rename=False renames nothing
        # the same snapshot again on the same worker: nothing is loaded, the corrupt chunk counts again
        verdict, files = p.verify_snapshot(base, snap, w, rename=True)
        res = files[1][2]
        assert verdict == "failed" and (res["loaded"], res["skipped_corrupt"], res["skipped_verified"]) == (0, 1, 43)
        assert os.path.exists(what["corrupt_path"])  # (found corrupt by the earlier run: not this index's to rename)
    with p.VerifyWorker(listing, device=False) as w:
        verdict, files = p.verify_snapshot(base, snap, w, rename=True, batch_bytes=1)
        assert verdict == "failed" and files[1][2]["newly_corrupt"] == 1
        assert not os.path.exists(what["corrupt_path"]) and os.path.exists(what["corrupt_path"] + ".0.bad")
    # a manifest that lies about an index, and one that does not load
    import json
    bad_files = [dict(f) for f in what["files"]]
    bad_files[1]["size"] += 1
    bad_files[2]["csum"] = "00" * 32
    bad_files.append({"filename": "notes.txt", "size": 0, "csum": "00" * 32})
    with open(os.path.join(snap, "index.json.blob"), "wb") as f:
        f.write(oracle.blob_compressed(json.dumps({"files": bad_files}).encode() + b" " * 200))
    with p.VerifyWorker(p.list_chunk_store(base), device=False) as w:
        verdict, files = p.verify_snapshot(base, snap, w)
        assert verdict == "failed"
        assert [e for _, e, _ in files][0] is None
        assert "wrong size" in files[1][1] and files[2][1] == "wrong index checksum" and "archive type" in files[3][1]
        assert (w.states() == v.UNKNOWN).all()
        with open(os.path.join(snap, "index.json.blob"), "wb") as f:
            f.write(b"not a blob")
        assert p.verify_snapshot(base, snap, w) == ("failed", [])
