"""The backup session's host mirror (include/pbs_backup.h, pbs_backup_*_host) against the Python
model of the reference (tests/bplanted.py) on every planted case: status, crc_out, ins, action,
is_duplicate, compressed_size, reg and first_failed per upload, the listing with present / size /
kind / known / known_size, the entry count and the table's L, n_done and err of the appends, the
close results with their images and statistics, and the session's counters.  No GPU."""
import hashlib
import zlib

import numpy as np
import pytest

import bplanted as b
import dplanted as d


@pytest.mark.parametrize("label", [c[0] for c in b.cases()])
def test_mirror_equals_the_model(pbschunk, oracle, label):
    c = b.case(label)
    s = b.Session(pbschunk, c[1], c[2], device=False)
    try:
        got = b.run(oracle, c, s)
    finally:
        s.close()
    assert b.diff(got, b.expected(oracle, c)) == []


def test_the_planted_outcomes_are_there(oracle):
    """The cases reach what they were planted for (by the model alone)."""
    seen_ins, seen_reg, seen_status, seen_err = set(), set(), set(), set()
    for c in b.cases():
        for name, value in b.expected(oracle, c):
            if isinstance(value, list) and len(value) == 2 and isinstance(value[1], dict) and "ins" in value[1]:
                seen_ins |= set(value[1]["ins"])
                seen_reg |= set(value[1]["reg"])
                seen_status |= set(value[1]["status"])
            if isinstance(value, list) and len(value) == 3 and all(isinstance(x, int) for x in value):
                seen_err.add(value[2])
    assert seen_ins >= {0, 1, 2, 3, 4, 5, 6, 16, 17, 18, 19}
    assert seen_reg >= {0, 1, 2, 3}
    assert seen_status >= {d.OK, d.TOO_SMALL, d.BAD_MAGIC, d.BAD_DIGEST, d.BAD_SIZE, 8, b.BAD_PARAM, b.WRONG_LENGTH}
    assert d.BAD_CRC not in seen_status and d.NO_CONFIG not in seen_status
    assert seen_err >= {0, b.E_NO_SUCH_CHUNK, b.E_STRANGE_OFFSET, b.ERR_INVALID, b.ERR_NOT_POW2}


def test_chain_orders_differ(oracle):
    """Lengths [98, 80, 89] and [80, 98, 89] of one chunk in one batch: the rule tells them apart."""
    log = dict()
    for name, value in b.expected(oracle, b.case("chain/3-in-3")):
        log.setdefault(name, []).append(value)
    first, second = (u[1]["ins"] for u in log["upload"])
    assert first == [b.INS_NEW, b.INS_REPLACE_BIGGER, b.INS_DUP_KEEP_SMALLER]
    assert second == [b.INS_NEW, b.INS_DUP_KEEP_SMALLER, b.INS_DUP_KEEP_SMALLER]


def test_wrong_stored_crc_is_accepted_here_and_refused_by_verify(pbschunk, oracle):
    """UploadChunk recomputes the CRC (upload_chunk.rs:77-85): a blob with a wrong stored CRC is
    accepted and crc_out is zlib's CRC of its payload; the same blob through VerifyWorker is BAD_CRC."""
    dg, c = b.chunk(9100)
    blob = d._flip(b.plain_blob(c), 10, 5)
    with pbschunk.BackupSession((np.zeros((0, 32), np.uint8), [], []), device=False) as s:
        assert s.create_dynamic() == (0, 1)
        rc, out = s.upload(1, b.rows([dg]), [len(c)], np.frombuffer(blob, np.uint8), [0, len(blob)])
    assert rc == 0 and out["status"][0] == d.OK and out["ins"][0] == b.INS_NEW and out["action"][0] == b.ACT_WRITE
    assert int(out["crc"][0]) == zlib.crc32(c) != int.from_bytes(blob[8:12], "little")
    with pbschunk.VerifyWorker((None, b.rows([dg])), device=False) as w:
        ts, _ = w.plan(b.rows([dg]), [len(c)], 0)
        assert ts.size == 1
        _, status = w.submit(np.frombuffer(blob, np.uint8), [0, len(blob)])
        assert int(status[0]) == d.BAD_CRC
        w.abort_index()


def test_the_alignment_copy_equals_the_index_writer(pbschunk):
    """backup_common.h's copy of check_chunk_alignment (the one a lane runs) is held to
    pbs_fidx_check_chunk_alignment by the mirror == device tests; here the model's own version is
    held to the library's on a grid, so all three agree."""
    import ctypes
    for size, cs in ((4096 * 9 + 100, 4096), (8192, 4096), (100, 64), (64, 64)):
        for end in (0, 1, 63, 64, 100, 4096, 4196, 8192, 4096 * 9, 4096 * 9 + 100, 4096 * 10):
            for ln in (0, 1, 36, 64, 100, 4095, 4096, 4097):
                idx = ctypes.c_size_t(0)
                rc = pbschunk.lib().pbs_fidx_check_chunk_alignment(size, cs, end, ln, ctypes.byref(idx))
                code, want = b.check_chunk_alignment(size, cs, end, ln)
                assert (rc, idx.value if rc == 0 else 0) == (code, want), (size, cs, end, ln)


def test_snapshot_through_the_mirror(pbschunk, oracle):
    """backup_snapshot over a hand-made upload result (what pbs_upload_stream_host returns): the
    close checksum is the client's, the image is the client's .didx, and the written chunks carry
    the computed CRC."""
    chunks = [b.chunk(9200 + i, 100 + i)[1] for i in range(5)]
    chunks.append(chunks[1])                                   # the client marks the repeat as known
    digs = [hashlib.sha256(c).digest() for c in chunks]
    ends = np.cumsum([len(c) for c in chunks]).astype(np.uint64)
    known = np.array([0, 0, 0, 0, 0, 1], dtype=np.uint8)
    blobs = [b.plain_blob(c) if not k else b"" for c, k in zip(chunks, known)]
    image, csum = b.didx_image([int(e) for e in ends], digs)
    up = dict(ends=ends, digests=b.rows(digs), known=known, csum=csum, blobs=np.frombuffer(b"".join(blobs), np.uint8),
              blob_offsets=np.concatenate([[0], np.cumsum([len(x) for x in blobs])]).astype(np.uint64))
    with pbschunk.BackupSession((np.zeros((0, 32), np.uint8), [], []), device=False) as s:
        out = pbschunk.backup_snapshot(s, up, manifest_blob=b.plain_blob(b"{}"))
        assert out["append"] == (0, 6, 0) and out["close"] == (0, 0) and out["finish"] == 0
        assert out["image"] == image
        assert out["written"] == {dg: bl for dg, bl, k in zip(digs, blobs, known) if not k}
        assert out["stat"]["count"] == 5 and out["stat"]["client_duplicates"] == 1 and out["stat"]["logged"] == 1
        assert s.stats()["finished"] == 1 and s.stats()["file_counter"] == 2
