"""The backup session on the GPU (include/pbs_backup.h): the device handle must equal the host
mirror and the model of the reference exactly -- status, crc_out, ins, action, is_duplicate,
compressed_size, reg and first_failed per upload, the listing with present / size / kind / known /
known_size, the entry count and the table's L, n_done and err of the appends, the close results,
images and statistics -- on the planted cases of tests/bplanted.py, on sizes that fill many
workgroups against the mirror, and end to end behind pbs_upload_stream_host."""
import zlib

import numpy as np
import pytest

import bplanted as b
import dplanted as d

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_dev(gpu):
    import torch

    torch.cuda.set_device(0)
    yield torch
    gpu.backup_release()
    gpu.restore_release()
    gpu.blob_encode_release()


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


@pytest.mark.parametrize("label", [c[0] for c in b.cases()])
def test_device_equals_the_model_and_the_mirror(gpu, oracle, torch_dev, label):
    c = b.case(label)
    want = b.expected(oracle, c)
    for device in (True, False):
        s = b.Session(gpu, c[1], c[2], device=device, upload=_uploader(torch_dev) if device else None)
        try:
            got = b.run(oracle, c, s)
        finally:
            s.close()
        assert b.diff(got, want) == [], "device" if device else "mirror"


def _pair(gpu, torch, listing, reserve=0):
    lst = (b.rows([x[0] for x in listing]), [x[1] for x in listing], [x[2] for x in listing])
    return gpu.BackupSession(lst, reserve=reserve), gpu.BackupSession(lst, reserve=reserve, device=False)


def _same_state(w, hw):
    assert (w.count, w.table_log2) == (hw.count, hw.table_log2)
    a, h = w.listing(), hw.listing()
    for k in a:
        assert np.array_equal(a[k], h[k]), (k, np.flatnonzero((a[k] != h[k]).reshape(a[k].shape[0], -1).any(axis=1))[:4])


def test_many_workgroups_register_and_append(gpu, torch_dev):
    """register_previous of 2^16 digests (a quarter repeat, some are listed) and three appends of
    2^18 entries on one writer, the last with an unknown chunk and a strange offset planted deep
    inside: everything against the mirror."""
    rng = np.random.default_rng(0x626B31)
    n, m = 1 << 16, 1 << 18
    store = rng.integers(0, 256, (1000, 32), dtype=np.uint8)
    digs = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    digs[n // 2:n // 2 + n // 4] = digs[rng.integers(0, n // 2, n // 4)]
    digs[5:905] = store[:900]
    sizes = rng.integers(1, 1 << 22, n, dtype=np.uint32)
    listing = [(store[j].tobytes(), 100 + j, j % 4) for j in range(1000)]
    w, hw = _pair(gpu, torch_dev, listing)
    with w, hw:
        assert w.register_previous(digs, sizes) == hw.register_previous(digs, sizes) == 0
        _same_state(w, hw)
        last = {}
        for i in range(n):
            last[digs[i].tobytes()] = i                                    # the highest i wins
        final = sizes[[last[digs[i].tobytes()] for i in range(n)]].astype(np.uint64)
        assert w.create_dynamic() == hw.create_dynamic() == (0, 1)
        start = 0
        for step in range(3):
            idx = rng.integers(0, n, m)
            pick, lens = digs[idx], final[idx]
            offs = start + np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
            if step == 2:
                pick[200000] = rng.integers(0, 256, 32, dtype=np.uint8)   # NO_SUCH_CHUNK
                offs[150001] += 1                                          # the lowest wins
                pick[150001 + 300] = store[950]                            # listed, never registered
            got, want = w.dynamic_append(1, pick, offs), hw.dynamic_append(1, pick, offs)
            assert got == want == ((0, m, 0) if step < 2 else (0, 150001, b.E_STRANGE_OFFSET)), step
            start += int(lens.sum())
        total = 2 * m + 150001
        bad = bytes(32)
        assert w.dynamic_close(1, total, 1, bad)[:2] == hw.dynamic_close(1, total, 1, bad)[:2] == (0, b.E_SIZE)


def test_many_workgroups_upload(gpu, torch_dev):
    """An upload of 2^16 encrypted 45-byte blobs, a quarter of them repeating digests (and some of
    those with another length, so the first stays), against the mirror."""
    rng = np.random.default_rng(0x626B32)
    k = 1 << 16
    digs = rng.integers(0, 256, (k, 32), dtype=np.uint8)
    rep = rng.integers(0, k // 2, k // 4)
    digs[k // 2:k // 2 + k // 4] = digs[rep]
    lens = np.full(k, 45, dtype=np.uint64)
    lens[k // 2:k // 2 + k // 8] = 46
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    raw = rng.integers(0, 256, int(off[-1]), dtype=np.uint8)
    for t in range(k):
        kind = 2 + (t & 1) if t < k // 2 else 2 if t < k // 2 + k // 8 else 3
        raw[int(off[t]):int(off[t]) + 8] = np.frombuffer(d.MAGICS[kind], np.uint8)
    sizes = rng.integers(1, 1 << 22, k, dtype=np.uint32)
    w, hw = _pair(gpu, torch_dev, [], reserve=10)
    with w, hw:
        assert w.create_fixed(1 << 40, 1 << 22) == hw.create_fixed(1 << 40, 1 << 22) == (0, 1)
        ptr, keep = _uploader(torch_dev)(raw)
        got, want = w.upload(1, digs, sizes, ptr, off), hw.upload(1, digs, sizes, raw, off)
        del keep
        assert got[0] == want[0] == 0
        for name in want[1]:
            assert np.array_equal(got[1][name], want[1][name]), name
        assert set(np.unique(want[1]["ins"])) >= {b.INS_NEW, b.INS_DUP_SAME, b.INS_DUP_KEEP_FIRST, b.INS_ERR_ENC_UNCOMPRESSED}
        assert set(np.unique(want[1]["reg"])) == {b.REG_NONE, b.REG_OK, b.REG_ERR_MULTI_SMALL}
        t = int(rng.integers(0, k))
        assert int(want[1]["crc"][t]) == zlib.crc32(raw[int(off[t]) + 44:int(off[t + 1])].tobytes())
        _same_state(w, hw)


def test_wrong_stored_crc_on_the_device(gpu, torch_dev):
    """The decode path's internal mode: the CRC is computed and not judged; the public decode call
    on the same blob still says BAD_CRC."""
    dg, c = b.chunk(9100)
    blob = np.frombuffer(d._flip(b.plain_blob(c), 10, 5), np.uint8)
    ptr, keep = _uploader(torch_dev)(blob)
    with gpu.BackupSession((np.zeros((0, 32), np.uint8), [], [])) as s:
        assert s.create_dynamic() == (0, 1)
        rc, out = s.upload(1, b.rows([dg]), [len(c)], ptr, [0, blob.size])
    assert rc == 0 and out["status"][0] == d.OK and out["action"][0] == b.ACT_WRITE
    assert int(out["crc"][0]) == zlib.crc32(c)
    with gpu.VerifyWorker((None, b.rows([dg]))) as w:
        ts, _ = w.plan(b.rows([dg]), [len(c)], 0)
        _, status = w.submit(ptr, [0, blob.size])
        assert ts.size == 1 and int(status[0]) == d.BAD_CRC
        w.abort_index()
    del keep


def test_end_to_end_behind_the_upload_path(gpu, oracle, torch_dev):
    """The blobs and the index pbs_upload_stream_host produces for a small stream go through a
    session: the close checksum is the client's, and the written store plus the image restore the
    stream with pbs_restore_range_device."""
    import corpus_gen

    torch = torch_dev
    data = np.concatenate([corpus_gen.text(300000, 11), np.random.default_rng(5).integers(0, 256, 200000, dtype=np.uint8),
                           corpus_gen.text(300000, 11)[:150000]])
    up = gpu.upload_stream_host(data, 16384)
    assert up["ends"].size > 8
    with gpu.BackupSession((np.zeros((0, 32), np.uint8), [], []), reserve=up["ends"].size) as s:
        out = gpu.backup_snapshot(s, up, upload=_uploader(torch), manifest_blob=b.plain_blob(b"{}"))
        assert out["upload"]["first_failed"] == b.NONE
        assert out["append"] == (0, up["ends"].size, 0) and out["close"] == (0, 0) and out["finish"] == 0
        assert out["image"] == bytes(up["didx"])
        lst = s.listing()
        assert lst["present"].all() and lst["known"].all() and s.count == len(out["written"])
    store_digs = list(out["written"])
    blobs = [out["written"][dg] for dg in store_digs]
    off = np.concatenate([[0], np.cumsum([len(x) for x in blobs])]).astype(np.uint64)
    ptr, keep = _uploader(torch)(np.frombuffer(b"".join(blobs), np.uint8))
    dst = torch.zeros(data.size, dtype=torch.uint8, device="cuda")
    status, _ = gpu.restore_range_device((up["ends"], up["digests"]), ptr, off, b.rows(store_digs), dst.data_ptr())
    assert (status == d.OK).all()
    assert np.array_equal(dst.cpu().numpy(), data)
    del keep
