#!/usr/bin/env python3
"""Measurement of the backup session (include/pbs_backup.h) on an MI355X.  Nothing here is a gate.

  a  pbs_backup_dynamic_append of 2^22 entries against 2^24 known chunks (a listing of 2^24, all
     registered) beside pbs_gc_mark_piece of the same piece on a table of the same listing in the
     same run, alternating; HIP-event times (the append's ms / mark_ms), the uploads outside them.
     Expected: within 2x the mark (the mark's probe plus a 4-byte gather, a scan and a reduction).
  b  pbs_backup_upload of every blob of a store in one call beside pbs_verify_submit of the same
     blobs in the same run, alternating, on the stores of scripts/measure_verify.py; host clock
     around the synchronous calls.  Expected: within 1.05x on the unencrypted sets.  The
     session's own share (claim, sort, walk, register: insert_ms) is reported beside it.
  c  pbs_backup_register_previous of 2^22 digests (all new) beside pbs_sync_plan of the same list
     on a worker of the same listing, alternating; HIP-event times.
  d  the table build of pbs_backup_begin beside pbs_sync_begin's over the same listing.

2 warm + 7 timed calls each; every number is a median with the least and the largest beside it.
One JSON line per part.

    python scripts/measure_backup.py [--gib 0.5] [--log2n 22] [--log2m 24] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("proxmox-backup_amd", "oracle", "tests", "scripts", ""):
    sys.path.insert(0, os.path.join(ROOT, sub))

import measure_verify as mv  # noqa: E402  (the stores of part b, and stat)
import pbschunk  # noqa: E402

WARM, REPS = mv.WARM, mv.REPS


def part_acd(torch, emit, log2n, log2m, parts):
    n, m = 1 << log2n, 1 << log2m
    rng = np.random.default_rng(0x626B7570)
    store = rng.integers(0, 256, size=(m, 32), dtype=np.uint8)
    lsize, lkind = np.full(m, 4 << 20, np.uint64), np.zeros(m, np.uint8)
    if "d" in parts:
        b_ms, s_ms = [], []
        for i in range(WARM + REPS):
            with pbschunk.BackupSession((store, lsize, lkind)) as s:
                b = s.build_ms
            with pbschunk.SyncWorker((None, store)) as w:
                sb = w.build_ms
            if i >= WARM:
                b_ms.append(b)
                s_ms.append(sb)
        emit(part="d", what="the table build of pbs_backup_begin beside pbs_sync_begin's, same listing", m=m,
             backup_build_ms=mv.stat(b_ms), sync_build_ms=mv.stat(s_ms), ratio_of_medians=float(np.median(b_ms) / np.median(s_ms)))
    if "c" in parts:
        fresh = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
        r_ms, p_ms = [], []
        for i in range(WARM + REPS):
            with pbschunk.BackupSession((store, lsize, lkind), reserve=n) as s:
                assert s.register_previous(fresh, np.full(n, 4096, np.uint32)) == 0 and s.count == m + n
                r = s.ms
            with pbschunk.SyncWorker((None, store), reserve=n) as w:
                w.plan(fresh, np.full(n, 4096, np.uint64))
                assert w.count == m + n
                p = w.plan_ms
            if i >= WARM:
                r_ms.append(r)
                p_ms.append(p)
        emit(part="c", what="pbs_backup_register_previous beside pbs_sync_plan, same listing and list (all new), alternating",
             n=n, m=m, register_ms=mv.stat(r_ms), sync_plan_ms=mv.stat(p_ms),
             ratio_of_medians=float(np.median(r_ms) / np.median(p_ms)))
        del fresh
    if "a" in parts:
        pick = rng.permutation(m)[:n]
        piece = np.ascontiguousarray(store[pick])
        ksize = rng.integers(1, 1 << 22, m, dtype=np.uint32)
        lens = ksize[pick].astype(np.uint64)
        offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
        d_piece = torch.from_numpy(piece).cuda()
        a_ms, g_ms = [], []
        with pbschunk.BackupSession((store, lsize, lkind)) as s, \
                pbschunk.GarbageCollector((None, store, np.zeros(m, np.uint8))) as gc:
            assert s.register_previous(store, ksize) == 0 and s.count == m
            reg_ms = s.ms
            for i in range(WARM + REPS):
                rc, wid = s.create_dynamic()
                assert rc == 0
                assert s.dynamic_append(wid, piece, offs) == (0, n, 0)
                a = s.ms
                s.dynamic_close(wid, 0, 0, bytes(32))  # (drops the writer and its entries)
                _, nm = gc.mark(d_piece.data_ptr(), 32, n)
                assert nm == 0
                if i >= WARM:
                    a_ms.append(a)
                    g_ms.append(gc.mark_ms)
        emit(part="a", what="pbs_backup_dynamic_append beside pbs_gc_mark_piece, same listing and piece, alternating", n=n,
             m=m, append_ms=mv.stat(a_ms), gc_mark_ms=mv.stat(g_ms), ratio_of_medians=float(np.median(a_ms) / np.median(g_ms)),
             expected="<= 2", register_all_ms=reg_ms)
        del d_piece
    pbschunk.gc_release()
    pbschunk.sync_release()
    pbschunk.backup_release()


def run_store(torch, emit, name, blobs, digests, sizes):
    """pbs_backup_upload beside pbs_verify_submit on the same blobs, alternating."""
    m = len(blobs)
    off = np.concatenate([[0], np.cumsum([len(b) for b in blobs])]).astype(np.uint64)
    src = torch.from_numpy(np.frombuffer(b"".join(blobs), np.uint8).copy()).cuda()
    dg = np.frombuffer(b"".join(digests), np.uint8).reshape(-1, 32).copy()
    sz = np.asarray(sizes, np.uint64)
    u_ms, v_ms, ins_ms, dec_ms = [], [], [], []
    empty = (np.zeros((0, 32), np.uint8), [], [])
    for i in range(WARM + REPS):
        with pbschunk.BackupSession(empty, reserve=m) as s:
            rc, wid = s.create_dynamic()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rc, out = s.upload(wid, dg, sz.astype(np.uint32), src.data_ptr(), off)
            t1 = time.perf_counter()
            tm = s.timing
        assert rc == 0 and out["first_failed"] == pbschunk.BACKUP_NONE and (out["ins"] == pbschunk.BACKUP_INS_NEW).all()
        with pbschunk.VerifyWorker((None, dg)) as vw:
            ts, _ = vw.plan(dg, sz, pbschunk.VERIFY_MODE_NONE)
            assert list(ts) == list(range(m))
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            _, status = vw.submit(src.data_ptr(), off)
            t3 = time.perf_counter()
            vres, _, _ = vw.finish(m)
        assert vres["ok"] == 1 and (status == 0).all(), vres
        if i >= WARM:
            u_ms.append((t1 - t0) * 1e3)
            v_ms.append((t3 - t2) * 1e3)
            ins_ms.append(tm["insert_ms"])
            dec_ms.append(tm["decode_ms"])
    um, vm = float(np.median(u_ms)), float(np.median(v_ms))
    emit(part="b", source=name, chunks=m, blob_bytes=int(off[-1]), content_bytes=int(sz.sum()), upload_ms=mv.stat(u_ms),
         verify_submit_ms=mv.stat(v_ms), ratio_of_medians=um / vm, expected="<= 1.05", insert_kernels_ms=mv.stat(ins_ms),
         decode_calls_ms=mv.stat(dec_ms), upload_gb_s_content=int(sz.sum()) / um / 1e6)
    del src


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=0.5)
    ap.add_argument("--log2n", type=int, default=22)
    ap.add_argument("--log2m", type=int, default=24)
    ap.add_argument("--parts", default="abcd")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    torch.cuda.set_device(0)
    emit(part="setup", device=torch.cuda.get_device_name(0), build_id=pbschunk.build_id(), warm=WARM, reps=REPS, gib=a.gib)
    if set("acd") & set(a.parts):
        part_acd(torch, emit, a.log2n, a.log2m, a.parts)
    if "b" in a.parts:
        for name, chunks in mv.sources(a.gib):
            packed = mv.compress_all(chunks)
            run_store(torch, emit, name, [p[0] for p in packed], [p[1] for p in packed], [len(c) for c in chunks])
    pbschunk.backup_release()
    pbschunk.verify_release()
    pbschunk.blob_encode_release()


if __name__ == "__main__":
    main()
