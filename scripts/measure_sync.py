#!/usr/bin/env python3
"""Measurement of the sync job (include/pbs_sync.h) on an MI355X.  Nothing here is a gate.

  a  pbs_sync_plan of a piece of 2^22 entries against a store of 2^24, with no repeats and a share
     of new digests of 0, 1 %, 50 % and 100 %, then with half the entries repeating the other half
     (all listed); beside pbs_gc_mark_piece of the same piece on a table of the same listing in
     the same run, alternating.  The worker is begun afresh for every call (reserve = n, so no
     plan grows the table, and every plan inserts the same digests); HIP-event times (plan_ms /
     mark_ms), the uploads outside them.
  b  the same all-listed piece on a worker begun with reserve = 0, so the plan rebuilds the table
     first (plan_ms includes it), beside the plan that does not, and pbs_gc_begin's build of the
     same listing.
  c  pbs_sync_submit of every blob of a store in one call beside pbs_verify_submit of the same
     blobs in the same run, alternating, on the stores of scripts/measure_verify.py (libzstd
     level-1 blobs of text, pxar-like data and the VM image, 4 MiB chunks); host clock around the
     synchronous calls.  Both are the same decode; the difference is the state kernel.

2 warm + 7 timed calls each; every number is a median with the least and the largest beside it.
One JSON line per part.

    python scripts/measure_sync.py [--gib 0.5] [--log2n 22] [--log2m 24] [--out FILE]
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

import measure_verify as mv  # noqa: E402  (the stores of part c, and stat)
import pbschunk  # noqa: E402

WARM, REPS = mv.WARM, mv.REPS


def part_a(torch, emit, log2n, log2m, with_rebuild):
    n, m = 1 << log2n, 1 << log2m
    rng = np.random.default_rng(0x73796E63)
    store = rng.integers(0, 256, size=(m, 32), dtype=np.uint8)
    listed = np.ascontiguousarray(store[rng.permutation(m)[:n]])  # n distinct listed digests
    fresh = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    sizes = np.full(n, 4 << 20, dtype=np.uint64)
    mixes = []
    for share in (0.0, 0.01, 0.5, 1.0):
        k = int(n * share)
        rows = np.concatenate([fresh[:k], listed[k:]])
        mixes.append((f"new {share:g}", np.ascontiguousarray(rows[rng.permutation(n)]), k, n - k, 0))
    half = listed[:n // 2]
    rows = np.concatenate([half, half])
    mixes.append(("repeats 0.5", np.ascontiguousarray(rows[rng.permutation(n)]), 0, n // 2, n // 2))
    with pbschunk.GarbageCollector((None, store, np.zeros(m, np.uint8))) as gc:
        for name, index, want_new, want_touch, want_dup in mixes:
            d_index = torch.from_numpy(index).cuda()
            plan_ms, mark_ms, L = [], [], 0
            for i in range(WARM + REPS):
                with pbschunk.SyncWorker((None, store), reserve=n) as w:
                    vd, fs, fe, ts = w.plan(index, sizes)
                    assert (fs.size, ts.size, int((vd == pbschunk.SYNC_DUP).sum())) == (want_new, want_touch, want_dup)
                    assert w.count == m + want_new
                    ms, L = w.plan_ms, w.table_log2
                _, nm = gc.mark(d_index.data_ptr(), 32, n)
                assert nm == want_new
                if i >= WARM:
                    plan_ms.append(ms)
                    mark_ms.append(gc.mark_ms)
            emit(part="a", what="pbs_sync_plan beside pbs_gc_mark_piece, same listing and piece, alternating", mix=name,
                 n=n, m=m, table_log2=L, gc_table_log2=int(pbschunk.lib().pbs_gc_table_log2(gc._h)),
                 fetch=want_new, touch=want_touch, dup=want_dup, plan_ms=mv.stat(plan_ms), gc_mark_ms=mv.stat(mark_ms),
                 ratio_of_medians=float(np.median(plan_ms) / np.median(mark_ms)))
            del d_index
        if with_rebuild:
            index = mixes[0][1]
            grow_ms, flat_ms, sync_build, L0, L1 = [], [], [], 0, 0
            for i in range(WARM + REPS):
                with pbschunk.SyncWorker((None, store), reserve=0) as w:
                    L0 = w.table_log2
                    w.plan(index, sizes)
                    g, L1, b = w.plan_ms, w.table_log2, w.build_ms
                with pbschunk.SyncWorker((None, store), reserve=n) as w:
                    w.plan(index, sizes)
                    f = w.plan_ms
                if i >= WARM:
                    grow_ms.append(g)
                    flat_ms.append(f)
                    sync_build.append(b)
            emit(part="b", what="a plan that rebuilds the table first beside one that does not; the builds of the begin calls",
                 n=n, m=m, log2_before=L0, log2_after=L1, plan_with_rebuild_ms=mv.stat(grow_ms), plan_ms=mv.stat(flat_ms),
                 rebuild_ms=float(np.median(grow_ms) - np.median(flat_ms)), sync_begin_build_ms=mv.stat(sync_build),
                 gc_begin_build_ms=gc.build_ms)
    pbschunk.gc_release()
    pbschunk.sync_release()


def run_store(torch, emit, name, blobs, digests, sizes):
    """pbs_sync_submit beside pbs_verify_submit on the same blobs, alternating."""
    m = len(blobs)
    off = np.concatenate([[0], np.cumsum([len(b) for b in blobs])]).astype(np.uint64)
    src = torch.from_numpy(np.frombuffer(b"".join(blobs), np.uint8).copy()).cuda()
    dg = np.frombuffer(b"".join(digests), np.uint8).reshape(-1, 32).copy()
    sz = np.asarray(sizes, np.uint64)
    s_ms, v_ms, s_state, v_state = [], [], [], []
    for i in range(WARM + REPS):
        with pbschunk.SyncWorker((None, np.zeros((0, 32), np.uint8)), reserve=m) as w:
            _, fs, fe, _ = w.plan(dg, sz)
            assert list(fe) == list(range(m))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, status = w.submit(src.data_ptr(), off)
            t1 = time.perf_counter()
            res = w.finish()
            st = w.timing["state_ms"]
        assert res["ok"] == 1 and res["inserted"] == m and (status == 0).all(), res
        with pbschunk.VerifyWorker((None, dg)) as vw:
            ts, _ = vw.plan(dg, sz, pbschunk.VERIFY_MODE_NONE)
            assert list(ts) == list(range(m))
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            _, status = vw.submit(src.data_ptr(), off)
            t3 = time.perf_counter()
            vres, _, _ = vw.finish(m)
            vst = vw.timing["state_ms"]
        assert vres["ok"] == 1 and (status == 0).all(), vres
        if i >= WARM:
            s_ms.append((t1 - t0) * 1e3)
            v_ms.append((t3 - t2) * 1e3)
            s_state.append(st)
            v_state.append(vst)
    sm, vm = float(np.median(s_ms)), float(np.median(v_ms))
    emit(part="c", source=name, chunks=m, blob_bytes=int(off[-1]), content_bytes=int(sz.sum()), sync_submit_ms=mv.stat(s_ms),
         verify_submit_ms=mv.stat(v_ms), ratio_of_medians=sm / vm, sync_state_kernel_ms=mv.stat(s_state),
         verify_state_kernel_ms=mv.stat(v_state), sync_gb_s_content=int(sz.sum()) / sm / 1e6)
    del src


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=0.5)
    ap.add_argument("--log2n", type=int, default=22)
    ap.add_argument("--log2m", type=int, default=24)
    ap.add_argument("--parts", default="abc")
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
    if "a" in a.parts or "b" in a.parts:
        part_a(torch, emit, a.log2n, a.log2m, "b" in a.parts)
    if "c" in a.parts:
        for name, chunks in mv.sources(a.gib):
            packed = mv.compress_all(chunks)
            run_store(torch, emit, name, [p[0] for p in packed], [p[1] for p in packed], [len(c) for c in chunks])
    pbschunk.sync_release()
    pbschunk.verify_release()
    pbschunk.blob_encode_release()


if __name__ == "__main__":
    main()
