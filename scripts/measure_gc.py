#!/usr/bin/env python3
"""Measurement of garbage collection (include/pbs_gc.h) on an MI355X.  In one run, on one box:

  store   2^24 random digests (--store-log2), all chunks.
  index   32 pieces (--pieces) of 2^22 entries (--piece-log2).  About 1 % of a piece's digests are
          absent from the store; piece k keeps about 90 % of piece k - 1's entries in place and
          draws the rest anew, as consecutive snapshots do.

  (a) pbs_gc_begin: the table build (HIP events: memsets + kernel) and the whole call with the
      upload of the listing (host clock), 1 warm + 3 timed.
  (b) the mark of every piece through one handle, the pieces resident on the device one at a
      time: mark_ms (HIP events) per piece, for the first piece alone (no store entry referenced
      yet: every hit stores its byte) and over all pieces.
  (c) pbs_gc_sweep over the store with random sizes and atimes.
  (d) what the parent commit has for membership: pbs_digest_lookup_device of piece 0 against the
      same store (it sorts both lists on every call).  It must report the same missing set.
  (e) the host mirror: pbs_gc_begin_host and pbs_gc_mark_host of piece 0; the same missing list.

One JSON line per part.

    python scripts/measure_gc.py [--out profiles/gc/gc.jsonl]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("proxmox-backup_amd", "oracle", "tests", "scripts", ""):
    sys.path.insert(0, os.path.join(ROOT, sub))

import pbschunk  # noqa: E402
from measure_encrypt import emit, med  # noqa: E402
from measure_restore import timed  # noqa: E402

ABSENT = 0.01
KEEP = 0.90


def draw(rng, store, n):
    """n digests: store entries at random, ABSENT of them replaced by random (absent) digests."""
    rows = store[rng.integers(0, store.shape[0], size=n)]
    gone = np.flatnonzero(rng.random(n) < ABSENT)
    rows[gone] = rng.integers(0, 1 << 63, size=(gone.size, 4), dtype=np.uint64).view(np.uint8).reshape(-1, 32)
    return rows


def next_piece(rng, store, prev):
    out = prev.copy()
    fresh = np.flatnonzero(rng.random(prev.shape[0]) >= KEEP)
    out[fresh] = draw(rng, store, fresh.size)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--store-log2", type=int, default=24)
    ap.add_argument("--piece-log2", type=int, default=22)
    ap.add_argument("--pieces", type=int, default=32)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("measure_gc.py needs a GPU")
    torch.cuda.set_device(0)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "w") if args.out else None
    m, n = 1 << args.store_log2, 1 << args.piece_log2
    emit(out, {"device": torch.cuda.get_device_name(0), "build_id": pbschunk.build_id(), "store_entries": m,
               "piece_entries": n, "pieces": args.pieces, "absent_share": ABSENT, "kept_share": KEEP})
    rng = np.random.default_rng(0x6C)
    store = rng.integers(0, 1 << 63, size=(m, 4), dtype=np.uint64).view(np.uint8).reshape(m, 32)
    listing = (None, store, np.zeros(m, dtype=np.uint8))

    # (a) the table
    builds, calls = [], []
    for i in range(1 + 3):
        t0 = time.perf_counter()
        gc = pbschunk.GarbageCollector(listing)
        dt = time.perf_counter() - t0
        if i >= 1:
            builds.append(gc.build_ms)
            calls.append(dt * 1e3)
        if i < 3:
            gc.close()
    b_ms = med(builds)
    emit(out, {"part": "a", "what": "pbs_gc_begin: table build (HIP events: memsets + kernel); the whole call with the "
                                    "upload of the listing (host clock)",
               "table_log2": gc.table_log2, "build_ms": [round(x, 3) for x in builds], "build_ms_median": round(b_ms, 3),
               "build_entries_per_s": round(m / (b_ms / 1e3)), "call_ms_median": round(med(calls), 1)})

    # (b) the marks
    piece0 = draw(rng, store, n)
    piece, marks, missing0, total_missing = piece0, [], None, 0
    for k in range(args.pieces):
        if k:
            piece = next_piece(rng, store, piece)
        dev = torch.from_numpy(piece).cuda()
        pos, nm = gc.mark(dev.data_ptr(), 32, n, index_bytes=(n << 22) if k == 0 else None)
        marks.append(gc.mark_ms)
        total_missing += nm
        if k == 0:
            missing0 = pos.copy()
        del dev
    all_ms = sum(marks)
    emit(out, {"part": "b", "what": "pbs_gc_mark_device / pbs_gc_mark_piece of every piece through one handle (HIP events)",
               "mark_ms": [round(x, 3) for x in marks], "first_piece_ms": round(marks[0], 3),
               "first_piece_entries_per_s": round(n / (marks[0] / 1e3)), "all_pieces_ms": round(all_ms, 3),
               "all_pieces_entries_per_s": round(n * args.pieces / (all_ms / 1e3)),
               "later_piece_ms_median": round(med(marks[1:]), 3) if len(marks) > 1 else None,
               "missing_first_piece": int(missing0.size), "missing_all": int(total_missing),
               "referenced": int(gc.touched().sum())})

    # (c) the sweep
    sizes = rng.integers(0, 4 << 20, size=m, dtype=np.uint64)
    p1 = 1_700_000_000
    atimes = p1 - rng.integers(0, 200_000, size=m, dtype=np.int64)
    sweeps, scalls = [], []
    for i in range(1 + 3):
        t0 = time.perf_counter()
        actions, status = gc.sweep(sizes, atimes, p1, p1)
        dt = time.perf_counter() - t0
        if i >= 1:
            sweeps.append(gc.sweep_ms)
            scalls.append(dt * 1e3)
    s_ms = med(sweeps)
    emit(out, {"part": "c", "what": "pbs_gc_sweep: touched + classify + reduce (HIP events); the whole call with sizes and "
                                    "atimes up and actions down (host clock)",
               "sweep_ms": [round(x, 3) for x in sweeps], "sweep_ms_median": round(s_ms, 3),
               "sweep_entries_per_s": round(m / (s_ms / 1e3)), "call_ms_median": round(med(scalls), 1), "status": status,
               "removed": int((actions == pbschunk.GC_REMOVE).sum())})
    gc.close()
    pbschunk.gc_release()

    # (d) the lookup call on piece 0
    d_store, d_piece = torch.from_numpy(store).cuda(), torch.from_numpy(piece0).cuda()
    d_pos = torch.empty(n, dtype=torch.int32, device="cuda")
    d_first = torch.empty(n, dtype=torch.int32, device="cuda")
    looks = []
    for i in range(1 + 3):
        res = {}

        def call():
            res["nm"], _ = pbschunk.digest_lookup_device(d_piece.data_ptr(), n, d_store.data_ptr(), m, d_pos.data_ptr(),
                                                         d_first.data_ptr())
        _, ev = timed(torch, call)
        if i >= 1:
            looks.append(ev)
    look_missing = np.flatnonzero(d_pos.cpu().numpy().view(np.uint32) == pbschunk.LOOKUP_MISSING).astype(np.uint32)
    same = bool(np.array_equal(look_missing, missing0)) and res["nm"] == missing0.size
    l_ms = med(looks)
    emit(out, {"part": "d", "what": "pbs_digest_lookup_device of piece 0 against the same store, both resident (HIP events "
                                    "around the call): how the parent commit answers membership",
               "lookup_ms": [round(x, 3) for x in looks], "lookup_ms_median": round(l_ms, 3),
               "lookup_entries_per_s": round(n / (l_ms / 1e3)), "membership_equal": same,
               "lookup_over_first_mark": round(l_ms / marks[0], 2),
               "lookup_over_later_mark": round(l_ms / med(marks[1:]), 2) if len(marks) > 1 else None,
               "pieces_until_build_is_repaid": round(b_ms / max(l_ms - marks[0], 1e-9), 2)})
    del d_store, d_piece, d_pos, d_first
    torch.cuda.empty_cache()
    pbschunk.restore_release()

    # (e) the host mirror
    with pbschunk.GarbageCollector(listing, device=False) as hgc:
        hpos, hnm = hgc.mark(piece0.ctypes.data, 32, n, index_bytes=0)
        emit(out, {"part": "e", "what": "the host mirror (one thread): pbs_gc_begin_host (sort) and pbs_gc_mark_host of piece 0",
                   "build_ms": round(hgc.build_ms, 1), "build_entries_per_s": round(m / (hgc.build_ms / 1e3)),
                   "mark_ms": round(hgc.mark_ms, 1), "mark_entries_per_s": round(n / (hgc.mark_ms / 1e3)),
                   "missing_equal": bool(np.array_equal(hpos, missing0)) and hnm == missing0.size,
                   "host_build_over_device": round(hgc.build_ms / b_ms, 1),
                   "host_mark_over_device_first_piece": round(hgc.mark_ms / marks[0], 1)})
    if not same:
        sys.exit("the lookup call and the mark disagree on the missing set")


if __name__ == "__main__":
    main()
