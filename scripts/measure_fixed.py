#!/usr/bin/env python3
"""Measurement of the fixed-size chunk path (include/pbs_fixed.h) on an MI355X.  In one run:

  (a) the dirty map: pairs of equal images (so every byte of both is read) of --dirty-gib GiB
      each (default 4 and 64), 4 MiB chunks, at base offsets (0, 0) and (1, 8), beside torch's
      Tensor.copy_ of one image onto the other (hipMemcpyAsync, device to device: the same
      2 x size bytes move).  1 warm + 5 timed calls each, alternating; HIP events and the host
      clock around the synchronous call.
  (b) digests and upload of --gib GiB (default 16) of the VM-image generator in 4 MiB chunks
      with 100 %, 10 % and 1 % of the chunks dirty: pbs_fixed_digests_device on the resident
      image; pbs_upload_fixed_host from host memory without a map and with each map, in pieces
      of 1 GiB and of 16 MiB (a piece without a dirty byte is not copied); and
      pbs_upload_stream_host at the 4 MiB average on the same buffer.  The digests of every
      variant are checked against the run without a map.

One JSON line per measurement.

    python scripts/measure_fixed.py [--dirty-gib 4,64] [--gib 16] [--out profiles/fixed/fixed.jsonl]
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
from measure_encrypt import REPS, GiB, emit, med  # noqa: E402
from measure_restore import timed  # noqa: E402

CHUNK = 4 << 20


def part_a(torch, gib, out):
    size = int(gib * GiB)
    n = pbschunk.fidx_count(size, CHUNK)
    prev = torch.empty(size + 64, dtype=torch.uint8, device="cuda:0")
    cur = torch.empty(size + 64, dtype=torch.uint8, device="cuda:0")
    pbschunk.generate_device(prev.data_ptr(), size + 64, pbschunk.GEN_RANDOM, 0x5EED0004, 0)
    cur.copy_(prev)
    flags = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    counts = {}

    def dirty(po, co):
        # (equal images at both offsets: cur[8:] must hold prev[1:])
        def f():
            counts[(po, co)] = pbschunk.fixed_dirty_device(prev.data_ptr() + po, cur.data_ptr() + co, size, CHUNK,
                                                           flags.data_ptr())
        return f

    runs = {"memcpy": lambda: cur[:size].copy_(prev[:size]), "dirty+0+0": dirty(0, 0)}
    res = {k: [] for k in ("memcpy", "dirty+0+0", "dirty+1+8")}
    for i in range(1 + REPS):
        for k, f in runs.items():
            t = timed(torch, f)
            if i >= 1:
                res[k].append(t)
    assert counts[(0, 0)] == 0 and not bool(flags.any()), "equal images have dirty chunks"
    cur[8:8 + size].copy_(prev[1:1 + size])
    for i in range(1 + REPS):
        t = timed(torch, dirty(1, 8))
        if i >= 1:
            res["dirty+1+8"].append(t)
    assert counts[(1, 8)] == 0
    cur[8 + size - 1] ^= 1  # and the kernel does look: the image's last byte
    assert dirty(1, 8)() is None and counts[(1, 8)] == 1 and int(flags[n - 1]) == 1
    base = med([e for _, e in res["memcpy"]])
    for k, ts in res.items():
        ev, host = med([e for _, e in ts]), med([h for h, _ in ts])
        what = ("torch Tensor.copy_ of one image (hipMemcpyAsync device to device)" if k == "memcpy" else
                f"pbs_fixed_dirty_device, equal images, 4 MiB chunks, base offsets ({k.split('+')[1]}, {k.split('+')[2]})")
        emit(out, {"part": "a", "what": what, "image_bytes": size, "bytes_moved": 2 * size, "chunks": n,
                   "event_ms": [round(e, 3) for _, e in ts], "event_ms_median": round(ev, 3),
                   "GB_s_read": round(2 * size / 1e9 / (ev / 1e3), 1), "host_ms_median": round(host * 1e3, 3),
                   "of_memcpy": round(base / ev, 3)})
    del prev, cur, flags
    torch.cuda.empty_cache()


def part_b(torch, gib, out):
    size = int(gib * GiB) // CHUNK * CHUNK
    n = size // CHUNK
    dev = torch.empty(size, dtype=torch.uint8, device="cuda:0")
    pbschunk.generate_device(dev.data_ptr(), size, pbschunk.GEN_VMIMAGE, 0x5EED0003, 0)
    host = dev.cpu().numpy()
    rng = np.random.default_rng(0x6D6170)
    maps = {}
    for pct in (100, 10, 1):
        m = np.zeros(n, dtype=np.uint8)
        m[rng.choice(n, size=max(1, n * pct // 100), replace=False)] = 1
        maps[pct] = m

    # digests of the resident image
    full = None
    for name, m in [("no map", None)] + [(f"{p} % dirty", maps[p]) for p in (100, 10, 1)]:
        ts = []
        for i in range(1 + REPS):
            t0 = time.perf_counter()
            dig, _, t = pbschunk.fixed_digests_device(dev.data_ptr(), size, CHUNK, dirty=m,
                                                      prev_digests=full if m is not None else None)
            t["wall_ms"] = (time.perf_counter() - t0) * 1e3
            if full is None:
                full = dig.copy()
            assert np.array_equal(dig, full), name
            if i >= 1:
                ts.append(t)
        ms = med([t["total_ms"] for t in ts])
        emit(out, {"part": "b-digests", "what": f"pbs_fixed_digests_device, 4 MiB chunks, {name}", "bytes": size, "chunks": n,
                   "hashed_chunks": int(ts[0]["hashed_chunks"]), "hashed_bytes": int(ts[0]["hashed_bytes"]),
                   "total_ms": [round(t["total_ms"], 3) for t in ts], "total_ms_median": round(ms, 3),
                   "gpu_ms_median": round(med([t["gpu_ms"] for t in ts]), 3), "GB_s_image": round(size / 1e9 / (ms / 1e3), 2)})
    del dev
    torch.cuda.empty_cache()
    pbschunk.digest_hybrid_release()

    # upload from host memory: the variants alternate inside each repetition
    blobs = np.empty(12 * (size // (CHUNK >> 2) + 4) + size, dtype=np.uint8)
    big, small = 1 << 30, 4 * CHUNK  # pieces: the default, and one that lets clean pieces stay on the host
    variants = [("pbs_upload_stream_host, 4 MiB average, 1 GiB pieces", None, "stream", big),
                ("pbs_upload_fixed_host, no map, 1 GiB pieces", None, "fixed", big),
                ("pbs_upload_fixed_host, no map, 16 MiB pieces", None, "fixed", small)]
    variants += [(f"pbs_upload_fixed_host, {p} % dirty, 1 GiB pieces", maps[p], "fixed", big) for p in (100, 10, 1)]
    variants += [(f"pbs_upload_fixed_host, {p} % dirty, 16 MiB pieces", maps[p], "fixed", small) for p in (10, 1)]
    res = {v[0]: [] for v in variants}
    for i in range(1 + REPS):
        for what, m, kind, piece in variants:
            t0 = time.perf_counter()
            if kind == "stream":
                o = pbschunk.upload_stream_host(host, CHUNK, piece=piece, blobs_out=blobs)
            else:
                o = pbschunk.upload_fixed_host(host, CHUNK, piece=piece, dirty=m,
                                               prev_digests=full if m is not None else None, blobs_out=blobs)
                assert np.array_equal(o["digests"], full), what
            t = o["timing"]
            t["wall_ms"] = (time.perf_counter() - t0) * 1e3
            t["stats"] = o["stats"]
            if i >= 1:
                res[what].append(t)
    for what, ts in res.items():
        ms = med([t["total_ms"] for t in ts])
        rec = {"part": "b-upload", "what": what, "bytes": size, "chunks": int(ts[0]["chunk_count"]),
               "total_ms": [round(t["total_ms"], 3) for t in ts], "total_ms_median": round(ms, 3),
               "GB_s_image": round(size / 1e9 / (ms / 1e3), 2),
               "h2d_ms_median": round(med([t["pipe"]["h2d_ms"] for t in ts]), 3),
               "drain_ms_median": round(med([t["pipe"]["drain_ms"] for t in ts]), 3),
               "host_chunks": int(ts[0]["pipe"]["host_chunks"]), "gpu_jobs": int(ts[0]["pipe"]["gpu_jobs"]),
               "chunk_reused": int(ts[0]["chunk_reused"]), "size_compressed": int(ts[0]["size_compressed"])}
        if "dirty_chunks" in ts[0]:
            rec["dirty_chunks"], rec["copied_bytes"] = int(ts[0]["dirty_chunks"]), int(ts[0]["copied_bytes"])
        emit(out, rec)
    pbschunk.pipeline_release()
    pbschunk.blob_encode_release()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dirty-gib", default="4,64")
    ap.add_argument("--gib", type=float, default=16.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--part", choices=("a", "b", "ab"), default="ab")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("measure_fixed.py needs a GPU")
    torch.cuda.set_device(0)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "w") if args.out else None
    emit(out, {"device": torch.cuda.get_device_name(0), "build_id": pbschunk.build_id(), "warm": 1, "reps": REPS})
    if "a" in args.part:
        for g in args.dirty_gib.split(","):
            part_a(torch, float(g), out)
    if "b" in args.part:
        part_b(torch, args.gib, out)


if __name__ == "__main__":
    main()
