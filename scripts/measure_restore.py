#!/usr/bin/env python3
"""Measurement of the restore path (include/pbs_restore.h) on an MI355X.  In one run, on one box:

  (a) the segment copy kernel: --gib GiB (default 1) in 4 MiB segments, the source of every
      segment 0, 1 and 8 bytes off the destination's 16-byte alignment, beside torch's
      Tensor.copy_ of the same bytes (hipMemcpyAsync, device to device).  1 warm + 5 timed
      calls each, alternating; the host clock around the synchronous call and HIP events.
  (b) pbs_restore_range_device on the device encoder's own blobs (compress on) of the text
      corpus, cut at the 4 MiB average: (i) pbs_blob_decode_inflate_device alone on the blobs
      in index order; (ii) the restore through an index without repeats -- the difference is
      the lookup and the two copies; (iii) the restore through an index that names every chunk
      four times: the decode time stays, the output grows fourfold.  Every status must be OK
      and the output the stream.

One JSON line per part.

    python scripts/measure_restore.py [--gib 1] [--out profiles/restore/restore.jsonl]
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
from measure_encrypt import REPS, GiB, cut, emit, med, text_host  # noqa: E402

SEG = 4 << 20


def timed(torch, f):
    """(host seconds, HIP-event ms) of one synchronous call."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    f()
    b.record()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, a.elapsed_time(b)


def part_a(torch, gib, out):
    nseg = max(1, int(gib * GiB) // SEG)
    n = nseg * SEG
    src = torch.empty(n + 64, dtype=torch.uint8, device="cuda:0")
    dst = torch.empty(n + 64, dtype=torch.uint8, device="cuda:0")
    pbschunk.generate_device(src.data_ptr(), n + 64, pbschunk.GEN_RANDOM, 0x5EED0002, 0)
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    offs = np.arange(nseg, dtype=np.uint64) * SEG
    lens = np.full(nseg, SEG, dtype=np.uint64)
    runs = {"memcpy": lambda: dst[:n].copy_(src[:n])}
    for mis in (0, 1, 8):
        runs[f"segments+{mis}"] = (lambda m: lambda: pbschunk.copy_segments_device(src.data_ptr() + m, dst.data_ptr(), offs,
                                                                                 offs, lens))(mis)
    res = {k: [] for k in runs}
    for i in range(1 + REPS):
        for k, f in runs.items():
            t = timed(torch, f)
            if k != "memcpy":  # (checked on every call: the kernel moved the bytes)
                m = int(k.split("+")[1])
                assert bool(torch.equal(dst[:n], src[m:m + n])), f"{k}: the copy differs from its source"
            if i >= 1:
                res[k].append(t)
    base = med([e for _, e in res["memcpy"]])
    for k, ts in res.items():
        ev, host = med([e for _, e in ts]), med([h for h, _ in ts])
        emit(out, {"part": "a", "what": ("torch Tensor.copy_ (hipMemcpyAsync device to device)" if k == "memcpy" else
                                         f"pbs_copy_segments_device, {nseg} segments of 4 MiB, source {k.split('+')[1]} "
                                         "bytes off the destination's alignment"),
                   "bytes": n, "event_ms": [round(e, 3) for _, e in ts], "event_ms_median": round(ev, 3),
                   "GB_s": round(n / 1e9 / (ev / 1e3), 1), "host_ms_median": round(host * 1e3, 3),
                   "GB_s_host_clock": round(n / 1e9 / host, 1), "of_memcpy": round(base / ev, 3)})
    del src, dst
    torch.cuda.empty_cache()
    pbschunk.restore_release()


def part_b(torch, gib, out):
    n = int(gib * GiB)
    host = text_host(n)
    dev = torch.from_numpy(host).to("cuda:0")
    bounds = cut(torch, dev, n, 4 << 20)
    nchunks = int(bounds.size - 1)
    sizes = np.diff(bounds.astype(np.int64)).astype(np.uint64)
    cap = pbschunk.blob_stream_bound(bounds)
    blobs = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
    offs, _, comp, _ = pbschunk.blob_encode_chunks_device(dev.data_ptr(), n, bounds, blobs.data_ptr(), cap, compress=True)
    digests = pbschunk.digest_chunks_device(dev.data_ptr(), n, bounds)
    assert len({d.tobytes() for d in digests}) == nchunks, "the corpus repeats a chunk"
    outb = torch.empty(4 * n, dtype=torch.uint8, device="cuda:0")

    ts = []
    for i in range(1 + REPS):
        _, lens, _, status, t = pbschunk.blob_decode_inflate_device(blobs.data_ptr(), offs, outb.data_ptr(), n, sizes,
                                                                    expect_digests=digests, sizes_exact=True)
        assert not status.any() and np.array_equal(lens, sizes)
        if i >= 1:
            ts.append(t)
    assert bool(torch.equal(outb[:n], dev)), "the decoded stream differs from the input"
    d_ms = med([t["total_ms"] for t in ts])
    emit(out, {"part": "b-i", "what": "pbs_blob_decode_inflate_device alone, the device encoder's blobs of the text corpus "
                                      "in index order, 4 MiB average",
               "bytes": n, "chunks": nchunks, "compressed_chunks": int(comp.sum()), "blob_bytes": int(offs[-1]),
               "total_ms": [round(t["total_ms"], 3) for t in ts], "total_ms_median": round(d_ms, 3),
               "inflate_ms_median": round(med([t["inflate_ms"] for t in ts]), 3),
               "GB_s": round(n / 1e9 / (d_ms / 1e3), 2)})

    for part, times in (("b-ii", 1), ("b-iii", 4)):
        idx_sizes = np.tile(sizes, times)
        ends = np.cumsum(idx_sizes).astype(np.uint64)
        idx_digests = np.tile(digests, (times, 1))
        ts = []
        for i in range(1 + REPS):
            outb.zero_()
            status, t = pbschunk.restore_range_device((ends, idx_digests), blobs.data_ptr(), offs, digests,
                                                      outb.data_ptr(), 0, None)
            assert not status.any()
            if i >= 1:
                ts.append(t)
        for k in range(times):
            assert bool(torch.equal(outb[k * n:(k + 1) * n], dev)), "the restored stream differs from the input"
        r_ms = med([t["total_ms"] for t in ts])
        stage = {k: round(med([t[k] for t in ts]), 3) for k in ("lookup_ms", "pack_ms", "decode_ms", "scatter_ms")}
        emit(out, {"part": part, "what": f"pbs_restore_range_device of the whole archive, every chunk named {times} time(s)",
                   "out_bytes": int(ends[-1]), "entries": int(ts[0]["entries"]), "unique": int(ts[0]["unique"]),
                   "decoded_bytes": int(ts[0]["decoded_bytes"]), "blob_bytes": int(ts[0]["blob_bytes"]),
                   "total_ms": [round(t["total_ms"], 3) for t in ts], "total_ms_median": round(r_ms, 3), **stage,
                   "inflate_ms_median": round(med([t["decode"]["inflate_ms"] for t in ts]), 3),
                   "over_decode_alone_ms": round(r_ms - d_ms, 3), "GB_s_out": round(int(ends[-1]) / 1e9 / (r_ms / 1e3), 2)})
    del dev, blobs, outb
    torch.cuda.empty_cache()
    pbschunk.blob_encode_release()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--part", choices=("a", "b", "ab"), default="ab")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("measure_restore.py needs a GPU")
    torch.cuda.set_device(0)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "w") if args.out else None
    emit(out, {"device": torch.cuda.get_device_name(0), "build_id": pbschunk.build_id(), "warm": 1, "reps": REPS})
    if "a" in args.part:
        part_a(torch, args.gib, out)
    if "b" in args.part:
        part_b(torch, args.gib, out)


if __name__ == "__main__":
    main()
