#!/usr/bin/env python3
"""Measurement of the zstd inflater (pbs_zstd_inflate_device) and of the finished read path
(pbs_blob_decode_inflate_device) on an MI355X: libzstd level-1 frames of text, pxar-like data
and the VM image, one frame per 4 MiB chunk, 2 warm + 5 timed calls, HIP-event times.  The
yardstick, in the same run on the same box: ZSTD_decompress on 16 threads over the same frames
in host memory.  Each source is 8 distinct chunks, repeated to the requested content size.

One JSON line per source and part.

    python scripts/measure_inflate.py [--gib 4] [--out FILE]
"""
import argparse
import ctypes
import hashlib
import json
import os
import struct
import sys
import time
import zlib
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("proxmox-backup_amd", "oracle", "tests", ""):
    sys.path.insert(0, os.path.join(ROOT, sub))

import corpus_gen  # noqa: E402
import oracle  # noqa: E402
import pbschunk  # noqa: E402

CHUNK, DISTINCT, WARM, REPS, THREADS = 4 << 20, 8, 2, 5, 16
COMPRESSED_MAGIC = bytes([49, 185, 88, 66, 111, 182, 163, 127])


def med(xs):
    return float(np.median(xs))


def sources():
    n = CHUNK * DISTINCT
    yield "text", corpus_gen.text(n + (1 << 20), 11)[:n]
    yield "pxar", corpus_gen.pxar(n + (1 << 20), 12)[:n]
    yield "vmimage", oracle.gen_vmimage(n, 13)


def compress_all(chunks):
    L = oracle.libzstd()

    def one(c):
        cap = L.ZSTD_compressBound(len(c))
        dst = ctypes.create_string_buffer(cap)
        r = L.ZSTD_compress(dst, cap, c, len(c), 1)
        assert not L.ZSTD_isError(r)
        return dst.raw[:r]
    with ThreadPoolExecutor(THREADS) as ex:
        return list(ex.map(one, chunks))


def cpu_yardstick(frames, sizes):
    L = oracle.libzstd()
    srcs = [np.frombuffer(f, np.uint8) for f in frames]
    dsts = [np.empty(s, np.uint8) for s in sizes]

    def one(i):
        r = L.ZSTD_decompress(dsts[i].ctypes.data, dsts[i].size, srcs[i].ctypes.data, srcs[i].size)
        assert r == sizes[i]
    ts = []
    with ThreadPoolExecutor(THREADS) as ex:
        for i in range(1 + 3):
            t0 = time.perf_counter()
            list(ex.map(one, range(len(frames))))
            if i:
                ts.append(time.perf_counter() - t0)
    return med(ts)


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    torch.cuda.set_device(0)
    for name, data in sources():
        data = np.ascontiguousarray(data)
        chunks = [data[i * CHUNK:(i + 1) * CHUNK].tobytes() for i in range(data.size // CHUNK)]
        reps = max(1, int(a.gib * (1 << 30)) // (CHUNK * len(chunks)))
        frames = compress_all(chunks) * reps
        sizes = [len(c) for c in chunks] * reps
        digests = [hashlib.sha256(c).digest() for c in chunks] * reps
        content = sum(sizes)
        foff = np.concatenate([[0], np.cumsum([len(f) for f in frames])]).astype(np.uint64)
        ooff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
        src = torch.from_numpy(np.frombuffer(b"".join(frames), np.uint8).copy()).cuda()
        out = torch.empty(content, dtype=torch.uint8, device="cuda")
        ts = []
        for i in range(WARM + REPS):
            lens, status, t = pbschunk.zstd_inflate_device(src.data_ptr(), foff, out.data_ptr(), ooff)
            assert not status.any() and [int(x) for x in lens] == sizes
            if i >= WARM:
                ts.append(t["inflate_ms"])
        first = out[:CHUNK].cpu().numpy().tobytes()
        assert first == chunks[0], "the inflated bytes differ"
        ms = med(ts)
        cpu_s = cpu_yardstick(frames, sizes)
        emit(part="inflate", source=name, frames=len(frames), content_bytes=content, frame_bytes=int(foff[-1]),
             inflate_ms=ms, gpu_gb_s=content / ms / 1e6, workgroups=t["workgroups"], per_workgroup_mb_s=content / ms / 1e3 / t["workgroups"],
             cpu16_s=cpu_s, cpu16_gb_s=content / cpu_s / 1e9, libzstd=int(oracle.libzstd().ZSTD_versionNumber()))
        blobs = [COMPRESSED_MAGIC + struct.pack("<I", zlib.crc32(f)) + f for f in frames]
        boff = np.concatenate([[0], np.cumsum([len(b) for b in blobs])]).astype(np.uint64)
        bsrc = torch.from_numpy(np.frombuffer(b"".join(blobs), np.uint8).copy()).cuda()
        for with_digests in (False, True):
            dg = np.frombuffer(b"".join(digests), np.uint8) if with_digests else None
            tt = []
            for i in range(WARM + REPS):
                oo, lens, kinds, status, t = pbschunk.blob_decode_inflate_device(
                    bsrc.data_ptr(), boff, out.data_ptr(), content, np.array(sizes, np.uint64), expect_digests=dg,
                    sizes_exact=True)
                assert not status.any()
                if i >= WARM:
                    tt.append(t)
            emit(part="decode_inflate", source=name, digests=with_digests, total_ms=med([t["total_ms"] for t in tt]),
                 inflate_ms=med([t["inflate_ms"] for t in tt]), crc_ms=med([t["crc_ms"] for t in tt]),
                 digest_ms=med([t["digest_ms"] for t in tt]),
                 gb_s=content / med([t["total_ms"] for t in tt]) / 1e6)
        del src, out, bsrc
    pbschunk.blob_encode_release()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
