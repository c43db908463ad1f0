#!/usr/bin/env python3
"""Measurement of the verify job (include/pbs_verify.h) on an MI355X.  Nothing here is a gate.

  a  the load plan (probe, first occurrence, compaction over the store axis) of an index of 2^22
     entries against a store of 2^24, beside pbs_gc_mark_device on the same arrays in the same
     run, alternating; HIP-event times (plan_ms / mark_ms), the uploads outside them.
  b  a whole pbs_verify_index_device over libzstd level-1 blobs of text, pxar-like data and the VM
     image (4 MiB chunks, every chunk distinct: a counter is stamped into each), beside one bare
     pbs_blob_decode_inflate_device on the same packed blobs, alternating; host clock around the
     synchronous calls.  The difference is what verify adds: plan, magic read, pack, states, count.
  c  the same over an all-encrypted store (CRC only; the ciphertext is random bytes: verify
     never opens it).

2 warm + 7 timed calls each; every number is a median with the least and the largest beside it.
One JSON line per part.

    python scripts/measure_verify.py [--gib 0.5] [--log2n 22] [--log2m 24] [--out FILE]
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

CHUNK, DISTINCT, WARM, REPS, THREADS = 4 << 20, 8, 2, 7, 16
COMPRESSED_MAGIC = bytes([49, 185, 88, 66, 111, 182, 163, 127])
ENCRYPTED_MAGIC = bytes([123, 103, 133, 190, 34, 45, 76, 240])


def stat(xs):
    return {"median": float(np.median(xs)), "min": float(np.min(xs)), "max": float(np.max(xs))}


def part_a(torch, emit, log2n, log2m):
    n, m = 1 << log2n, 1 << log2m
    rng = np.random.default_rng(0x766572)
    store = rng.integers(0, 256, size=(m, 32), dtype=np.uint8)
    pick = rng.integers(0, m, size=n)
    index = np.ascontiguousarray(store[pick])
    sizes = np.full(n, CHUNK, dtype=np.uint64)
    d_index = torch.from_numpy(index).cuda()
    plan_ms, mark_ms, todo = [], [], 0
    with pbschunk.VerifyWorker((None, store)) as w, pbschunk.GarbageCollector((None, store, np.zeros(m, np.uint8))) as gc:
        for i in range(WARM + REPS):
            ts, _ = w.plan(index, sizes, pbschunk.VERIFY_MODE_NONE)
            todo = int(ts.size)
            w.abort_index()  # (the states stay UNKNOWN: every plan is the same work)
            _, nm = gc.mark(d_index.data_ptr(), 32, n)
            assert nm == 0 and todo == np.unique(pick).size and bool((np.diff(ts.astype(np.int64)) > 0).all())
            if i >= WARM:
                plan_ms.append(w.plan_ms)
                mark_ms.append(gc.mark_ms)
        build = {"verify_build_ms": w.build_ms, "gc_build_ms": gc.build_ms}
    emit(part="a", what="pbs_verify_plan beside pbs_gc_mark_piece, same store and index, alternating", n=n, m=m,
         todo=todo, plan_ms=stat(plan_ms), gc_mark_ms=stat(mark_ms),
         ratio_of_medians=float(np.median(plan_ms) / np.median(mark_ms)), **build)
    pbschunk.gc_release()
    pbschunk.verify_release()


def sources(gib):
    n = CHUNK * DISTINCT
    reps = max(1, int(gib * (1 << 30)) // n)
    for name, data in (("text", corpus_gen.text(n + (1 << 20), 11)[:n]), ("pxar", corpus_gen.pxar(n + (1 << 20), 12)[:n]),
                       ("vmimage", oracle.gen_vmimage(n, 13))):
        data = np.ascontiguousarray(data)
        chunks = []
        for r in range(reps):
            for i in range(DISTINCT):
                c = bytearray(data[i * CHUNK:(i + 1) * CHUNK].tobytes())
                c[:8] = struct.pack("<Q", r * DISTINCT + i)  # every chunk distinct
                chunks.append(bytes(c))
        yield name, chunks


def compress_all(chunks):
    L = oracle.libzstd()

    def one(c):
        cap = L.ZSTD_compressBound(len(c))
        dst = ctypes.create_string_buffer(cap)
        r = L.ZSTD_compress(dst, cap, c, len(c), 1)
        assert not L.ZSTD_isError(r)
        f = dst.raw[:r]
        return COMPRESSED_MAGIC + struct.pack("<I", zlib.crc32(f)) + f, hashlib.sha256(c).digest()
    with ThreadPoolExecutor(THREADS) as ex:
        return list(ex.map(one, chunks))


def run_store(torch, emit, part, name, blobs, digests, sizes, mode):
    """verify_index_device beside one bare decode call on the same blobs, alternating."""
    m = len(blobs)
    off = np.concatenate([[0], np.cumsum([len(b) for b in blobs])]).astype(np.uint64)
    src = torch.from_numpy(np.frombuffer(b"".join(blobs), np.uint8).copy()).cuda()
    dg = np.frombuffer(b"".join(digests), np.uint8).reshape(-1, 32).copy()
    sz = np.asarray(sizes, np.uint64)
    image, _ = pbschunk.didx_build(np.cumsum(sz), dg)
    enc = mode == pbschunk.VERIFY_MODE_ENCRYPT
    content = int(sz.sum())
    slots = np.zeros(m, np.uint64) if enc else sz
    out = torch.empty(max(1, int(slots.sum())), dtype=torch.uint8, device="cuda")
    v_ms, d_ms = [], []
    for i in range(WARM + REPS):
        with pbschunk.VerifyWorker((None, dg)) as w:  # (a fresh worker: every chunk is UNKNOWN again)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res, cs, mp = w.verify_index(image, mode, store=(src.data_ptr(), off))
            t1 = time.perf_counter()
        assert res["ok"] == 1 and res["loaded"] == m and res["decoded_bytes"] == content, res
        t2 = time.perf_counter()
        _, _, _, status, t = pbschunk.blob_decode_inflate_device(src.data_ptr(), off, out.data_ptr(), int(slots.sum()), slots,
                                                                 expect_digests=dg, sizes_exact=True)
        t3 = time.perf_counter()
        assert (status == (pbschunk.BLOB_ST_NO_CONFIG if enc else 0)).all()
        if i >= WARM:
            v_ms.append((t1 - t0) * 1e3)
            d_ms.append((t3 - t2) * 1e3)
    vm, dm = float(np.median(v_ms)), float(np.median(d_ms))
    emit(part=part, source=name, chunks=m, blob_bytes=int(off[-1]), content_bytes=content, verify_index_ms=stat(v_ms),
         bare_decode_ms=stat(d_ms), verify_adds_ms=vm - dm, verify_gb_s_content=content / vm / 1e6,
         verify_gb_s_read=int(off[-1]) / vm / 1e6, bare_gb_s_content=content / dm / 1e6)
    del src, out


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
    emit(part="setup", device=torch.cuda.get_device_name(0), build_id=pbschunk.build_id() if hasattr(pbschunk, "build_id") else None,
         warm=WARM, reps=REPS, gib=a.gib)
    if "a" in a.parts:
        part_a(torch, emit, a.log2n, a.log2m)
    if "b" in a.parts:
        for name, chunks in sources(a.gib):
            packed = compress_all(chunks)
            run_store(torch, emit, "b", name, [p[0] for p in packed], [p[1] for p in packed], [len(c) for c in chunks],
                      pbschunk.VERIFY_MODE_NONE)
    if "c" in a.parts:
        rng = np.random.default_rng(0x656E63)
        m = max(1, int(a.gib * (1 << 30)) // CHUNK)
        blobs, digests = [], []
        for k in range(m):
            ct = rng.bytes(CHUNK)
            blobs.append(ENCRYPTED_MAGIC + struct.pack("<I", zlib.crc32(ct)) + rng.bytes(32) + ct)
            digests.append(rng.bytes(32))  # (the digest of an encrypted chunk is not checked without the key)
        run_store(torch, emit, "c", "all-encrypted (random ciphertext)", blobs, digests, [CHUNK] * m, pbschunk.VERIFY_MODE_ENCRYPT)
    pbschunk.verify_release()
    pbschunk.blob_encode_release()


if __name__ == "__main__":
    main()
