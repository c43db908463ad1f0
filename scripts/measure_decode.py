#!/usr/bin/env python3
"""Measurement of the read side (pbs_blob_decode_device) on an MI355X, at the shape of
measure_encrypt.py's part (a): a device-resident random stream cut at the 4 MiB average,
compress off, 2 warm + 5 timed calls, HIP-event times.  In one run, on one box:

  (i)   encrypt_ms of the existing encrypted encode, which makes the blobs -- the yardstick;
  (ii)  decrypt_ms and total_ms (and the other stages) of the decode of those blobs, with and
        without expected digests and sizes; every status must be OK and the output the stream;
  (iii) the CPU baseline: libcrypto's EVP_aes_256_gcm decrypt (16-byte IV, tag checked) on 16
        threads over the same blobs in host memory -- reported as missing when libcrypto does
        not load.

One JSON line per part.

    python scripts/measure_decode.py [--gib 4] [--out FILE]
"""
import argparse
import ctypes
import ctypes.util
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for sub in ("proxmox-backup_amd", "oracle", "tests", "scripts", ""):
    sys.path.insert(0, os.path.join(ROOT, sub))

import pbschunk  # noqa: E402
from measure_encrypt import KEY, REPS, WARM, GiB, cut, emit, med  # noqa: E402


def decode_series(blobs, offs, out, cap, cfg, dig, sizes):
    ts = []
    for i in range(WARM + REPS):
        oo, kinds, status, t = pbschunk.blob_decode_device(blobs.data_ptr(), offs, out.data_ptr(), cap, crypt=cfg,
                                                           expect_digests=dig, expect_sizes=sizes)
        assert not status.any() and (kinds == pbschunk.BLOB_KIND_ENCRYPTED).all(), "a blob of the measurement failed"
        if i >= WARM:
            ts.append(t)
    return ts, oo


def cpu_baseline(host, offs, out):
    try:
        L = ctypes.CDLL(ctypes.util.find_library("crypto") or "libcrypto.so.3")
        L.EVP_CIPHER_CTX_new.restype = ctypes.c_void_p
        L.EVP_aes_256_gcm.restype = ctypes.c_void_p
        L.EVP_CIPHER_CTX_free.argtypes = [ctypes.c_void_p]
        vp, ip = ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)
        L.EVP_DecryptInit_ex.argtypes = [vp, vp, vp, vp, vp]
        L.EVP_CIPHER_CTX_ctrl.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp]
        L.EVP_DecryptUpdate.argtypes = [vp, vp, ip, vp, ctypes.c_int]
        L.EVP_DecryptFinal_ex.argtypes = [vp, vp, ip]
        L.OpenSSL_version.restype = ctypes.c_char_p
        version = L.OpenSSL_version(0).decode()
    except (OSError, AttributeError) as e:
        emit(out, {"part": "iii", "what": "CPU baseline", "missing": f"libcrypto does not load here: {e}"})
        return
    n = int(offs.size - 1)
    dst = np.empty(host.size, dtype=np.uint8)
    cipher = L.EVP_aes_256_gcm()

    def one(i):
        s, e = int(offs[i]), int(offs[i + 1])
        ctx = L.EVP_CIPHER_CTX_new()
        m = ctypes.c_int(0)
        ok = L.EVP_DecryptInit_ex(ctx, cipher, None, None, None) == 1
        ok = ok and L.EVP_CIPHER_CTX_ctrl(ctx, 0x9, 16, None) == 1  # EVP_CTRL_GCM_SET_IVLEN
        ok = ok and L.EVP_DecryptInit_ex(ctx, None, None, KEY, host.ctypes.data + s + 12) == 1
        ok = ok and L.EVP_DecryptUpdate(ctx, dst.ctypes.data + s, ctypes.byref(m), host.ctypes.data + s + 44,
                                        e - s - 44) == 1
        ok = ok and L.EVP_CIPHER_CTX_ctrl(ctx, 0x11, 16, host.ctypes.data + s + 28) == 1  # EVP_CTRL_GCM_SET_TAG
        ok = ok and L.EVP_DecryptFinal_ex(ctx, dst.ctypes.data + e - 44, ctypes.byref(m)) == 1  # (the tag check)
        L.EVP_CIPHER_CTX_free(ctx)
        return ok

    times = []
    with ThreadPoolExecutor(16) as ex:
        for i in range(1 + 3):
            t0 = time.perf_counter()
            ok = all(ex.map(one, range(n)))
            dt = time.perf_counter() - t0
            assert ok, "libcrypto EVP_aes_256_gcm decrypt failed"
            if i >= 1:
                times.append(dt)
    payload = int(host.size) - 44 * n
    emit(out, {"part": "iii", "what": "libcrypto EVP_aes_256_gcm decrypt with tag check, 16 threads, the blobs of (i), "
                                      "host memory",
               "bytes": payload, "seconds": [round(x, 3) for x in times],
               "GiB_s": round(payload / GiB / med(times), 2), "openssl": version})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("measure_decode.py needs a GPU")
    torch.cuda.set_device(0)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out = open(args.out, "w") if args.out else None
    emit(out, {"device": torch.cuda.get_device_name(0), "build_id": pbschunk.build_id(), "warm": WARM, "reps": REPS})
    n = int(args.gib * GiB)
    dev = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    pbschunk.generate_device(dev.data_ptr(), n, pbschunk.GEN_RANDOM, 0x5EED0001, 0)
    bounds = cut(torch, dev, n, 4 << 20)
    nchunks = int(bounds.size - 1)
    cap = pbschunk.blob_stream_bound_encrypted(bounds)
    blobs = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
    with pbschunk.CryptConfig(KEY) as cfg:
        enc = []
        for i in range(WARM + REPS):
            offs, _, _, t = pbschunk.blob_encode_chunks_device(dev.data_ptr(), n, bounds, blobs.data_ptr(), cap,
                                                               compress=False, crypt=cfg)
            if i >= WARM:
                enc.append(t)
        e_ms = med([t["encrypt_ms"] for t in enc])
        emit(out, {"part": "i", "what": "encrypted encode (compress off) of a random stream in HBM, 4 MiB average: "
                                        "the yardstick",
                   "bytes": n, "chunks": nchunks, "segments": int(enc[0]["gcm_segments"]),
                   "encrypt_ms": [round(t["encrypt_ms"], 3) for t in enc], "encrypt_ms_median": round(e_ms, 3),
                   "encrypt_GiB_s": round(n / GiB / (e_ms / 1e3), 2),
                   "crc_ms": round(med([t["crc_ms"] for t in enc]), 3),
                   "total_ms": round(med([t["total_ms"] for t in enc]), 3)})
        dig = pbschunk.digest_chunks_device(dev.data_ptr(), n, bounds, key=cfg.id_key)
        sizes = np.diff(bounds.astype(np.int64)).astype(np.uint64)
        ocap = pbschunk.blob_decode_bound(offs)
        outb = torch.empty(ocap, dtype=torch.uint8, device="cuda:0")
        for name, dg, sz in (("with digests and sizes", dig, sizes), ("without digests", None, None)):
            ts, oo = decode_series(blobs, offs, outb, ocap, cfg, dg, sz)
            assert int(oo[-1]) == n and bool(torch.equal(outb[:n], dev)), "the decoded stream differs from the input"
            d_ms = med([t["decrypt_ms"] for t in ts])
            emit(out, {"part": "ii", "what": "decode of the blobs of (i), " + name,
                       "bytes": n, "chunks": nchunks, "segments": int(ts[0]["gcm_segments"]),
                       "decrypt_ms": [round(t["decrypt_ms"], 3) for t in ts], "decrypt_ms_median": round(d_ms, 3),
                       "decrypt_GiB_s": round(n / GiB / (d_ms / 1e3), 2),
                       "decrypt_over_encrypt": round(d_ms / e_ms, 4),
                       "classify_ms": round(med([t["classify_ms"] for t in ts]), 3),
                       "crc_ms": round(med([t["crc_ms"] for t in ts]), 3),
                       "digest_ms": round(med([t["digest_ms"] for t in ts]), 3),
                       "total_ms": [round(t["total_ms"], 3) for t in ts],
                       "total_ms_median": round(med([t["total_ms"] for t in ts]), 3),
                       "total_GiB_s": round(n / GiB / (med([t["total_ms"] for t in ts]) / 1e3), 2)})
        host = None if args.no_cpu else blobs[:int(offs[-1])].cpu().numpy()
        del dev, blobs, outb
        torch.cuda.empty_cache()
        pbschunk.blob_encode_release()
        if host is not None:
            cpu_baseline(host, offs, out)


if __name__ == "__main__":
    main()
