#!/usr/bin/env python3
"""Measurements of the encrypted blob path on an MI355X (the AES-256-GCM section):

  (a) encrypt-only rate from HBM: compress off, a device-resident random stream cut at the
      4 MiB average; `encrypt_ms` is the HIP-event time of the three GCM launches;
  (b) what encryption adds to the compressed encode of the text corpus: encrypt_ms beside
      compress_ms, and the whole call with and without a crypt config;
  (c) pbs_upload_stream_host with and without a crypt config over the text corpus;
  (d) the CPU baseline: libcrypto's EVP_aes_256_gcm (16-byte IV) on 16 threads over the
      chunks of (a) on the same machine -- reported as missing when libcrypto does not load.

Warm launches first, then several timed repeats (the variants alternate); board power and
GFX clock are sampled beside the runs (amd-smi, read only).  One JSON line per part.

    python scripts/measure_encrypt.py [--gib 4] [--text-gib 4] [--upload-gib 16] [--out FILE]
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
from avg_table import PowerSampler  # noqa: E402

GiB = 1 << 30
KEY = bytes(range(32))
WARM, REPS = 2, 5


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def emit(out, rec):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def cut(torch, dev, n, avg):
    with pbschunk.Chunker(avg) as c:
        c.set_stream(torch.cuda.current_stream().cuda_stream)
        ends = c.find_cuts_device(dev.data_ptr(), n, is_final=True)
    return np.concatenate([[0], ends]).astype(np.uint64)


def encode_series(dev, n, bounds, blobs, cap, compress, cfg):
    """WARM + REPS calls; the timing dicts of the timed ones."""
    ts = []
    for i in range(WARM + REPS):
        _, _, _, t = pbschunk.blob_encode_chunks_device(dev.data_ptr(), n, bounds, blobs.data_ptr(), cap,
                                                        compress=compress, crypt=cfg)
        if i >= WARM:
            ts.append(t)
    return ts


def part_a(torch, cfg, gib, out):
    n = int(gib * GiB)
    dev = torch.empty(n, dtype=torch.uint8, device="cuda:0")
    pbschunk.generate_device(dev.data_ptr(), n, pbschunk.GEN_RANDOM, 0x5EED0001, 0)
    bounds = cut(torch, dev, n, 4 << 20)
    cap = pbschunk.blob_stream_bound_encrypted(bounds)
    blobs = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
    with PowerSampler() as ps:
        enc = encode_series(dev, n, bounds, blobs, cap, False, cfg)
        plain = encode_series(dev, n, bounds, blobs, cap, False, None)
    e_ms = med([t["encrypt_ms"] for t in enc])
    emit(out, {"part": "a", "what": "encrypt only, compress off, random stream in HBM, 4 MiB average",
               "bytes": n, "chunks": int(bounds.size - 1), "segments": int(enc[0]["gcm_segments"]),
               "encrypt_ms": [round(t["encrypt_ms"], 3) for t in enc],
               "encrypt_GiB_s": round(n / GiB / (e_ms / 1e3), 2),
               "assemble_ms": round(med([t["assemble_ms"] for t in enc]), 3),
               "crc_ms": round(med([t["crc_ms"] for t in enc]), 3),
               "total_ms_crypt": round(med([t["total_ms"] for t in enc]), 3),
               "total_ms_plain": round(med([t["total_ms"] for t in plain]), 3),
               "box": ps.summary()})
    host = dev.cpu().numpy()
    del dev, blobs
    torch.cuda.empty_cache()
    return host, bounds


def text_host(n):
    import bench

    return bench.corpus_host("text", n)[0]


def part_b(torch, cfg, gib, out):
    n = int(gib * GiB)
    host = text_host(n)
    dev = torch.from_numpy(host).to("cuda:0")
    bounds = cut(torch, dev, n, 4 << 20)
    cap = pbschunk.blob_stream_bound_encrypted(bounds)
    blobs = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
    with PowerSampler() as ps:
        enc = encode_series(dev, n, bounds, blobs, cap, True, cfg)
        plain = encode_series(dev, n, bounds, blobs, cap, True, None)
    t_c, t_p = med([t["total_ms"] for t in enc]), med([t["total_ms"] for t in plain])
    e_ms, c_ms = med([t["encrypt_ms"] for t in enc]), med([t["compress_ms"] for t in enc])
    emit(out, {"part": "b", "what": "compressed encode of the text corpus in HBM, with and without crypt",
               "bytes": n, "chunks": int(bounds.size - 1), "bytes_out": int(enc[0]["bytes_out"]),
               "compress_ms": round(c_ms, 3), "encrypt_ms": round(e_ms, 3),
               "assemble_ms": round(med([t["assemble_ms"] for t in enc]), 3),
               "crc_ms": round(med([t["crc_ms"] for t in enc]), 3),
               "total_ms_crypt": round(t_c, 3), "total_ms_plain": round(t_p, 3),
               "encode_GiB_s_crypt": round(n / GiB / (t_c / 1e3), 2),
               "encode_GiB_s_plain": round(n / GiB / (t_p / 1e3), 2),
               "encrypt_share_of_call": round(e_ms / t_c, 4), "box": ps.summary()})
    del dev, blobs
    torch.cuda.empty_cache()


def part_c(torch, cfg, gib, out):
    n = int(gib * GiB)
    host = text_host(n)
    cap = n // (1 << 20) + 4
    blobs = np.empty(44 * cap + n, dtype=np.uint8)
    res = {"plain": [], "crypt": []}
    enc_ms, sizes = [], {}
    with PowerSampler() as ps:
        for i in range(1 + 3):
            for name, c in (("plain", None), ("crypt", cfg)):
                t0 = time.perf_counter()
                o = pbschunk.upload_stream_host(host, 4 << 20, crypt=c, blobs_out=blobs)
                dt = time.perf_counter() - t0
                if i >= 1:
                    res[name].append(dt)
                    if c is not None:
                        enc_ms.append(o["timing"]["encrypt_ms"])
                sizes[name] = o["stats"]["size_compressed"]
    p, c = med(res["plain"]), med(res["crypt"])
    emit(out, {"part": "c", "what": "upload_stream_host over the text corpus (pageable host buffers), 4 MiB average",
               "bytes": n, "seconds_plain": [round(x, 3) for x in res["plain"]],
               "seconds_crypt": [round(x, 3) for x in res["crypt"]],
               "GiB_s_plain": round(n / GiB / p, 2), "GiB_s_crypt": round(n / GiB / c, 2),
               "encrypt_ms_sum": round(med(enc_ms), 2), "encrypt_share_of_call": round(med(enc_ms) / 1e3 / c, 4),
               "size_compressed": sizes, "box": ps.summary()})


def part_d(host, bounds, out):
    try:
        L = ctypes.CDLL(ctypes.util.find_library("crypto") or "libcrypto.so.3")
        L.EVP_CIPHER_CTX_new.restype = ctypes.c_void_p
        L.EVP_aes_256_gcm.restype = ctypes.c_void_p
        L.EVP_CIPHER_CTX_free.argtypes = [ctypes.c_void_p]
        vp, ip = ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)
        L.EVP_EncryptInit_ex.argtypes = [vp, vp, vp, vp, vp]
        L.EVP_CIPHER_CTX_ctrl.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp]
        L.EVP_EncryptUpdate.argtypes = [vp, vp, ip, vp, ctypes.c_int]
        L.EVP_EncryptFinal_ex.argtypes = [vp, vp, ip]
        L.OpenSSL_version.restype = ctypes.c_char_p
        version = L.OpenSSL_version(0).decode()
    except (OSError, AttributeError) as e:
        emit(out, {"part": "d", "what": "CPU baseline", "missing": f"libcrypto does not load here: {e}"})
        return
    dst = np.empty(host.size, dtype=np.uint8)
    n = int(bounds.size - 1)
    tags = np.zeros((n, 16), dtype=np.uint8)
    cipher = L.EVP_aes_256_gcm()
    iv = bytes(range(16, 32))

    def one(i):
        s, e = int(bounds[i]), int(bounds[i + 1])
        ctx = L.EVP_CIPHER_CTX_new()
        m = ctypes.c_int(0)
        ok = L.EVP_EncryptInit_ex(ctx, cipher, None, None, None) == 1
        ok = ok and L.EVP_CIPHER_CTX_ctrl(ctx, 0x9, 16, None) == 1
        ok = ok and L.EVP_EncryptInit_ex(ctx, None, None, KEY, iv) == 1
        ok = ok and L.EVP_EncryptUpdate(ctx, dst.ctypes.data + s, ctypes.byref(m), host.ctypes.data + s, e - s) == 1
        ok = ok and L.EVP_EncryptFinal_ex(ctx, dst.ctypes.data + e, ctypes.byref(m)) == 1
        ok = ok and L.EVP_CIPHER_CTX_ctrl(ctx, 0x10, 16, tags[i].ctypes.data) == 1
        L.EVP_CIPHER_CTX_free(ctx)
        return ok

    times = []
    with ThreadPoolExecutor(16) as ex:
        for i in range(1 + 3):
            t0 = time.perf_counter()
            ok = all(ex.map(one, range(n)))
            dt = time.perf_counter() - t0
            assert ok, "libcrypto EVP_aes_256_gcm failed"
            if i >= 1:
                times.append(dt)
    emit(out, {"part": "d", "what": "libcrypto EVP_aes_256_gcm, 16 threads, the chunks of (a), host memory",
               "bytes": int(host.size), "seconds": [round(x, 3) for x in times],
               "GiB_s": round(host.size / GiB / med(times), 2), "openssl": version})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gib", type=float, default=4.0)
    ap.add_argument("--text-gib", type=float, default=4.0)
    ap.add_argument("--upload-gib", type=float, default=16.0)
    ap.add_argument("--parts", default="abcd")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("measure_encrypt.py needs a GPU")
    torch.cuda.set_device(0)
    out = open(args.out, "w") if args.out else None
    emit(out, {"device": torch.cuda.get_device_name(0), "build_id": pbschunk.build_id(), "warm": WARM, "reps": REPS})
    with pbschunk.CryptConfig(KEY) as cfg:
        host = bounds = None
        if "a" in args.parts or "d" in args.parts:
            host, bounds = part_a(torch, cfg, args.gib, out)
        if "b" in args.parts:
            part_b(torch, cfg, args.text_gib, out)
        pbschunk.blob_encode_release()
        if "d" in args.parts:
            part_d(host, bounds, out)
        del host
        if "c" in args.parts:
            part_c(torch, cfg, args.upload_gib, out)
    pbschunk.blob_encode_release()
    pbschunk.pipeline_release()


if __name__ == "__main__":
    main()
