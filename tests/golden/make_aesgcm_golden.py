"""Generates tests/golden/aesgcm_vectors.json from the local libcrypto (EVP_aes_256_gcm with
a 16-byte IV, empty AAD) through ctypes:  python tests/golden/make_aesgcm_golden.py

Per case: key, IV, length, plaintext seed (aesgcm_ref.golden_plaintext), tag and the SHA-256
of the ciphertext.  Two IVs per key are built by inverting the J0 map so that the 32-bit
counter wraps inside the message (J0's low word 0xFFFFFFF0 and 0xFFFFFFFF); the expected
values of those cases, like all others, come from libcrypto.
"""
import ctypes
import ctypes.util
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle"))

import aesgcm_ref  # noqa: E402

LENGTHS = [0, 1, 15, 16, 17, 31, 32, 33, 255, 4105, 65536, 100000]
KEYS = [bytes([1]) * 32, hashlib.sha256(b"aesgcm golden key").digest()]
EVP_CTRL_GCM_SET_IVLEN, EVP_CTRL_GCM_GET_TAG = 0x9, 0x10


def libcrypto():
    L = ctypes.CDLL(ctypes.util.find_library("crypto") or "libcrypto.so.3")
    L.EVP_CIPHER_CTX_new.restype = ctypes.c_void_p
    L.EVP_aes_256_gcm.restype = ctypes.c_void_p
    L.EVP_CIPHER_CTX_free.argtypes = [ctypes.c_void_p]
    return L


def evp_encrypt(L, key: bytes, iv: bytes, data: bytes):
    ctx = ctypes.c_void_p(L.EVP_CIPHER_CTX_new())
    try:
        ok = L.EVP_EncryptInit_ex(ctx, ctypes.c_void_p(L.EVP_aes_256_gcm()), None, None, None) == 1
        ok = ok and L.EVP_CIPHER_CTX_ctrl(ctx, EVP_CTRL_GCM_SET_IVLEN, len(iv), None) == 1
        ok = ok and L.EVP_EncryptInit_ex(ctx, None, None, key, iv) == 1
        out = ctypes.create_string_buffer(len(data) + 16)
        n, m = ctypes.c_int(0), ctypes.c_int(0)
        ok = ok and L.EVP_EncryptUpdate(ctx, out, ctypes.byref(n), data, len(data)) == 1
        ok = ok and L.EVP_EncryptFinal_ex(ctx, ctypes.byref(out, n.value), ctypes.byref(m)) == 1
        tag = ctypes.create_string_buffer(16)
        ok = ok and L.EVP_CIPHER_CTX_ctrl(ctx, EVP_CTRL_GCM_GET_TAG, 16, tag) == 1
        if not ok:
            raise RuntimeError("libcrypto EVP_aes_256_gcm failed")
        return out.raw[:len(data)], tag.raw
    finally:
        L.EVP_CIPHER_CTX_free(ctx)


def main():
    L = libcrypto()
    cases = []
    for ki, key in enumerate(KEYS):
        c = aesgcm_ref.cipher(key)
        for n in LENGTHS:
            iv = hashlib.sha256(b"iv %d %d" % (ki, n)).digest()[:16]
            cases.append((key, iv, n, 16 * ki + n % 13, None))
        for low in (0xFFFFFFF0, 0xFFFFFFFF):
            j0 = int.from_bytes(hashlib.sha256(b"j0 %d" % ki).digest()[:12], "big") << 32 | low
            iv = c.iv_for_j0(j0)
            for n in (1024, 100000):
                cases.append((key, iv, n, 7 + ki, low))
    out = []
    for key, iv, n, seed, low in cases:
        ct, tag = evp_encrypt(L, key, iv, aesgcm_ref.golden_plaintext(n, seed))
        e = {"key": key.hex(), "iv": iv.hex(), "len": n, "seed": seed, "tag": tag.hex(),
             "ct_sha256": hashlib.sha256(ct).hexdigest()}
        if low is not None:
            e["j0_low32"] = "%08x" % low
        out.append(e)
    doc = {"source": "libcrypto EVP_aes_256_gcm, IV length 16, empty AAD",
           "plaintext": "byte i = (i * 131 + seed) % 251", "cases": out}
    with open(os.path.join(HERE, "aesgcm_vectors.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"{len(out)} cases")


if __name__ == "__main__":
    main()
