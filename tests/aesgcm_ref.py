"""Independent AES-256-GCM (16-byte IV, empty AAD) for the tests of the encrypted blob
path, written from FIPS 197 and NIST SP 800-38D and sharing nothing with csrc/:

  - AES in the specification's own steps (SubBytes / ShiftRows / MixColumns on a
    (blocks, 16) NumPy byte array; the S-box from log / antilog tables of generator 3),
    not the T-table form of the kernels;
  - GHASH on Python integers with a per-key 16 x 256 table of (byte at position i) * H;
  - J0 = GHASH_H(IV || 0^64 || [128]_64) for the 16-byte IV, inc32 on the low 32 bits.

``blob_load_decode_encrypted`` is the encrypted arm of the reference's verify_test_blob /
DataBlob::decode (tests/blob_writer.rs:35-68, data_blob.rs:196-252).
"""
import hashlib
import struct
import zlib

import numpy as np

ENCRYPTED_BLOB_MAGIC = bytes([123, 103, 133, 190, 34, 45, 76, 240])  # file_formats.rs:15
ENCR_COMPR_BLOB_MAGIC = bytes([230, 89, 27, 191, 11, 191, 216, 11])  # file_formats.rs:18
ENC_HEADER = 44  # magic[8] crc[4] iv[16] tag[16], file_formats.rs:47-58
_R = 0xE1 << 120


def _xtime(x: int) -> int:
    return ((x << 1) ^ (0x1B if x & 0x80 else 0)) & 0xFF


def _make_sbox() -> np.ndarray:
    exp, log = [0] * 255, [0] * 256
    x = 1
    for i in range(255):
        exp[i] = x
        log[x] = i
        x = _xtime(x) ^ x  # times the generator 3
    sbox = np.zeros(256, dtype=np.uint8)
    for a in range(256):
        inv = exp[(255 - log[a]) % 255] if a else 0
        r = inv
        for k in range(1, 5):
            r ^= ((inv << k) | (inv >> (8 - k))) & 0xFF
        sbox[a] = r ^ 0x63
    return sbox


_SBOX = _make_sbox()
_XT = np.array([_xtime(x) for x in range(256)], dtype=np.uint8)
# ShiftRows on the column-major state: new[r + 4 c] = old[r + 4 ((c + r) % 4)]
_SHIFT = np.array([r + 4 * ((c + r) % 4) for c in range(4) for r in range(4)])


def _expand_key(key: bytes) -> np.ndarray:
    assert len(key) == 32
    w = [list(key[4 * i:4 * i + 4]) for i in range(8)]
    rcon = 1
    for i in range(8, 60):
        t = list(w[i - 1])
        if i % 8 == 0:
            t = [int(_SBOX[b]) for b in t[1:] + t[:1]]
            t[0] ^= rcon
            rcon = _xtime(rcon)
        elif i % 8 == 4:
            t = [int(_SBOX[b]) for b in t]
        w.append([a ^ b for a, b in zip(w[i - 8], t)])
    return np.array(w, dtype=np.uint8).reshape(15, 16)


def _gf_mul(x: int, y: int) -> int:
    z, v = 0, y
    for i in range(128):
        if (x >> (127 - i)) & 1:
            z ^= v
        v = (v >> 1) ^ _R if v & 1 else v >> 1
    return z


class AesGcm256:
    def __init__(self, key: bytes):
        self.rk = _expand_key(bytes(key))
        self.h = int.from_bytes(self.encrypt_blocks(np.zeros((1, 16), dtype=np.uint8)).tobytes(), "big")
        # table[i][b] = (byte b at position i) * H; bit k (MSB first) of byte i is x^(8 i + k)
        hx = [self.h]
        for _ in range(127):
            v = hx[-1]
            hx.append((v >> 1) ^ _R if v & 1 else v >> 1)
        self.tab = []
        for i in range(16):
            row = [0] * 256
            for b in range(1, 256):
                low = b & -b
                row[b] = row[b ^ low] ^ hx[8 * i + 7 - low.bit_length() + 1]
            self.tab.append(row)

    def encrypt_blocks(self, blocks: np.ndarray) -> np.ndarray:
        s = blocks ^ self.rk[0]
        for r in range(1, 15):
            s = _SBOX[s][:, _SHIFT]
            if r < 14:
                a = s.reshape(-1, 4, 4)
                b = _XT[a]
                a1, a2, a3 = np.roll(a, -1, axis=2), np.roll(a, -2, axis=2), np.roll(a, -3, axis=2)
                s = (b ^ np.roll(b, -1, axis=2) ^ a1 ^ a2 ^ a3).reshape(-1, 16)
            s = s ^ self.rk[r]
        return s

    def _mul_h(self, y: int) -> int:
        t = self.tab
        z = 0
        for i, b in enumerate(y.to_bytes(16, "big")):
            z ^= t[i][b]
        return z

    def ghash(self, data: bytes) -> int:
        """GHASH_H over `data` zero-padded to whole blocks."""
        if len(data) % 16:
            data = data + bytes(16 - len(data) % 16)
        y = 0
        for o in range(0, len(data), 16):
            y = self._mul_h(y ^ int.from_bytes(data[o:o + 16], "big"))
        return y

    def j0(self, iv: bytes) -> int:
        assert len(iv) == 16
        return self.ghash(bytes(iv) + bytes(8) + struct.pack(">Q", 128))

    def _keystream(self, j0: int, nblocks: int) -> np.ndarray:
        hi, lo = j0 >> 32, j0 & 0xFFFFFFFF
        ctr = (lo + 1 + np.arange(nblocks, dtype=np.uint64)) & np.uint64(0xFFFFFFFF)  # inc32
        blocks = np.empty((nblocks, 16), dtype=np.uint8)
        blocks[:, :12] = np.frombuffer(hi.to_bytes(12, "big"), dtype=np.uint8)
        blocks[:, 12:] = ctr.astype(">u4").view(np.uint8).reshape(-1, 4)
        return self.encrypt_blocks(blocks).reshape(-1)

    def _tag(self, j0: int, ct: bytes) -> bytes:
        s = self.ghash(ct)
        s = self._mul_h(s ^ (8 * len(ct)))  # [len(A) = 0]_64 || [len(C)]_64
        ek = int.from_bytes(self.encrypt_blocks(np.frombuffer(j0.to_bytes(16, "big"), dtype=np.uint8)
                                                .reshape(1, 16)).tobytes(), "big")
        return (s ^ ek).to_bytes(16, "big")

    def encrypt(self, iv: bytes, data: bytes):
        data = bytes(data)
        j0 = self.j0(iv)
        ks = self._keystream(j0, (len(data) + 15) // 16)[:len(data)]
        ct = (np.frombuffer(data, dtype=np.uint8) ^ ks).tobytes()
        return ct, self._tag(j0, ct)

    def decrypt(self, iv: bytes, ct: bytes, tag: bytes) -> bytes:
        ct = bytes(ct)
        j0 = self.j0(iv)
        if self._tag(j0, ct) != bytes(tag):
            raise ValueError("AES-GCM tag mismatch")
        ks = self._keystream(j0, (len(ct) + 15) // 16)[:len(ct)]
        return (np.frombuffer(ct, dtype=np.uint8) ^ ks).tobytes()

    def iv_for_j0(self, j0: int) -> bytes:
        """The 16-byte IV whose J0 is `j0`: IV = ((J0 H^-1) ^ 128) H^-1 (for counter-wrap cases)."""
        hinv = 1 << 127  # the field's one
        base, e = self.h, (1 << 128) - 2
        while e:
            if e & 1:
                hinv = _gf_mul(hinv, base)
            base = _gf_mul(base, base)
            e >>= 1
        return _gf_mul(_gf_mul(j0, hinv) ^ 128, hinv).to_bytes(16, "big")


_CACHE = {}


def cipher(key: bytes) -> AesGcm256:
    key = bytes(key)
    if key not in _CACHE:
        _CACHE[key] = AesGcm256(key)
    return _CACHE[key]


def id_key(enc_key: bytes) -> bytes:
    """CryptConfig::new, crypt_config.rs:42-61."""
    return hashlib.pbkdf2_hmac("sha256", bytes(enc_key), b"_id_key", 10, 32)


def blob_encode_encrypted(data: bytes, enc_key: bytes, iv: bytes, payload_is_zstd: bool = False) -> bytes:
    """DataBlob::encode(data, Some(config), ..) (data_blob.rs:107-131) with a given IV;
    `payload_is_zstd`: `data` is already the zstd frame (ENCR_COMPR magic)."""
    ct, tag = cipher(enc_key).encrypt(iv, data)
    magic = ENCR_COMPR_BLOB_MAGIC if payload_is_zstd else ENCRYPTED_BLOB_MAGIC
    return magic + struct.pack("<I", zlib.crc32(ct)) + bytes(iv) + tag + ct


def blob_decrypt_payload(blob: bytes, enc_key: bytes) -> bytes:
    """The decrypted payload (chunk bytes or zstd frame) after magic, size, CRC and tag checks."""
    blob = bytes(blob)
    if len(blob) < ENC_HEADER:  # from_raw, data_blob.rs:279-281
        raise ValueError(f"encrypted blob too small ({len(blob)} bytes).")
    if blob[:8] not in (ENCRYPTED_BLOB_MAGIC, ENCR_COMPR_BLOB_MAGIC):
        raise ValueError("unable to parse raw blob - wrong magic")
    if struct.unpack("<I", blob[8:12])[0] != zlib.crc32(blob[ENC_HEADER:]):  # verify_crc :78-84
        raise ValueError("Data blob has wrong CRC checksum.")
    return cipher(enc_key).decrypt(blob[12:28], blob[ENC_HEADER:], blob[28:44])


def blob_load_decode_encrypted(blob: bytes, cfg_key: bytes, digest=None) -> bytes:
    """DataBlob::load_from_reader(blob).decode(Some(config), digest) for the two encrypted
    magics: raises ValueError where the reference bails."""
    import oracle

    blob = bytes(blob)
    data = blob_decrypt_payload(blob, cfg_key)
    if blob[:8] == ENCR_COMPR_BLOB_MAGIC:  # decode :226-241: decode_all of the plaintext
        data = oracle.zstd_decode_stream(data, 1 << 17)
    if digest is not None:  # verify_digest with the config: SHA-256(data || id_key)
        if hashlib.sha256(data + id_key(cfg_key)).digest() != bytes(digest):
            raise ValueError("detected chunk with wrong digest.")
    return data


def golden_plaintext(length: int, seed: int) -> bytes:
    """The plaintext of a tests/golden/aesgcm_vectors.json case: byte i = (i * 131 + seed) % 251."""
    i = np.arange(length, dtype=np.uint64)
    return ((i * np.uint64(131) + np.uint64(seed)) % np.uint64(251)).astype(np.uint8).tobytes()
