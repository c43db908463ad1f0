"""Blob images to open, planted on the boundaries of the read side (helpers of
test_dplanted_cpu.py and test_gpu_decode.py; not a conftest).

The read side (proxmox-backup_amd/csrc/pbs_decode.hip) classifies every blob (12- or 44-byte
header), checks its CRC, copies the unencrypted payloads and opens the encrypted ones with the
geometry of the sealing kernel -- 64 KiB segments counted from the payload's end, 256 lanes,
16 rows, the last partial block byte by byte -- but out of place: the plaintext goes to the
packed output, whose residue mod 16 differs from the source's.

Every item is an Item: the blob image, what the caller passes for it (expected digest, expected
size) and what the call must return (kind, status, payload).  Blobs come from
tests/aesgcm_ref.py (blob_encode_encrypted), oracle.blob_uncompressed and
oracle.blob_compressed; the wanted status of a corrupted blob is stated where it is planted and
test_dplanted_cpu.py proves it with the reference functions alone (reference_outcome).
Families a-f are the gplanted families re-used as blobs to open.
"""
import hashlib
import struct
import zlib
from typing import NamedTuple, Optional

import numpy as np

import aesgcm_ref
import gplanted as g

HDR, EHDR = 12, g.HDR
KIND_NONE = 255                   # PBS_BLOB_KIND_NONE
OK, TOO_SMALL, BAD_MAGIC, BAD_CRC, NO_CONFIG, BAD_TAG, BAD_DIGEST, BAD_SIZE = range(8)  # PBS_BLOB_ST_*
STATUS_NAMES = ("OK", "TOO_SMALL", "BAD_MAGIC", "BAD_CRC", "NO_CONFIG", "BAD_TAG", "BAD_DIGEST", "BAD_SIZE")
UNCOMPRESSED_MAGIC = bytes([66, 171, 56, 7, 190, 131, 112, 161])   # file_formats.rs:9
COMPRESSED_MAGIC = bytes([49, 185, 88, 66, 111, 182, 163, 127])    # file_formats.rs:12
MAGICS = (UNCOMPRESSED_MAGIC, COMPRESSED_MAGIC, aesgcm_ref.ENCRYPTED_BLOB_MAGIC, aesgcm_ref.ENCR_COMPR_BLOB_MAGIC)
ZERO32 = bytes(32)


class Item(NamedTuple):
    label: str
    blob: bytes
    digest: bytes      # what the caller expects (32 bytes; ignored by the call for kinds 1 and 3)
    size: int          # what the caller expects (checked for kind 0 only)
    kind: int          # wanted
    status: int        # wanted
    payload: bytes     # wanted output (zeros for a failed encrypted blob, b"" before the length is known)


def kind_of(blob: bytes) -> int:
    return MAGICS.index(blob[:8]) if len(blob) >= HDR and blob[:8] in MAGICS else KIND_NONE


def _with_crc(blob: bytes) -> bytes:
    h = EHDR if kind_of(blob) >= 2 else HDR
    return blob[:8] + struct.pack("<I", zlib.crc32(blob[h:])) + blob[12:]


def _flip(blob: bytes, at: int, bit: int = 0) -> bytes:
    b = bytearray(blob)
    b[at] ^= 1 << bit
    return bytes(b)


def plain_digest(data: bytes) -> bytes:
    return hashlib.sha256(data).digest()


def keyed_digest(data: bytes, key: bytes) -> bytes:
    return hashlib.sha256(data + aesgcm_ref.id_key(key)).digest()


def good(label: str, blob: bytes, key: Optional[bytes], data: Optional[bytes] = None) -> Item:
    """An intact blob: its payload is what follows the header (decrypted for the encrypted
    kinds); `data`: the chunk for kinds 0 and 2 (digest and size are the chunk's)."""
    k = kind_of(blob)
    pay = aesgcm_ref.blob_decrypt_payload(blob, key) if k >= 2 else blob[HDR:]
    if k in (0, 2):
        assert data is None or data == pay
        dig = keyed_digest(pay, key) if k == 2 else plain_digest(pay)
    else:
        dig = ZERO32
    return Item(label, blob, dig, len(pay), k, OK, pay)


def bad(label: str, src: Item, blob: bytes, status: int, digest=None, size=None) -> Item:
    """A corrupted form of the intact item `src`."""
    k = kind_of(blob)
    plen = 0 if status in (TOO_SMALL, BAD_MAGIC) else len(blob) - (EHDR if k >= 2 else HDR)
    pay = b"" if plen == 0 else bytes(plen) if k >= 2 else blob[HDR:]
    return Item(label, blob, src.digest if digest is None else digest, src.size if size is None else size, k, status,
                pay)


# ---- the reference's verdict -------------------------------------------------------------------

_MESSAGES = (("too small", TOO_SMALL), ("wrong magic", BAD_MAGIC), ("wrong CRC", BAD_CRC), ("tag mismatch", BAD_TAG),
             ("wrong digest", BAD_DIGEST))


def _status_of(err: ValueError) -> int:
    for text, st in _MESSAGES:
        if text in str(err):
            return st
    raise err


def reference_outcome(oracle, it: Item, key: Optional[bytes]):
    """(status, payload or None) of `it` by the reference functions alone:
    DataBlob::load_from_reader + decode (+ verify_unencrypted's length for kind 0), as
    oracle.blob_load_decode and aesgcm_ref.blob_load_decode_encrypted restate them.  The digest
    of a compressed kind is the caller's to check after inflating, so none is passed there."""
    blob = it.blob
    enc = len(blob) >= HDR and blob[:8] in MAGICS[2:]
    try:
        if not enc:
            k = kind_of(blob)
            data = oracle.blob_load_decode(blob, it.digest if k == 0 else None, read_sizes=(64 * 1024,))
            if k == 0 and len(data) != it.size:  # verify_unencrypted, data_blob.rs:324-331
                return BAD_SIZE, blob[HDR:]
            return OK, blob[HDR:]
        if key is None:  # load (size, magic, CRC) passes or fails as with any key; then decode :247-249
            try:
                aesgcm_ref.blob_decrypt_payload(blob, g.KEY1)
            except ValueError as e:
                if _status_of(e) != BAD_TAG:
                    return _status_of(e), None
            return NO_CONFIG, None
        aesgcm_ref.blob_load_decode_encrypted(blob, key, it.digest if blob[:8] == MAGICS[2] else None)
        return OK, aesgcm_ref.blob_decrypt_payload(blob, key)
    except ValueError as e:
        return _status_of(e), None


# ---- a-f: the gplanted families as blobs to open ------------------------------------------------

def _from_gplanted(family: str, *args) -> list:
    return [good(c.label, b, c.key, c.chunk.tobytes()) for c, b in zip(g.cases(family, *args), g.expected(family, *args))]


OUT_PADS = tuple(range(8))       # residues of the packed output's start the GPU test runs family a at


def tail_triples(in_pads=g.TAIL_PADS, out_pads=g.TAIL_PADS) -> set:
    """Every (payload length mod 16, source residue mod 16, destination residue mod 16) family a
    shows when its blob stream starts at residue in_pad and its packed output at out_pad."""
    out = set()
    for ip in in_pads:
        starts = g.tail_starts(ip)
        for op in out_pads:
            at = op
            for n, s in zip(g.TAIL_LENGTHS, starts):
                out.add((n % 16, s % 16, at % 16))
                at += n
    return out


def compressed_items(oracle) -> list:
    """f. gplanted's compressed payloads (encrypted frames, or chunks where the frame is no
    shorter) and the same chunks as unencrypted blobs of the oracle."""
    cs = g.cases("f")
    out = []
    for c, (blob, z) in zip(cs, g.compressed_expected(oracle, cs)):
        out.append(good(c.label + "/enc", blob, c.key, None if z else c.chunk.tobytes()))
        out.append(good(c.label + "/plain", oracle.blob_compressed(c.chunk.tobytes()), None))
    return out


# ---- g: mixed stream -----------------------------------------------------------------------------

MIX_LENGTHS = (1, 15, 16, 17, 600, 4096, 65536, 65537, 70001, 3 * 65536 - 5)


def _chunk(seed: int, n: int, compressible: bool) -> bytes:
    if compressible:
        import corpus_gen
        return corpus_gen.text(n + 64, seed)[:n].tobytes() if n >= 4096 else bytes(n)
    return np.random.default_rng([0x6D6978, seed]).integers(0, 256, n, dtype=np.uint8).tobytes()


def make_blob(oracle, kind: int, chunk: bytes, key: bytes, iv: bytes) -> bytes:
    if kind == 0:
        return oracle.blob_uncompressed(chunk)
    plain = oracle.blob_compressed(chunk)
    if kind == 1:
        return plain
    if kind == 2:
        return aesgcm_ref.blob_encode_encrypted(chunk, key, iv)
    return aesgcm_ref.blob_encode_encrypted(plain[HDR:], key, iv, plain[:8] == COMPRESSED_MAGIC)


def mixed_items(oracle) -> list:
    """g. All four kinds interleaved, the kind advancing with every blob, and a zero-length
    payload (kind 0 or 2 in turn: a zstd frame is never empty) after each: consecutive blobs
    switch between the 12- and the 44-byte header.  The compressed kinds hold chunks that
    compress (zeros, text), so their magic is the compressed one from 4096 bytes up."""
    out = []
    for j, n in enumerate(MIX_LENGTHS * 2):
        kind = (j + j // len(MIX_LENGTHS)) % 4
        chunk = _chunk(j, n, kind in (1, 3))
        blob = make_blob(oracle, kind, chunk, g.KEY1, g._iv(7000 + j))
        out.append(good(f"g/{j}/kind{kind}/len{n}", blob, g.KEY1))
        ek = (0, 2)[j % 2]
        out.append(good(f"g/{j}/empty-kind{ek}", make_blob(oracle, ek, b"", g.KEY1, g._iv(7500 + j)), g.KEY1, b""))
    return out


# ---- h: corruptions ------------------------------------------------------------------------------

H_LEN = g.CTR_LEN                 # 300 + 4096 blocks, 5 bytes in the last: two segments
H_FIRST = g.CTR_FIRST
# payload bytes to flip one bit of: byte 0; the last byte (in the partial block); either side of
# the segment boundary (block 299 | 300); of a lane's row step in segment 1 (its blocks 255 | 256)
# and in segment 0 (block 0 is slot 3796, row 14: row 15 starts at block 44); of the first block
# of the ragged first segment (block 0 | 1)
H_FLIPS = (("byte0", 0), ("last", H_LEN - 1),
           ("seg-lo", 16 * H_FIRST - 1), ("seg-hi", 16 * H_FIRST),
           ("row-lo", 16 * (H_FIRST + 256) - 1), ("row-hi", 16 * (H_FIRST + 256)),
           ("row0-lo", 16 * 44 - 1), ("row0-hi", 16 * 44),
           ("first-lo", 15), ("first-hi", 16))


def flips_hold() -> bool:
    """The planted flip positions are where their names say (gplanted.geometry)."""
    m, nseg, first, rem = g.geometry(H_LEN)
    slot0 = g.SEGBLOCKS - first
    return ((m, nseg, first, rem) == (g.SEGBLOCKS + H_FIRST, 2, H_FIRST, 5)
            and (slot0 + 44) % g.LANES == 0 and (slot0 + 43) // g.LANES == 14
            and dict(H_FLIPS)["last"] // 16 == m - 1 and rem != 0
            and all(0 <= at < H_LEN for _, at in H_FLIPS))


def _neighbour(oracle, i: int) -> Item:
    kind = i % 4
    chunk = _chunk(900 + i, (33, 4500, 160, 5000)[kind] + i, kind in (1, 3))
    return good(f"h/neighbour{i}/kind{kind}", make_blob(oracle, kind, chunk, g.KEY1, g._iv(8000 + i)), g.KEY1)


def corrupt_items(oracle) -> list:
    """h. The corrupted blobs alone (corrupt_stream puts the intact neighbours between)."""
    key = g.KEY1
    big = np.random.default_rng(0x68).integers(0, 256, H_LEN, dtype=np.uint8).tobytes()
    text = _chunk(0x69, 70000, True)
    base = {k: good(f"h/base{k}", make_blob(oracle, k, big if k in (0, 2) else text, key, g._iv(8800 + k)), key)
            for k in range(4)}
    assert [base[k].kind for k in range(4)] == [0, 1, 2, 3]
    small = {k: good(f"h/small{k}", make_blob(oracle, k, _chunk(0x70 + k, 100, False), key, g._iv(8900 + k)), key)
             for k in (0, 2)}
    out = []
    for k in (0, 2):
        s, hdr = small[k], (HDR, EHDR)[k // 2]
        for n in range(12):  # from_raw :269-271
            out.append(bad(f"h/kind{k}/len{n}", s, s.blob[:n], TOO_SMALL))
        # the header alone: the stored CRC is the full payload's (stale); then the genuine empty blob
        out.append(bad(f"h/kind{k}/len{hdr}-stale", s, s.blob[:hdr], BAD_CRC))
        out.append(good(f"h/kind{k}/len{hdr}-empty", make_blob(oracle, k, b"", key, g._iv(8950 + k)), key, b""))
        out.append(bad(f"h/kind{k}/magic-bit", s, _flip(s.blob, 0, 3), BAD_MAGIC))
        out.append(bad(f"h/kind{k}/magic-last-bit", s, _flip(s.blob, 7, 7), BAD_MAGIC))
        out.append(bad(f"h/kind{k}/crc-bit", s, _flip(s.blob, 8 + k, 5), BAD_CRC))
        out.append(bad(f"h/kind{k}/wrong-digest", s, s.blob, BAD_DIGEST, digest=_flip(s.digest, 31, 0)))
        # verify_unencrypted returns Ok for encrypted blobs: the size is checked for kind 0 only
        out.append(bad(f"h/kind{k}/wrong-size", s, s.blob, BAD_SIZE, size=s.size + 1) if k == 0
                   else s._replace(label="h/kind2/wrong-size-ignored", size=s.size + 1))
    s = small[2]
    for n in range(12, 44):  # an encrypted magic under 44 bytes, from_raw :276-278
        out.append(bad(f"h/kind2/len{n}", s, s.blob[:n], TOO_SMALL))
    for name, at in (("iv0", 12), ("iv15", 27), ("tag0", 28), ("tag15", 43)):  # (the CRC does not cover them)
        for k in (2, 3):
            b = small[2] if k == 2 else base[3]
            out.append(bad(f"h/kind{k}/{name}", b, _flip(b.blob, at, 6), BAD_TAG))
    for k in (2, 3):
        b = small[2] if k == 2 else base[3]
        chunk = b.payload if k == 2 else text
        out.append(bad(f"h/kind{k}/wrong-key", b, make_blob(oracle, k, chunk, g.SPARE_KEY, g._iv(8990 + k)), BAD_TAG))
    # one flipped payload bit: the CRC left stale, then recomputed
    for k in (0, 2):
        b, hdr = base[k], (HDR, EHDR)[k // 2]
        for name, at in H_FLIPS:
            f = _flip(b.blob, hdr + at, at % 8)
            out.append(bad(f"h/kind{k}/flip-{name}/stale-crc", b, f, BAD_CRC))
            out.append(bad(f"h/kind{k}/flip-{name}/crc-recomputed", b, _with_crc(f), BAD_DIGEST if k == 0 else BAD_TAG))
    for k in (1, 3):  # (a recomputed CRC over a damaged frame of kind 1 is the inflater's to find)
        b, hdr = base[k], (HDR, EHDR)[k // 2]
        for name, at in (("byte0", 0), ("last", len(b.payload) - 1)):
            f = _flip(b.blob, hdr + at, 2)
            out.append(bad(f"h/kind{k}/flip-{name}/stale-crc", b, f, BAD_CRC))
            if k == 3:
                out.append(bad(f"h/kind3/flip-{name}/crc-recomputed", b, _with_crc(f), BAD_TAG))
    return out


def corrupt_stream(oracle) -> list:
    """h as one stream: every corrupted blob between two intact neighbours of changing kinds."""
    out = [_neighbour(oracle, 0)]
    for i, it in enumerate(corrupt_items(oracle)):
        out += [it, _neighbour(oracle, i + 1)]
    return out


def no_config_stream(oracle) -> list:
    """h, `cfg` absent: the mixed stream opened without a config -- the unencrypted blobs as
    before, every encrypted one NO_CONFIG with a zeroed payload; one encrypted blob with a stale
    CRC (load fails before decode asks for the config) and one too small."""
    out = []
    for it in mixed_items(oracle):
        out.append(it if it.kind < 2 else bad(it.label + "/no-config", it, it.blob, NO_CONFIG))
    enc = next(it for it in out if it.kind == 2 and len(it.blob) > EHDR + 16)
    out.insert(3, bad("h/no-config/stale-crc", enc, _flip(enc.blob, EHDR + 3), BAD_CRC))
    out.insert(6, bad("h/no-config/len30", enc, enc.blob[:30], TOO_SMALL))
    return out


_streams = {}


def stream(name: str, oracle=None, *args) -> list:
    """The items of a family, built once per process: a, b, c, d (ncu), e, e-spare, f, g, h,
    h-nocfg."""
    k = (name,) + args
    if k not in _streams:
        if name in ("f", "g", "h", "h-nocfg"):
            _streams[k] = {"f": compressed_items, "g": mixed_items, "h": corrupt_stream,
                           "h-nocfg": no_config_stream}[name](oracle)
        else:
            _streams[k] = _from_gplanted(name, *args)
    return _streams[k]


# ---- the GPU side (test_gpu_decode.py) -----------------------------------------------------------

FILL_IN, FILL_OUT, GUARD = 0x5A, 0xA5, 4096


class Decoded(NamedTuple):
    payloads: list
    offsets: np.ndarray
    kinds: np.ndarray
    status: np.ndarray
    input_unchanged: bool
    outside_clean: bool   # every output byte outside [0, out_offsets[n]) as it was filled, guard included
    timing: dict


def layout(items):
    """(blob stream, offsets)"""
    stream_ = b"".join(it.blob for it in items)
    return np.frombuffer(stream_, np.uint8), np.concatenate([[0], np.cumsum([len(it.blob) for it in items])]).astype(np.uint64)


def gpu_upload(torch, data: np.ndarray, pad: int):
    """(tensor, lead): the blob stream `pad` mod 16 into a buffer filled with FILL_IN."""
    t = torch.full((32 + data.size + 64,), FILL_IN, dtype=torch.uint8, device="cuda")
    lead = (-t.data_ptr()) % 16 + pad
    if data.size:
        t[lead:lead + data.size] = torch.from_numpy(data.copy()).to("cuda")
    return t, lead


def gpu_decode(gpu, torch, cfg, items, pad: int = 5, out_pad: int = 9, use_digests: bool = True, use_sizes: bool = True,
               hip_stream: int = 0, src=None) -> Decoded:
    """One decode call: the input at residue `pad` in a filled buffer, the output at residue
    `out_pad` in a pre-filled buffer with GUARD bytes behind pbs_blob_decode_bound."""
    data, offs = layout(items)
    t, lead = src or gpu_upload(torch, data, pad)
    before = t.clone()
    cap = gpu.blob_decode_bound(offs)
    out = torch.full((32 + cap + GUARD,), FILL_OUT, dtype=torch.uint8, device="cuda")
    olead = (-out.data_ptr()) % 16 + out_pad
    torch.cuda.synchronize()
    dig = np.frombuffer(b"".join(it.digest for it in items), np.uint8) if use_digests else None
    siz = np.array([it.size for it in items], np.uint64) if use_sizes else None
    oo, kinds, status, timing = gpu.blob_decode_device(t.data_ptr() + lead, offs, out.data_ptr() + olead, cap, crypt=cfg,
                                                       expect_digests=dig, expect_sizes=siz, hip_stream=hip_stream)
    torch.cuda.synchronize()
    img = out.cpu().numpy()
    end = olead + int(oo[-1])
    assert int(oo[0]) == 0 and int(oo[-1]) <= cap
    pays = [img[olead + int(oo[i]):olead + int(oo[i + 1])].tobytes() for i in range(len(items))]
    return Decoded(pays, oo, kinds, status, bool(torch.equal(t, before)),
                   bool((img[:olead] == FILL_OUT).all() and (img[end:] == FILL_OUT).all()), timing)


def where(it: Item, at: int) -> str:
    """Payload byte `at` of an item, in the opening kernel's terms (encrypted kinds)."""
    n = len(it.payload)
    return g.where(n, at + EHDR) if it.kind in (2, 3) else f"byte {at} of {n} (64 KiB piece {at // g.SEG})"


def mismatches(items, dec: Decoded) -> list:
    """One line per item whose outcome differs from the wanted one: label, first differing
    byte, and for the encrypted kinds its GCM block, segment, row and lane."""
    bad_ = []
    exp_off = np.concatenate([[0], np.cumsum([len(it.payload) for it in items])])
    if [int(x) for x in dec.offsets] != [int(x) for x in exp_off]:
        i = next(i for i, (a, b) in enumerate(zip(dec.offsets, exp_off)) if int(a) != int(b))
        bad_.append(f"out_offsets[{i}] = {int(dec.offsets[i])}, wanted {int(exp_off[i])} (after {items[i - 1].label})")
    for it, pay, kind, st in zip(items, dec.payloads, dec.kinds, dec.status):
        if (int(kind), int(st)) != (it.kind, it.status):
            bad_.append(f"{it.label}: kind {int(kind)} status {STATUS_NAMES[int(st)] if int(st) < 8 else int(st)}, "
                        f"wanted kind {it.kind} status {STATUS_NAMES[it.status]}")
        elif pay != it.payload:
            a, b = np.frombuffer(pay, np.uint8), np.frombuffer(it.payload, np.uint8)
            n = min(a.size, b.size)
            d = np.flatnonzero(a[:n] != b[:n])
            at = int(d[0]) if d.size else n
            bad_.append(f"{it.label}: payload differs at byte {at} ({where(it, at)}); {d.size} bytes differ; "
                        f"{len(pay)} bytes, wanted {len(it.payload)}")
    return bad_
