"""zstd frames to inflate, planted on every branch of the reading side (helpers of
test_iplanted_cpu.py, test_gpu_inflate.py and test_sanitize_inflate.py; not a conftest).

The decoder (proxmox-backup_amd/csrc/zstd_dec.h, pbs_inflate.hip, pbs_inflate_host.cpp) must
read what libzstd writes at any level, what this project's encoder writes, and what the format
allows but neither writes on demand.  Three sources:

 * libzstd through ZSTD_CCtx_setParameter (ctypes, the library oracle.libzstd() loads);
 * this project's frames (oracle.zstd_twin_frame: 64 KiB blocks, repeat offsets);
 * hand-assembled frames from the small writer below: raw or RLE literals and all three
   sequence tables in RLE_Mode, so the bitstream holds extra bits only and needs no FSE encoder.

Every frame's wanted bytes come from libzstd alone (oracle.zstd_decompress), never from the code
under test; the hand writer states the bytes it means and test_iplanted_cpu.py checks that
libzstd agrees.

Corrupted frames: each is derived from an intact one; its wanted outcome is what libzstd does
with it on the CPU (judge()): an error -> the status must not be OK; bytes -> the status is OK
with those bytes, unless the label is in RFC_FORBIDDEN_BUT_ACCEPTED (frames RFC 8878 forbids
and libzstd 1.4.8 lets pass).  The list starts with the four labels this corpus
found, each with what the mirror reports.  A frame with a checksum is judged below its header by
libzstd's verdict on the same frame without the field (libzstd verifies it; the decoder consumes
it unverified by contract).  Two cases are outside that rule because the call's contract
names their status: a second frame and a skippable frame are PBS_ZST_UNSUPPORTED (libzstd
decodes concatenated frames; multi-frame payloads are out of scope here).
"""
import ctypes
import random
import struct
from typing import NamedTuple, Optional

import numpy as np

import oracle

OK, BAD_FRAME, TOO_LARGE, UNSUPPORTED = range(4)  # PBS_ZST_*
STATUS_NAMES = ("OK", "BAD_FRAME", "TOO_LARGE", "UNSUPPORTED")
MAGIC = b"\x28\xb5\x2f\xfd"
BLOCK_MAX = 128 * 1024

# label -> RFC 8878 clause: frames the RFC forbids and libzstd 1.4.8 decodes all the same.
_OVERRUN = ("RFC 8878 3.1.1.3.2.1.2 (decoding sequences) and 4.1: the sequence bitstream must be consumed exactly; "
            "reading past its first bit is corruption.  libzstd 1.4.8 checks the stream only before it decodes a "
            "sequence, so the last one may read zeros from before the stream's start")
_OFFSET_0 = ("RFC 8878 3.1.1.5 (repeat offsets): offset code 3 with a literal length of 0 means Repeated_Offset1 - 1, "
             "and an offset of 0 is corrupted data; libzstd 1.4.8 turns it into offset 1 and goes on")
RFC_FORBIDDEN_BUT_ACCEPTED = {
    # block 1 holds one sequence; the flip changes a bit of its first state, and the extra bits of the code it now
    # names need one bit more than the stream holds.  The host mirror reports BAD_FRAME from decode_sequences'
    # check after the extra bits (the reader's position is -1) with the 131 072 bytes of block 0 produced
    "mixture/flip-block1-seq-last": _OVERRUN,
    # the block that set a repeat offset is read as a raw block, so the history holds 1 where it held 9 / 17 / 40; the
    # mirror reports BAD_FRAME at the first sequence whose "repeat 1 minus 1" is 0, after 227 / 227 / 226 bytes
    "hand-repeat-codes/flip-block0-header-bit2": _OFFSET_0,
    "hand-repeat-codes/flip-block1-header-bit2": _OFFSET_0,
    "hand-repeat-codes/flip-block2-header-bit2": _OFFSET_0,
}

# labels whose status the contract of pbs_zstd_inflate_device names (see the module text)
UNSUPPORTED_BY_CONTRACT = ("second-frame", "skippable-frame")


class Item(NamedTuple):
    label: str
    frame: bytes
    cap: int                  # the slot handed to the decoder
    want: Optional[bytes]     # content, or None: the status must not be OK
    status: Optional[int]     # the exact status where the contract names it, else None
    family: str               # "libzstd", "twin", "hand", "bad"


# ---- libzstd with parameters ---------------------------------------------------------------
_P = {"level": 100, "windowLog": 101, "minMatch": 105, "contentSizeFlag": 200, "checksumFlag": 201}


def zstd_compress(data: bytes, **params) -> bytes:
    L = oracle.libzstd()
    if not hasattr(L, "_cctx_ready"):
        sz, p = ctypes.c_size_t, ctypes.c_void_p
        L.ZSTD_createCCtx.restype = p
        L.ZSTD_createCCtx.argtypes = []
        L.ZSTD_freeCCtx.restype = sz
        L.ZSTD_freeCCtx.argtypes = [p]
        L.ZSTD_CCtx_setParameter.restype = sz
        L.ZSTD_CCtx_setParameter.argtypes = [p, ctypes.c_int, ctypes.c_int]
        L.ZSTD_compress2.restype = sz
        L.ZSTD_compress2.argtypes = [p, p, sz, p, sz]
        L._cctx_ready = True
    c = L.ZSTD_createCCtx()
    try:
        for k, v in params.items():
            r = L.ZSTD_CCtx_setParameter(c, _P[k], int(v))
            assert not L.ZSTD_isError(r), (k, v, L.ZSTD_getErrorName(r))
        cap = L.ZSTD_compressBound(len(data)) + 64
        dst = ctypes.create_string_buffer(cap)
        r = L.ZSTD_compress2(c, dst, cap, data, len(data))
        assert not L.ZSTD_isError(r), L.ZSTD_getErrorName(r)
        return dst.raw[:r]
    finally:
        L.ZSTD_freeCCtx(c)


def judge(frame: bytes, cap: int) -> Optional[bytes]:
    """What libzstd does with `frame` and a destination of `cap` bytes: the content, or None
    for an error.  Both of its decoders must accept: ZSTD_decompress, and the streaming one
    that `decode_all` (data_blob.rs:214) drives, which also enforces the window limit."""
    try:
        a = oracle.zstd_decompress(frame, cap)
        b = oracle.zstd_decode_stream(frame, 1 << 17)
    except ValueError:
        return None
    assert a == b, "libzstd's two decoders disagree"
    return a


# ---- sources ----------------------------------------------------------------------------------
def _rng(seed):
    return random.Random(seed)


def text(n: int, seed: int = 1, vocab: int = 400) -> bytes:
    r = _rng(seed)
    words = [bytes(r.choices(b"abcdefghijklmnopqrstuvwxyzETAOIN", k=r.randint(2, 10))) for _ in range(vocab)]
    out = bytearray()
    while len(out) < n:
        out += r.choice(words) + (b" " if r.random() < 0.9 else b".\n")
    return bytes(out[:n])


def noise(n: int, seed: int, alphabet: bytes = None) -> bytes:
    r = _rng(seed)
    if alphabet is None:
        return r.randbytes(n)
    return bytes(r.choices(alphabet, k=n))


def sparse_matches(n: int, seed: int) -> bytes:
    """Noise with a short copy of earlier bytes every few hundred bytes."""
    r = _rng(seed)
    out = bytearray(r.randbytes(2000))
    while len(out) < n:
        out += r.randbytes(r.randint(150, 600))
        src = len(out) - r.randint(100, min(len(out), 60_000))
        out += out[src:src + r.randint(8, 40)]
    return bytes(out[:n])


def libzstd_items():
    t300 = text(300_000, 1)
    out = []

    def add(label, data, **params):
        out.append(Item(label, zstd_compress(data, **params), len(data), data, OK, "libzstd"))

    for lvl in (-5, 1, 3, 19):
        add(f"text300k-L{lvl}", t300, level=lvl)
    add("text300k-L1-nosize", t300, level=1, contentSizeFlag=0)  # copy_encode's shape: window descriptor
    add("text5k-wlog10-nosize", text(5_000, 2), level=1, windowLog=10, contentSizeFlag=0)
    add("text200k-wlog17-nosize", text(200_000, 3), level=3, windowLog=17, contentSizeFlag=0)
    add("text40k-checksum", text(40_000, 4), level=1, checksumFlag=1)
    add("noise4-minmatch3", noise(20_000, 5, b"acgt"), level=1, minMatch=3)
    add("noise4-low-bytes", noise(20_000, 14, bytes(range(4))), level=1)  # a 2-byte tree: direct weights
    add("noise3-single-stream", noise(900, 6, b"xyz"), level=1)
    add("noise3-long", noise(60_000, 7, b"xyz"), level=3)
    add("periodic", (b"0123456789abcdefghijklm" * 3000)[:65_000], level=1)
    two = text(260_000, 8, vocab=3000)
    add("two-copies-L19", two + two, level=19)
    add("sparse-matches-L9", sparse_matches(400_000, 15), level=9)    # few sequences per block: Repeat_Mode
    add("sparse-matches-L19", sparse_matches(300_000, 16), level=19)
    add("zeros", bytes(300_000), level=1)
    add("random", noise(150_000, 9), level=1)
    add("mixture", text(70_000, 10) + bytes(140_000) + noise(135_000, 11) + text(90_000, 12) + bytes(7), level=1)
    add("vmimage", oracle.gen_vmimage(400_000, 13).tobytes(), level=1)
    add("len0", b"", level=1)
    add("len1", b"q", level=1)
    add("len0-nosize", b"", level=1, contentSizeFlag=0)
    return out


def twin_items():
    out = []
    for label, data in (("twin-text", text(150_000, 20)), ("twin-mixture", text(30_000, 21) + bytes(70_000) + noise(40_000, 22)),
                        ("twin-vmimage", oracle.gen_vmimage(200_000, 23).tobytes()), ("twin-len0", b""),
                        ("twin-len1", b"z"), ("twin-periodic", b"abcabcabd" * 9000)):
        out.append(Item(label, oracle.zstd_twin_frame(data), len(data), data, OK, "twin"))
    return out


# ---- the hand writer ----------------------------------------------------------------------------
LL_BASE = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 18, 20, 22, 24, 28, 32, 40, 48, 64, 128, 256, 512,
           1024, 2048, 4096, 8192, 16384, 32768, 65536]
LL_BITS = [0] * 16 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]
ML_BASE = list(range(3, 35)) + [35, 37, 39, 41, 43, 47, 51, 59, 67, 83, 99, 131, 259, 515, 1027, 2051, 4099, 8195,
                                16387, 32771, 65539]
ML_BITS = [0] * 32 + [1, 1, 1, 1, 2, 2, 3, 3, 4, 4, 5, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16]


def frame_header(content: Optional[int], fcs_bytes: int = 0, window_log: int = 17) -> bytes:
    """fcs_bytes 0: no content size, a window descriptor; 1: single segment; 2, 4, 8: with a
    window descriptor."""
    if fcs_bytes == 0:
        return MAGIC + bytes([0x00, (window_log - 10) << 3])
    if fcs_bytes == 1:
        assert content < 256
        return MAGIC + bytes([0x20, content])
    flag = {2: 1, 4: 2, 8: 3}[fcs_bytes]
    v = content - 256 if fcs_bytes == 2 else content
    return MAGIC + bytes([flag << 6, (window_log - 10) << 3]) + v.to_bytes(fcs_bytes, "little")


def block_header(last: bool, btype: int, size: int) -> bytes:
    return struct.pack("<I", (1 if last else 0) | btype << 1 | size << 3)[:3]


def literals_section(lit: bytes, rle: bool = False, size_format: Optional[int] = None) -> bytes:
    """Raw literals, or RLE ones (`lit` is then one byte repeated); size_format 0 / 2: one
    header byte (5 bits), 1: two (12 bits), 3: three (20 bits); None: the smallest."""
    n = len(lit)
    if rle:
        assert lit == lit[:1] * n and n > 0
    if size_format is None:
        size_format = 0 if n < 32 else 1 if n < 4096 else 3
    t = 1 if rle else 0
    if size_format in (0, 2):
        assert n < 32
        h = bytes([t | size_format << 2 | n << 3])
    elif size_format == 1:
        assert n < 4096
        h = struct.pack("<H", t | 1 << 2 | n << 4)
    else:
        h = struct.pack("<I", t | 3 << 2 | n << 4)[:3]
    return h + (lit[:1] if rle else lit)


def nbseq_field(n: int, three: bool = False) -> bytes:
    if three or n >= 0x7F00:
        assert n >= 0x7F00
        return b"\xff" + struct.pack("<H", n - 0x7F00)
    if n < 128:
        return bytes([n])
    return bytes([128 + (n >> 8), n & 255])


def sequences_section(seqs, ll_code: int, of_code: int, ml_code: int, three: bool = False) -> bytes:
    """`seqs`: (ll, ml, offset_value) triples whose codes are the three given ones (RLE_Mode for
    all three tables: one symbol each, zero state bits).  offset_value is the coded value:
    1-3 the repeat codes, offset + 3 above."""
    if not seqs:
        return b"\x00"
    acc, nb = 0, 0
    for ll, ml, ov in reversed(seqs):  # the decoder reads backwards: the last sequence goes in first
        for v, base, bits in ((ll, LL_BASE[ll_code], LL_BITS[ll_code]), (ml, ML_BASE[ml_code], ML_BITS[ml_code]),
                              (ov, 1 << of_code, of_code)):
            assert 0 <= v - base < (1 << bits) or (bits == 0 and v == base), (v, base, bits)
            acc |= (v - base) << nb
            nb += bits
    acc |= 1 << nb  # the end mark
    stream = acc.to_bytes(nb // 8 + 1, "little")
    modes = 1 << 6 | 1 << 4 | 1 << 2
    return nbseq_field(len(seqs), three) + bytes([modes, ll_code, of_code, ml_code]) + stream


class Sim:
    """What the frame means: the sequences executed with the repeat-offset rule."""

    def __init__(self):
        self.out = bytearray()
        self.rep = [1, 4, 8]

    def block(self, lit: bytes, seqs):
        at = 0
        for ll, ml, ov in seqs:
            self.out += lit[at:at + ll]
            at += ll
            r = self.rep
            if ov > 3:
                off = ov - 3
                self.rep = [off, r[0], r[1]]
            else:
                idx = ov - 1 + (1 if ll == 0 else 0)
                if idx == 0:
                    off = r[0]
                else:
                    off = r[idx] if idx < 3 else r[0] - 1
                    self.rep = [off, r[0], r[1]] if idx != 1 else [off, r[0], r[2]]
            assert 0 < off <= len(self.out), (off, len(self.out))
            for _ in range(ml):
                self.out.append(self.out[-off])
        self.out += lit[at:]


def compressed_block(sim: Sim, last: bool, lit: bytes, seqs, codes, rle_lit=False, size_format=None, three=False):
    sim.block(lit, seqs)
    body = literals_section(lit, rle_lit, size_format) + sequences_section(seqs, *codes, three=three)
    assert len(body) <= BLOCK_MAX
    return block_header(last, 2, len(body)) + body


def hand_items():
    out = []

    def emit(label, blocks_fn, fcs_bytes=0, window_log=17):
        sim = Sim()
        body = blocks_fn(sim)
        content = bytes(sim.out)
        frame = frame_header(len(content), fcs_bytes, window_log) + body
        out.append(Item("hand-" + label, frame, len(content), content, OK, "hand"))

    r = _rng(77)
    # literal size formats, raw and RLE; the content-size widths ride along
    for sf, n, fcs in ((0, 9, 1), (2, 31, 0), (1, 1000, 2), (3, 5000, 4)):
        lit = r.randbytes(n)
        emit(f"raw-lit-sf{sf}", lambda s, lit=lit, sf=sf: compressed_block(
            s, True, lit, [(len(lit), 20, 4)], (_ll_code(len(lit)), 2, 17), size_format=sf), fcs_bytes=fcs)
        emit(f"rle-lit-sf{sf}", lambda s, n=n, sf=sf: compressed_block(
            s, True, b"\x5a" * n, [(n, 3, 5)], (_ll_code(n), 2, 0), rle_lit=True, size_format=sf))
    # nbSeq encodings: ll 1 + ml 3 with repeat code 1 (rep1 = 1 at the frame's start): no extra bits at all
    for n, three in ((127, False), (128, False), (0x7EFF, False), (0x7F00, False), (32_700, True)):
        lit = r.randbytes(n)
        emit(f"nbseq-{n}", lambda s, lit=lit, n=n, three=three: compressed_block(
            s, True, lit, [(1, 3, 1)] * n, (1, 0, 0), three=three))
    # offsets with match lengths on both sides of each (overlap copies), one block per offset
    for off in (1, 2, 3, 15, 16, 63, 64, 65):
        ov = off + 3
        oc = ov.bit_length() - 1

        def blocks(s, off=off, ov=ov, oc=oc):
            lit = r.randbytes(70)
            b = compressed_block(s, False, lit, [(70, 3, ov)], (_ll_code(70), oc, 0))
            for ml in sorted({3, max(3, off - 1), max(3, off), max(3, off + 1), 2 * off + 1, 34}):
                mc = _ml_code(ml)
                lit = r.randbytes(2)
                b += compressed_block(s, False, lit, [(2, ml, ov)], (2, oc, mc))
            return b + block_header(True, 0, 0)  # and a last block of size 0
        emit(f"offset-{off}", blocks)

    # repeat codes 1, 2, 3 with literal length 0 and > 0
    def rep_blocks(s):
        lit = r.randbytes(200)
        b = compressed_block(s, False, lit[:100], [(100, 5, 40 + 3)], (_ll_code(100), 5, 2))
        b += compressed_block(s, False, lit[100:150], [(50, 5, 17 + 3)], (_ll_code(50), 4, 2))
        b += compressed_block(s, False, lit[150:], [(50, 5, 9 + 3)], (_ll_code(50), 3, 2))
        for ll in (0, 3):
            for ov in (1, 2, 3, 3, 2, 1):
                oc = ov.bit_length() - 1
                b += compressed_block(s, False, r.randbytes(ll), [(ll, 4, ov)], (ll, oc, 1))
        # "repeat 1 minus 1": code 3 with no literals
        b += compressed_block(s, False, b"", [(0, 6, 3), (0, 6, 3)], (0, 1, 3))
        s.out += b"!!!"
        return b + block_header(True, 1, 3) + b"!"  # an RLE block ends the frame
    emit("repeat-codes", rep_blocks)

    # a match of 65 539 + extra bits, ending on the block's last byte, after a raw block
    def long_match(s):
        raw = r.randbytes(300)
        s.out += raw
        b = block_header(False, 0, len(raw)) + raw
        return b + compressed_block(s, True, b"ab", [(2, 65_539 + 12_345, 7 + 3)], (2, 3, 52))
    emit("match-65539", long_match, fcs_bytes=8)

    # a match whose source starts at the frame's byte 0, and one that ends the block
    def from_zero(s):
        lit = r.randbytes(40)
        return compressed_block(s, True, lit, [(40, 40, 40 + 3)], (_ll_code(40), 5, _ml_code(40)))
    emit("source-at-byte-0", from_zero, fcs_bytes=1)

    # literals only (nbSeq 0), then last literals after the sequences
    def lits_only(s):
        b = compressed_block(s, False, r.randbytes(50), [], (0, 0, 0))
        return b + compressed_block(s, True, r.randbytes(30), [(10, 3, 1 + 3)], (10, 2, 0))
    emit("last-literals", lits_only)
    return out


def _ll_code(ll):
    return max(c for c in range(36) if LL_BASE[c] <= ll)


def _ml_code(ml):
    return max(c for c in range(53) if ML_BASE[c] <= ml)


# ---- a block walker (for the corruptions' positions and the feature census) ---------------------
def read_ncount(buf: bytes, at: int):
    """Bytes an FSE table description takes at buf[at:], and its accuracy log."""
    bits = int.from_bytes(buf[at:at + 64], "little")
    pos = 4
    log = (bits & 15) + 5
    remaining, sym = 1 << log, 0
    while remaining > 0 and sym < 256:
        nb = (remaining + 1).bit_length()
        lower = (1 << (nb - 1)) - 1
        threshold = (1 << nb) - 1 - (remaining + 1)
        val = (bits >> pos) & ((1 << nb) - 1)
        if (val & lower) < threshold:
            pos += nb - 1
            val &= lower
        else:
            pos += nb
            if val > lower:
                val -= threshold
        proba = val - 1
        remaining -= abs(proba)
        sym += 1
        if proba == 0:
            while True:
                rep = (bits >> pos) & 3
                pos += 2
                sym += rep
                if rep != 3:
                    break
    return (pos + 7) // 8, log


def walk(frame: bytes):
    """The frame's structure: a dict with the header's fields and positions, and `blocks`, each
    a dict of its fields and the byte positions of its parts.  For intact frames only."""
    assert frame[:4] == MAGIC
    d = frame[4]
    single, fcs_flag, did = (d >> 5) & 1, d >> 6, d & 3
    at = 5
    info = {"descriptor": 4, "single": bool(single), "checksum": bool(d & 4), "window_desc": None, "blocks": [],
            "fields": [5]}
    if not single:
        info["window_desc"] = at
        at += 1
        info["fields"].append(at)
    at += (0, 1, 2, 4)[did]
    fcs_len = (single, 2, 4, 8)[fcs_flag]
    info["fcs_len"] = fcs_len
    at += fcs_len
    info["fields"].append(at)
    while True:
        h = int.from_bytes(frame[at:at + 3], "little")
        last, btype, size = h & 1, (h >> 1) & 3, h >> 3
        b = {"header": at, "type": btype, "size": size, "last": bool(last)}
        info["blocks"].append(b)
        body = at + 3
        info["fields"].append(body)
        if btype == 2:
            _walk_compressed(frame, body, size, b, info["fields"])
        at = body + (1 if btype == 1 else size)
        if last:
            break
    info["end_of_blocks"] = at
    return info


def _walk_compressed(frame, at, size, b, fields):
    end = at + size
    b0 = frame[at]
    lt, sf = b0 & 3, (b0 >> 2) & 3
    b["lit_header"] = at
    b["lit_type"], b["lit_sf"] = lt, sf
    if lt < 2:
        hs = 1 if sf in (0, 2) else 2 if sf == 1 else 3
        regen = int.from_bytes(frame[at:at + hs], "little") >> (3 if hs == 1 else 4)
        body = regen if lt == 0 else 1
        b["streams"] = 0
    else:
        hs = 3 if sf < 2 else sf + 2
        v = int.from_bytes(frame[at:at + hs], "little")
        nbits = 10 if sf < 2 else 14 if sf == 2 else 18
        regen = (v >> 4) & ((1 << nbits) - 1)
        body = v >> (4 + nbits)
        b["streams"] = 1 if sf == 0 else 4
        t = at + hs
        if lt == 2:
            hb = frame[t]
            b["weights"] = t + 1
            b["weights_fse"] = hb < 128
            tree = 1 + (hb if hb < 128 else (hb - 127 + 1) // 2)
            b["huf_stream_mid"] = t + tree + (body - tree) // 2
        else:
            b["huf_stream_mid"] = t + body // 2
    fields.append(at + hs)
    b["regen"] = regen
    at += hs + body
    fields.append(at)
    b["seq_header"] = at
    n = frame[at]
    if n == 0:
        b["nbseq"], b["nbseq_form"] = 0, 1
        return
    if n < 128:
        form = 1
    elif n < 255:
        n, form = ((n - 128) << 8) + frame[at + 1], 2
    else:
        n, form = int.from_bytes(frame[at + 1:at + 3], "little") + 0x7F00, 3
    at += form
    b["nbseq"], b["nbseq_form"] = n, form
    m = frame[at]
    b["modes"] = (m >> 6, (m >> 4) & 3, (m >> 2) & 3)
    at += 1
    fields.append(at)
    for mode in b["modes"]:
        if mode == 1:
            at += 1
        elif mode == 2:
            b.setdefault("ncount", at)
            used, _ = read_ncount(frame, at)
            at += used
    fields.append(at)
    b["seq_stream"] = (at, end - 1)


# ---- corruptions ------------------------------------------------------------------------------------
def _flip(frame: bytes, at: int, bit: int) -> bytes:
    b = bytearray(frame)
    b[at] ^= 1 << bit
    return bytes(b)


def bad_items(good):
    """Corrupted forms of frames of `good`; the wanted outcome of each comes from judge()."""
    out = []
    by = {it.label: it for it in good}

    def add(label, frame, cap, status=None, rule=True, stripped=False):
        # `stripped`: libzstd judges the same frame without its checksum field (it verifies the
        # field; the decoder consumes it unverified by contract)
        want = judge(_without_checksum(frame) if stripped else frame, cap) if rule else None
        out.append(Item(label, frame, cap, want, status, "bad"))

    victims = [by[k] for k in ("text300k-L1-nosize", "noise4-minmatch3", "noise3-single-stream", "two-copies-L19",
                               "mixture", "twin-text", "hand-offset-16", "hand-repeat-codes", "text40k-checksum")]
    for v in victims:
        w = walk(v.frame)
        f, cap = v.frame, v.cap + 64
        # truncation after every header field (the first fields of the first blocks; the frame's end)
        for pos in sorted(set(w["fields"][:14] + [len(f) - 1])):
            if pos < len(f):
                add(f"{v.label}/cut@{pos}", f[:pos], cap)
        add(f"{v.label}/flip-descriptor", _flip(f, 4, 6), cap)
        add(f"{v.label}/reserved-bit", _flip(f, 4, 3), cap)
        add(f"{v.label}/dict-id", _with_dict_id(f), cap, status=UNSUPPORTED)
        # every block header; the flips inside a block for the first three blocks.  Below the header
        # of a frame with a checksum, libzstd's verdict is taken on the frame without the field.
        ck = w["checksum"]
        for i, b in enumerate(w["blocks"]):
            for bit in (1, 2, 9):
                add(f"{v.label}/flip-block{i}-header-bit{bit}", _flip(f, b["header"] + bit // 8, bit % 8), cap, stripped=ck)
            add(f"{v.label}/block{i}-type3", _set_block_type3(f, b["header"]), cap, status=BAD_FRAME)
            if b["type"] != 2 or i >= 3:
                continue
            for bit in (0, 3, 5):
                add(f"{v.label}/flip-block{i}-lit-header-bit{bit}", _flip(f, b["lit_header"], bit), cap, stripped=ck)
            if "weights" in b:
                add(f"{v.label}/flip-block{i}-weights", _flip(f, b["weights"], 5), cap, stripped=ck)
                add(f"{v.label}/flip-block{i}-weights-b", _flip(f, b["weights"] + 1, 2), cap, stripped=ck)
            if "huf_stream_mid" in b:
                add(f"{v.label}/flip-block{i}-huf-mid", _flip(f, b["huf_stream_mid"], 4), cap, stripped=ck)
            if "ncount" in b:
                add(f"{v.label}/flip-block{i}-ncount", _flip(f, b["ncount"], 5), cap, stripped=ck)
                add(f"{v.label}/flip-block{i}-ncount-b", _flip(f, b["ncount"] + 1, 1), cap, stripped=ck)
            if "seq_stream" in b:
                s0, s1 = b["seq_stream"]
                add(f"{v.label}/flip-block{i}-seq-first", _flip(f, s0, 2), cap, stripped=ck)
                add(f"{v.label}/flip-block{i}-seq-last", _flip(f, s1, 0), cap, stripped=ck)
        if w["window_desc"] is not None:
            big = bytearray(f)
            big[w["window_desc"]] = (28 - 10) << 3  # Window_Log 28: 256 MiB
            add(f"{v.label}/window-log-28", bytes(big), cap, status=UNSUPPORTED)
        add(f"{v.label}/slot-one-short", f, v.cap - 1, status=TOO_LARGE) if v.cap else None
        add(f"{v.label}/trailing-byte", f + b"\x00", cap, status=BAD_FRAME)
        add(f"{v.label}/second-frame", f + by["len1"].frame, cap, status=UNSUPPORTED, rule=False)
        add(f"{v.label}/skippable-frame", b"\x50\x2a\x4d\x18\x04\x00\x00\x00abcd" + f, cap, status=UNSUPPORTED, rule=False)
    return out


def _with_dict_id(frame: bytes) -> bytes:
    d = frame[4]
    assert d & 3 == 0
    at = 5 + (0 if d & 0x20 else 1)
    return frame[:4] + bytes([d | 1]) + frame[5:at] + b"\x07" + frame[at:]


def _without_checksum(frame: bytes) -> bytes:
    """The same frame with the Content_Checksum flag cleared and the 4-byte field dropped."""
    return frame[:4] + bytes([frame[4] & ~4]) + frame[5:-4]


def _set_block_type3(frame: bytes, at: int) -> bytes:
    b = bytearray(frame)
    b[at] |= 6
    return bytes(b)


# ---- the corpus -----------------------------------------------------------------------------------
_corpus = None


def corpus():
    """Every item, intact ones first: {"good": [...], "bad": [...]} (built once)."""
    global _corpus
    if _corpus is None:
        good = libzstd_items() + twin_items() + hand_items()
        _corpus = {"good": good, "bad": bad_items(good)}
    return _corpus


def interleaved():
    """All items in one list, every bad frame between two intact neighbours."""
    c = corpus()
    small = [it for it in c["good"] if len(it.frame) < 4096]
    out = list(c["good"])
    for i, b in enumerate(c["bad"]):
        out.append(b)
        out.append(small[i % len(small)])
    return out


def check(it: Item, status: int, got: bytes) -> Optional[str]:
    """None when (status, bytes produced) obeys the rule for `it`, else what is wrong."""
    name = STATUS_NAMES[status] if status < 4 else str(status)
    if it.status is not None and it.want is None and status != it.status:
        return f"{it.label}: status {name}, wanted {STATUS_NAMES[it.status]}"
    if it.want is None:
        return None if status != OK else f"{it.label}: status OK where libzstd fails"
    if it.label in RFC_FORBIDDEN_BUT_ACCEPTED:
        return None if status != OK or got == it.want else f"{it.label}: OK with other bytes than libzstd's"
    if status != OK:
        return f"{it.label}: status {name} where libzstd returns {len(it.want)} bytes"
    if got != it.want:
        return f"{it.label}: {len(got)} bytes differ from libzstd's {len(it.want)}"
    return None


def layout(items, pad: int = 0, out_pad: int = 0, guard: int = 256):
    """Frames back to back after `pad` bytes; slots back to back after `out_pad` bytes, each of
    its item's cap, with `guard` bytes behind the last: (data, frame_offsets, out_offsets,
    output size)."""
    foff = np.zeros(len(items) + 1, dtype=np.uint64)
    ooff = np.zeros(len(items) + 1, dtype=np.uint64)
    foff[0], ooff[0] = pad, out_pad
    for i, it in enumerate(items):
        foff[i + 1] = foff[i] + np.uint64(len(it.frame))
        ooff[i + 1] = ooff[i] + np.uint64(it.cap)
    data = np.frombuffer(bytes(pad) + b"".join(it.frame for it in items), dtype=np.uint8)
    return data, foff, ooff, int(ooff[-1]) + guard
