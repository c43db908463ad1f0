"""Chunks whose matches, literals and sizes sit on the zstd blob encoder's own boundaries
(helpers of test_zplanted_cpu.py and test_gpu_zplanted.py; not a conftest).

The encoder (proxmox-backup_amd/csrc/pbs_zstd.hip) parses a 64 KiB block as eight
sub-blocks, one wave and one hash table each, and its entropy stage changes path at a
handful of sizes.  The geometry below restates those values once, each with the symbol
it restates; test_zplanted_cpu.py pins the seam table and the window to the host twin's behaviour
(oracle/zstd_twin.cpp), so a change of either fails there first.

Every case is (label, chunk, predicate).  The predicate is evaluated on the CPU against the
twin's parse (oracle.zstd_twin_parse) or the twin's frame (oracle.zstd_twin_frame, read by
walk_frame below) and states the feature the case exists for; a case whose predicate is
false fails test_zplanted_cpu.py -- none is skipped or dropped.

What the twin finds depends on which positions its sampled rounds visit and on which
history positions are still in the 4096-entry table, so a recipe names its free value (a
source position, a seed, a length) and FOUND fixes the value at which the twin shows the
feature.  `python tests/zplanted.py search` recomputes the table (deterministic: the first
candidate in a fixed order).

Sampling rules used by the recipes (zstd_twin.cpp parse(); pbs_zstd.hip parse_subblock):
  * a sub-block's first round samples every `step` = min(hs, 8) bytes, hs = 2 without
    history and 8 after 3 KiB of history without repeats; a round without a match doubles
    the step, a round with one is followed by a round at step 1;
  * the history before a sub-block enters the table from the window start wlo every 2 bytes
    for 1 KiB, every 4 for 2 KiB, then every 8: a source at an odd distance from wlo is
    never a table candidate;
  * a `helper` -- a match that runs past its round's end to 32 bytes before the feature --
    makes the next round start there at step 1, so every position of the feature is sampled.
"""
import os
import sys
from typing import Callable, NamedTuple

import numpy as np

KiB = 1024
# ---- geometry (pbs_zstd.hip unless stated) -------------------------------------------
BLOCK = 64 * KiB                  # zstd_enc.h kEncBlock
ZSUB_DELTA = 768                  # PBS_ZSUB_DELTA
ZSUB_A, ZSUB_B = 8192 + ZSUB_DELTA, 8192 - ZSUB_DELTA  # kZSubA / kZSubB


def sub_start(w: int) -> int:     # zsub_start
    return w * ZSUB_A if w <= 4 else 4 * ZSUB_A + (w - 4) * ZSUB_B


SEAMS = tuple(sub_start(w) for w in range(1, 8))  # 8960 17920 26880 35840 43264 50688 58112
ZHIST = 16384                     # kZHist: bytes of the previous block staged
ZROUND, ZCAP, ZMIN, ZMAXSTEP, ZBACK = 256, 32, 5, 8, 8  # kZRound, kZCap, kZMin, kZMaxStep, kZBack
ZWIN = 12288                      # PBS_ZWIN -> kZWin
ZSUBSEQ = ZSUB_A // ZMIN + 2      # kZSubSeq
HUFSTREAMS = 48 * KiB             # kHufStreams
HUFMAX = 11                       # kHufMax
ZRUNS = 64                        # kZRuns
ESTREAMS = 36 * KiB + 512         # kEStreams
ZEXT_LANE, ZEXT_STEP = 16, 1024   # parse_subblock's capped match: 16 bytes per lane, 64 lanes a step
# header-size thresholds (RFC 8878; the writers in zstd_twin.cpp)
FCS_EDGES = (256, 65536 + 256)    # frame content size in 1 / 2 / 4 bytes (frame_header)
SEQ_COUNT_EDGE = 128              # sequence count in 1 / 2 bytes (sequences)
RAW_LIT_EDGES = (32, 4096)        # raw / RLE literals header 1 / 2 / 3 bytes (raw_literals)
HUF_LIT_EDGES = (1024, 16384)     # coded literals header 3 / 4 / 5 bytes (literals)
HUF_FOUR = 256                    # four streams from 256 literals (literals)
assert SEAMS == (8960, 17920, 26880, 35840, 43264, 50688, 58112) and sub_start(8) == BLOCK


# ---- the frame walker (RFC 8878 3.1; reads the format, decodes nothing) ----------------

def walk_frame(frame: bytes) -> dict:
    """{header_len, content_size, blocks: [{last, type, size, lit, nseq, modes, huf0}]} of a
    single-segment frame.  `lit` = {type, fmt, regen, comp, streams} (type 0 raw, 1 RLE,
    2 Huffman); `huf0` the first byte of the Huffman tree description; `modes` = (LL, OF, ML)
    each 0 predefined, 1 RLE, 2 FSE-compressed; lit / nseq / modes only for compressed blocks."""
    f = bytes(frame)
    assert f[:4] == b"\x28\xb5\x2f\xfd", f[:4]
    fhd = f[4]
    assert fhd & 0x20 and not fhd & 0x03, hex(fhd)  # single segment, no dictionary id
    fl = fhd >> 6
    nb = (1, 2, 4, 8)[fl]
    size = int.from_bytes(f[5:5 + nb], "little") + (256 if fl == 1 else 0)
    o = 5 + nb
    out = {"header_len": o, "content_size": size, "blocks": []}
    while True:
        h = int.from_bytes(f[o:o + 3], "little")
        o += 3
        b = {"last": h & 1, "type": (h >> 1) & 3, "size": h >> 3, "lit": None, "nseq": None, "modes": None,
             "huf0": None}
        assert b["type"] != 3
        body = 1 if b["type"] == 1 else b["size"]
        if b["type"] == 2:
            p = o
            t, fmt = f[p] & 3, (f[p] >> 2) & 3
            if t < 2:
                if fmt in (0, 2):  # one byte: bit 3 belongs to the size; reported as format 0
                    regen, hl, fmt = f[p] >> 3, 1, 0
                elif fmt == 1:
                    regen, hl = int.from_bytes(f[p:p + 2], "little") >> 4, 2
                else:
                    regen, hl = int.from_bytes(f[p:p + 3], "little") >> 4, 3
                comp, streams = (regen if t == 0 else 1), 0
            else:
                hl, bits = ((3, 10), (3, 10), (4, 14), (5, 18))[fmt]
                v = int.from_bytes(f[p:p + hl], "little") >> 4
                regen, comp = v & ((1 << bits) - 1), v >> bits
                streams = 1 if fmt == 0 else 4
                b["huf0"] = f[p + hl]
            b["lit"] = {"type": t, "fmt": fmt, "regen": regen, "comp": comp, "streams": streams}
            p += hl + comp
            n0 = f[p]
            if n0 < 128:
                ns, p = n0, p + 1
            elif n0 < 255:
                ns, p = ((n0 - 128) << 8) + f[p + 1], p + 2
            else:
                ns, p = f[p + 1] + (f[p + 2] << 8) + 0x7F00, p + 3
            b["nseq"] = ns
            if ns:
                b["modes"] = (f[p] >> 6, (f[p] >> 4) & 3, (f[p] >> 2) & 3)
            assert p <= o + body
        o += body
        out["blocks"].append(b)
        if b["last"]:
            break
    assert o == len(f), (o, len(f))
    return out


def huf_streams_bytes(blk: dict) -> int:
    """Bytes of the Huffman streams of a compressed block's literals: the compressed size less
    the tree description and the jump table (what pbs_zstd.hip compares with kEStreams and
    kHufStreams)."""
    h0 = blk["huf0"]
    desc = 1 + h0 if h0 < 128 else 1 + (h0 - 127 + 1) // 2
    return blk["lit"]["comp"] - desc - (6 if blk["lit"]["streams"] == 4 else 0)


# ---- the twin's view of a chunk ----------------------------------------------------------

class View:
    """What the predicates read: the twin's frame, its walk and the parse of each block."""

    def __init__(self, oracle, chunk: np.ndarray):
        self.o, self.chunk, self._f, self._w, self._p = oracle, chunk, None, None, {}

    @property
    def frame(self) -> bytes:
        if self._f is None:
            self._f = self.o.zstd_twin_frame(self.chunk.tobytes())
        return self._f

    @property
    def walk(self) -> dict:
        if self._w is None:
            self._w = walk_frame(self.frame)
        return self._w

    def parse(self, b: int = 0) -> list:
        """[(pos, ml, off)] of block b (block positions)."""
        if b not in self._p:
            c = self.chunk
            s = self.o.zstd_twin_parse(c[b * BLOCK:(b + 1) * BLOCK].tobytes(), c[:b * BLOCK].tobytes())
            self._p[b] = [tuple(int(x) for x in r) for r in s]
        return self._p[b]

    def with_off(self, off: int, b: int = 0) -> list:
        return [(p, m) for p, m, o in self.parse(b) if o == off]

    def literals(self, b: int = 0) -> np.ndarray:
        blk = self.chunk[b * BLOCK:(b + 1) * BLOCK]
        keep = np.ones(blk.size, bool)
        for p, m, _ in self.parse(b):
            keep[p:p + m] = False
        return blk[keep]

    def per_sub(self, b: int = 0) -> list:
        n = [0] * 8
        for p, _, _ in self.parse(b):
            n[max(w for w in range(8) if sub_start(w) <= p)] += 1
        return n


class Recipe(NamedTuple):
    """make(x) -> chunk and pred(view, x) -> bool; x = FOUND[label], searched among `cands`
    (None: the recipe has no free value and x is None)."""
    label: str
    what: str                       # the feature, in words
    make: Callable
    pred: Callable
    cands: object = None            # candidates in search order, or measure(view) -> x
    key: object = None              # FOUND's key when the label holds the value


class Case(NamedTuple):
    label: str
    chunk: np.ndarray
    what: str
    pred: Callable[[View], bool]


def _case(r: Recipe) -> Case:
    key = r.key or r.label
    if r.cands is not None and key not in FOUND:
        raise AssertionError(f"no constant for {key}: run python tests/zplanted.py search")
    x = FOUND[key] if r.cands is not None else None
    return Case(r.label, np.ascontiguousarray(r.make(x), dtype=np.uint8), r.what, lambda v, r=r, x=x: bool(r.pred(v, x)))


# ---- backgrounds and plants --------------------------------------------------------------

def bg(n: int, seed: int, syms: int = 64) -> np.ndarray:
    """n seeded bytes uniform over `syms` symbols: 64 leave no 5-byte repeat to find (30 bits)
    and code to 6 bits each, so a block of them is a compressed one with Huffman literals (a
    full 64 KiB of them passes kHufStreams and stays raw)."""
    return np.random.default_rng(seed).integers(0, syms, n, dtype=np.uint8)


def plant(buf: np.ndarray, m: int, q: int, L: int) -> None:
    """buf[m:m+L] = buf[q:q+L], the bytes either side made to differ from the source's (the
    match is L bytes, neither longer forwards nor backwards)."""
    assert 0 <= q and q + L <= m and m + L <= buf.size, (q, m, L, buf.size)
    buf[m:m + L] = buf[q:q + L]
    if q > 0 and buf[m - 1] == buf[q - 1]:
        buf[m - 1] ^= 1
    if m + L < buf.size and buf[m + L] == buf[q + L]:
        buf[m + L] ^= 1


def quiet_rounds(w: int, first_block: bool = True) -> list:
    """Round starts of sub-block w (block positions) while no match is found."""
    r, step, out = sub_start(w), (2 if first_block and w == 0 else 8), []
    while r < sub_start(w + 1):
        out.append(r)
        r, step = r + ZROUND * step, min(2 * step, ZMAXSTEP)
    return out


def helper(buf: np.ndarray, w: int, before: int, base: int = 0, first_block: bool = True, hd: int = 4096) -> int:
    """A match (offset hd) of sub-block w that starts at a sampled position 256 bytes before a
    quiet round's end and runs past it to `before` - 32: the next round starts where it ends
    and samples every position of the 256 bytes from there (a step-1 round lasts 256 bytes;
    after one without a match the step doubles again).  Returns the helper's block position."""
    end = before - 32
    rs = [r for r in quiet_rounds(w, first_block) if r <= end]
    assert len(rs) >= 2, (w, before)
    hp = rs[-1] - 256
    plant(buf, base + hp, base + hp - hd, end - hp)
    return hp


def _only(v: View, off: int, want, b: int = 0) -> bool:
    return sorted(v.with_off(off, b)) == sorted(want)


def _untouched(v: View, m: int, L: int, b: int = 0) -> bool:
    return all(p + ml <= m or p >= m + L for p, ml, _ in v.parse(b))


def _visible(v: View) -> bool:
    """Every block with sequences is a compressed block whose sequence count is the parse's:
    the parse shows in the frame's bytes."""
    for b, blk in enumerate(v.walk["blocks"]):
        n = len(v.parse(b))
        if n and (blk["type"] != 2 or blk["nseq"] != n):
            return False
    return True


# ---- a. seams ------------------------------------------------------------------------

SEAM_L = (5, 12, 33, 300)
SEAM_PLACES = (("start", "-L/2"), ("start", "-1"), ("start", "0"), ("end", "-L/2"), ("end", "-1"), ("end", "0"))


def _seam_geometry(w: int, L: int, kind: str, d: str):
    seam = SEAMS[w - 1]
    delta = -(L // 2) if d == "-L/2" else int(d)
    m = seam + delta if kind == "start" else seam + delta - L
    a = max(0, min(m + L, seam) - m)  # bytes before the seam
    want = ([(m, a)] if a >= ZMIN else []) + ([(max(m, seam), L - a)] if L - a >= ZMIN else [])
    return seam, m, want


def _src_cands(seam: int):
    lo = max(0, seam - ZWIN) + 8
    return [(q, hd) for hd in (4096, 4160, 4224) for q in range(lo, lo + 2048)]


def seam_recipes():
    """a. For each seam w a match of L bytes that starts or ends at seam + {-L/2, -1, 0}: the
    part before the seam (sub-block w - 1, found in a step-1 round) and the part after it
    (sub-block w, found at its first position) are each one sequence with the planted offset
    when they hold kZMin bytes, and literals otherwise."""
    for w in range(1, 8):
        for kind, d in SEAM_PLACES:
            for L in sorted(SEAM_L, reverse=True):
                seam, m, want = _seam_geometry(w, L, kind, d)
                label = f"a/seam{w}/{kind}{d}/L{L}"

                def make(x, w=w, L=L, seam=seam, m=m):
                    buf = bg(max(seam, m + L) + 40, 1000 + w)
                    helper(buf, w - 1, m, hd=x[1])
                    plant(buf, m, x[0], L)
                    return buf

                if want:
                    yield Recipe(label, f"sequences {want} with the planted offset, split at seam {seam}", make,
                                 lambda v, x, m=m, want=want: _only(v, m - x[0], want) and _visible(v), _src_cands(seam))
                else:  # neither part holds kZMin bytes: the source of the 12-byte sibling, which is found
                    sib = f"a/seam{w}/{kind}{d}/L12"
                    yield Recipe(label, f"no sequence touches the {L} planted bytes at {m} (parts under kZMin)",
                                 lambda _, make=make, sib=sib: make(FOUND[sib]),
                                 lambda v, _, m=m, L=L, sib=sib: _untouched(v, m, L) and not v.with_off(m - FOUND[sib][0]))


# ---- b. window edge ------------------------------------------------------------------

WINDOW_SUBS = tuple((0, w) for w in range(2, 8)) + ((1, 0), (1, 1))  # (block, sub-block) with a full window


def window_recipes():
    """b. A 24-byte match at the first position of a sub-block whose source lies kZWin - 1,
    kZWin and kZWin + 1 bytes back (and, because odd distances from the window start are
    never table candidates, also kZWin - 2 and kZWin + 2).  The window is a bound on the
    SOURCE: at kZWin + 2 the match is found from the sub-block's third byte on, where its
    source is the window's first byte.  kZWin - 1 at the first position cannot be a table
    candidate; its case plants 2144 bytes with a run of equal bytes in them, which gives the
    sub-block's first round a match and so a step-1 round that finds the offset."""
    for blk, w in WINDOW_SUBS:
        s0, pos, L = blk * BLOCK + sub_start(w), sub_start(w), 24
        seeds = range(2000 + 16 * (8 * blk + w), 2000 + 16 * (8 * blk + w) + 16)
        tag = f"b/blk{blk}sub{w}"

        syms = 48 if blk else 64  # (a full block of 64 symbols stays raw: the blob would be the uncompressed one)

        def make(seed, d, s0=s0, L=L, syms=syms):
            buf = bg(s0 + L + 40, seed, syms)
            plant(buf, s0, s0 - d, L)
            return buf

        def make_long(seed, s0=s0, syms=syms):
            L2, d = 2144, ZWIN - 1
            buf = bg(s0 + L2 + 40, seed, syms)
            buf[s0 - d + 7:s0 - d + 15] = 5
            plant(buf, s0, s0 - d, L2)
            return buf

        yield Recipe(f"{tag}/d=kZWin", f"sequence ({pos}, {L}) at offset kZWin", lambda s, make=make: make(s, ZWIN),
                     lambda v, s, blk=blk, pos=pos, L=L: (pos, L) in v.with_off(ZWIN, blk) and _visible(v), seeds)
        yield Recipe(f"{tag}/d=kZWin-2", f"sequence ({pos}, {L}) at offset kZWin - 2", lambda s, make=make: make(s, ZWIN - 2),
                     lambda v, s, blk=blk, pos=pos, L=L: (pos, L) in v.with_off(ZWIN - 2, blk) and _visible(v), seeds)
        yield Recipe(f"{tag}/d=kZWin-1", "a sequence at offset kZWin - 1 that ends where the planted bytes end", make_long,
                     lambda v, s, blk=blk, pos=pos: any(p + m == pos + 2144 for p, m in v.with_off(ZWIN - 1, blk))
                     and _visible(v), seeds)
        sib = f"{tag}/d=kZWin"
        yield Recipe(f"{tag}/d=kZWin+1", "no sequence at offset kZWin + 1 (the seed at which kZWin is found)",
                     lambda _, make=make, sib=sib: make(FOUND[sib], ZWIN + 1),
                     lambda v, _, blk=blk, pos=pos, L=L: not v.with_off(ZWIN + 1, blk) and _untouched(v, pos, L, blk))
        yield Recipe(f"{tag}/d=kZWin+2", f"sequence ({pos + 2}, {L - 2}) at offset kZWin + 2: the source starts at the window",
                     lambda s, make=make: make(s, ZWIN + 2),
                     lambda v, s, blk=blk, pos=pos, L=L: v.with_off(ZWIN + 2, blk) == [(pos + 2, L - 2)] and _visible(v), seeds)


# ---- c. extension --------------------------------------------------------------------

EXT_LENGTHS = (ZMIN - 1, ZMIN, ZMIN + 1, ZCAP - 1, ZCAP, ZCAP + 1, ZCAP + ZEXT_LANE - 1, ZCAP + ZEXT_LANE, ZCAP + ZEXT_LANE + 1,
               ZCAP + 255, ZCAP + 256, ZCAP + 257, ZCAP + ZEXT_STEP - 1, ZCAP + ZEXT_STEP, ZCAP + ZEXT_STEP + 1)
EXT_BACK = (0, 1, 7, 8, 9)
_EXT_M = SEAMS[0] + 1024  # a sampled position of sub-block 1's first round (step 8)
_OFFS8 = tuple(range(4096, 4096 + 8 * 24, 8))


def hash5(b) -> int:
    """The table hash of 5 bytes (pbs_zstd.hip hash5, zstd_twin.cpp hash5)."""
    w = int.from_bytes(bytes(b[:4]), "little")
    return ((((w * 2654435761) & 0xFFFFFFFF) ^ ((int(b[4]) * 2246822519) & 0xFFFFFFFF)) >> 20) & 0xFFF


def _shadow(buf: np.ndarray, at: int, victim: int, seed: int) -> None:
    """5 bytes at `at` (a later history position) with the table hash of the 5 bytes at
    `victim` and other content: the table keeps the last position per hash, so `victim` is
    no candidate any more."""
    rng, want = np.random.default_rng(seed), hash5(buf[victim:victim + 5])
    for _ in range(1 << 16):
        c = rng.integers(0, 64, 5, dtype=np.uint8)
        if hash5(c) == want and bytes(c) != bytes(buf[victim:victim + 5]):
            buf[at:at + 5] = c
            return
    raise AssertionError("no shadow bytes")


def extension_recipes():
    """c. Match lengths around kZMin, kZCap and the capped match's forward extension (16
    bytes per lane, 1024 bytes a step, the walk of pbs_zstd.hip parse_subblock; 256 past the cap as well);
    matches that run to the sub-block, block and chunk end; backward extension of 0, 1, 7, 8
    and 9 bytes before a sampled hit (capped at kZBack; the position 8 bytes earlier is kept
    out of the table by a later position with the same hash), and one stopped by the
    previous match's end."""
    m = _EXT_M
    for L in sorted(EXT_LENGTHS, reverse=True):
        def make(d, L=L):
            buf = bg(m + L + 40, 3000)
            plant(buf, m, m - d, L)
            return buf
        if L >= ZMIN:
            yield Recipe(f"c/len{L}", f"one sequence ({m}, {L})", make,
                         lambda v, d, L=L: _only(v, d, [(m, L)]) and _visible(v), _OFFS8)
        else:
            yield Recipe(f"c/len{L}", f"no sequence on {L} equal bytes (under kZMin)",
                         lambda _, make=make: make(FOUND["c/len5"]),
                         lambda v, _, L=L: _untouched(v, m, L) and not v.with_off(FOUND["c/len5"]))
    seam = SEAMS[1]

    def make_sub(d):
        buf = bg(seam + 200 + 40, 3001)
        plant(buf, seam - 200, seam - 200 - d, 400)
        return buf
    yield Recipe("c/to-subblock-end", f"a capped match cut at the sub-block end {seam}, the rest a second sequence", make_sub,
                 lambda v, d: _only(v, d, [(seam - 200, 200), (seam, 200)]) and _visible(v), _OFFS8)

    def make_blk(d):
        buf = bg(BLOCK + 200 + 40, 3002)
        plant(buf, BLOCK - 200, BLOCK - 200 - d, 400)
        return buf
    yield Recipe("c/to-block-end", "a capped match cut at the block end, the rest the next block's first sequence", make_blk,
                 lambda v, d: _only(v, d, [(BLOCK - 200, 200)]) and _only(v, d, [(0, 200)], 1) and _visible(v), _OFFS8)

    def make_end(d):
        buf = bg(m + 203, 3003)
        plant(buf, m, m - d, 203)
        return buf
    yield Recipe("c/to-chunk-end", "a capped match that runs to the chunk's last byte", make_end,
                 lambda v, d: _only(v, d, [(m, 203)]) and _visible(v), _OFFS8)
    p = m + 64
    for k in EXT_BACK:
        e = min(k, ZBACK)

        def make_back(d, k=k):
            buf = bg(p + 20 + 40, 3004)
            if k >= ZBACK:
                _shadow(buf, 8000, p - d - 8, 3005)
            plant(buf, p - k, p - d - k, 20 + k)
            return buf
        yield Recipe(f"c/back{k}", f"a hit sampled at {p} starts {e} bytes earlier", make_back,
                     lambda v, d, e=e: _only(v, d, [(p - e, 20 + e)]) and _visible(v), _OFFS8)

    def make_prev(x):
        da, d = x
        buf = bg(p + 20 + 40, 3006)
        plant(buf, p - 24, p - 24 - da, 21)       # ends at p - 3
        plant(buf, p, p - d, 20)
        buf[p - d - 7:p - d] = buf[p - 7:p]       # the 7 bytes before p equal the source's
        return buf
    yield Recipe("c/back-stops-at-previous-match", f"7 equal bytes before the hit at {p}, the previous match ends at {p - 3}",
                 make_prev, lambda v, x: _only(v, x[0], [(p - 24, 21)]) and _only(v, x[1], [(p - 3, 23)]) and _visible(v),
                 [(da, d) for da in (5120, 5128, 5136) for d in _OFFS8])


# ---- d. repeat codes -----------------------------------------------------------------

def rep_events(seqs) -> list:
    """(literal length, index of the offset in the running repeat history or None) per
    sequence; the history per sub-block and updated as RFC 8878 3.1.1.5 says."""
    out, rep, end, sub = [], [0, 0, 0], 0, -1
    for pos, ml, off in seqs:
        s = max(w for w in range(8) if sub_start(w) <= pos)
        if s != sub:
            sub, rep = s, [0, 0, 0]
        ll = pos - end
        which = next((j for j in range(3) if rep[j] == off), None)
        if which == 0 and ll == 0:
            which = None  # with no literals the first entry cannot be named
        out.append((ll, which))
        if which is None:
            rep = [off, rep[0], rep[1]]
        elif which:
            rep = [off] + [r for j, r in enumerate(rep) if j != which]
        end = pos + ml
    return out


def repeat_recipes():
    """d. Matches back to back (no literals) and one literal apart that alternate between two
    and rotate among three offsets: each sequence's offset is the second (two offsets) or
    third (three) entry of the repeat history."""
    m0, n = _EXT_M, 12
    for nof, which in ((2, 1), (3, 2)):
        for ll in (0, 1):
            def make(seed, nof=nof, ll=ll):
                buf = bg(m0 + 16 * n + 40, seed)
                for i in range(n):
                    d = (4096, 5120, 6144)[i % nof]
                    buf[m0 + 16 * i:m0 + 16 * i + 16 - ll] = buf[m0 + 16 * i - d:m0 + 16 * i - d + 16 - ll]
                return buf

            def pred(v, seed, ll=ll, which=which):
                s = v.parse()
                ev = rep_events(s)
                adj = [i for i in range(1, len(s)) if s[i][0] == s[i - 1][0] + s[i - 1][1] + ll and ev[i] == (ll, which)]
                return len(s) == n and len(adj) >= n - nof - 1 and _visible(v)
            yield Recipe(f"d/{nof}offsets/ll{ll}", f"{n} sequences {ll} literals apart, offsets the repeat history's entry {which + 1}",
                         make, pred, range(4000, 4040))
    m = SEAMS[1] - 200

    def make_del(d):  # 32 source bytes with the 16th left out: two matches, the second one byte nearer
        buf = bg(m + 31 + 40, 4100)
        helper(buf, 1, m)
        s = m - d
        buf[m:m + 15], buf[m + 15:m + 31] = buf[s:s + 15], buf[s + 16:s + 32]
        return buf
    yield Recipe("d/rep0-1", "two sequences back to back, the second's offset the first's less one (repeat code 3 at ll == 0)",
                 make_del, lambda v, d: [x for x in v.parse() if x[0] >= m] == [(m, 15, d), (m + 15, 16, d - 1)] and _visible(v),
                 _OFFS8)


# ---- e. ends -------------------------------------------------------------------------

END_DELTAS = (-1, 0, 1, 4, 5)


def _end_chunk(w: int, n: int, x) -> np.ndarray:
    """n bytes whose last 8 are a copy from x[0], found in a step-1 round (helper offset x[1]);
    48 symbols when the chunk reaches the block end, so that the block's literals stay coded."""
    buf = bg(n, 5000 + w, 48 if w == 8 else 64)
    helper(buf, w - 1, n - 8, hd=x[1])
    plant(buf, n - 8, x[0], 8)
    return buf


def end_recipes():
    """e. One-block chunks that end seam + {-1, 0, 1, 4, 5} (and block end + {-1, 0}), the last
    8 bytes a copy (the guards P + kZMin <= N and s0 < N): the part before the seam is a
    sequence when it holds kZMin bytes, the part after it only when the chunk still holds
    kZMin bytes there.  Chunks of 64 KiB + 1..6: the first block ends in such a copy (a
    sequence that ends on the block's last byte, in a compressed block), the second block's
    bytes are a copy too -- a block of 2 to 6 bytes is always a raw one (one sequence alone
    takes 6 bytes), so what shows of it in the frame is its raw header behind a compressed
    block.  Chunks of 1..6 bytes, and the frame-content-size widths."""
    for w in range(1, 9):
        seam = sub_start(w)
        for delta in (END_DELTAS if w < 8 else (-1, 0)):
            n = seam + delta
            a = min(n, seam) - (n - 8)
            want = ([(n - 8, a)] if a >= ZMIN else []) + ([(seam, 8 - a)] if 8 - a >= ZMIN else [])
            label = f"e/seam{w}{delta:+d}"
            if want:
                yield Recipe(label, f"chunk of {n} bytes, its last 8 a copy: sequences {want}",
                             lambda x, w=w, n=n: _end_chunk(w, n, x),
                             lambda v, x, n=n, want=want: _only(v, n - 8 - x[0], want) and _visible(v), _src_cands(seam))
            else:
                sib = f"e/seam{w}+0"
                yield Recipe(label, f"chunk of {n} bytes, its last 8 a copy split 4 + 4 by the seam: no sequence there",
                             lambda _, w=w, n=n, sib=sib: _end_chunk(w, n, FOUND[sib]),
                             lambda v, _, n=n: _untouched(v, n - 8, 8) and _visible(v))
    for n in range(1, 7):
        yield Recipe(f"e/len{n}", f"a chunk of {n} distinct bytes: one raw block (one byte: RLE)",
                     lambda _, n=n: np.arange(17, 17 + n, dtype=np.uint8),
                     lambda v, _, n=n: [b["type"] for b in v.walk["blocks"]] == [0 if n > 1 else 1] and v.walk["header_len"] == 6)
        yield Recipe(f"e/len{n}-same", f"a chunk of {n} equal bytes: one RLE block", lambda _, n=n: np.full(n, 9, np.uint8),
                     lambda v, _: [b["type"] for b in v.walk["blocks"]] == [1])
    for k in range(1, 7):
        def make_tail(d, k=k):
            buf = np.concatenate([_end_chunk(8, BLOCK, FOUND["e/seam8+0"]), np.zeros(k, np.uint8)])
            buf[BLOCK:] = buf[BLOCK - d:BLOCK - d + k]
            return buf

        def pred(v, d, k=k):
            b0, b1 = v.walk["blocks"]
            return (v.parse(1) == ([(0, k, d)] if k >= ZMIN else []) and len(v.frame) < BLOCK + k
                    and b0["type"] == 2 and b0["nseq"] == len(v.parse(0)) and v.parse(0)[-1][:2] == (BLOCK - 8, 8)
                    and (b1["type"], b1["size"]) == (0 if k > 1 else 1, k))  # (one byte: an RLE block)
        if k >= ZMIN:
            yield Recipe(f"e/block+{k}", f"a compressed block whose last sequence ends on its last byte, then {k} bytes "
                         "that parse as one sequence and are written raw", make_tail, pred, _OFFS8)
        else:
            yield Recipe(f"e/block+{k}", f"a compressed block whose last sequence ends on its last byte, then {k} raw "
                         "bytes without a sequence (under kZMin)",
                         lambda _, make_tail=make_tail: make_tail(FOUND["e/block+5"]),
                         lambda v, _, pred=pred: pred(v, FOUND["e/block+5"]))
    for n, hl in ((FCS_EDGES[0] - 1, 6), (FCS_EDGES[0], 7), (FCS_EDGES[0] + 1, 7), (FCS_EDGES[1] - 1, 7), (FCS_EDGES[1], 9)):
        yield Recipe(f"e/fcs{n}", f"frame header of {hl} bytes", lambda _, n=n: bg(n, 5300),
                     lambda v, _, n=n, hl=hl: v.walk["header_len"] == hl and v.walk["content_size"] == n)


# ---- f. sequence counts --------------------------------------------------------------

SEQ_COUNTS = (0, 1, ZRUNS - 1, ZRUNS, ZRUNS + 1, SEQ_COUNT_EDGE - 1, SEQ_COUNT_EDGE)


def dense_block() -> np.ndarray:
    """Sub-block 0 background, every later sub-block 5-byte copies back to back: each from a
    position 260 to 400 bytes back (every position of a step-1 round is in the table, and few
    later ones have displaced it yet), the sub-block's first ones from even positions of the
    last 2 KiB before it, and each chosen so that the copy cannot run into a sixth byte."""
    buf, rng = bg(BLOCK, 6100), np.random.default_rng(6101)
    for w in range(1, 8):
        s0, stop = sub_start(w), None
        for p in range(s0, min(sub_start(w + 1), BLOCK - 4), ZMIN):
            for _ in range(100):
                s = 2 * int(rng.integers((s0 - 2048) // 2, (s0 - 16) // 2)) if p - s0 < 408 else p - int(rng.integers(260, 400))
                if stop is None or buf[s] != stop:
                    break
            buf[p:p + 5] = buf[s:s + 5]
            stop = buf[s + 5]
    return buf


def count_recipes():
    """f. Blocks with exactly 0, 1, kZRuns - 1 .. kZRuns + 1, 127 and 128 sequences (16-byte
    copies 320 apart, as many planted as it takes), and the densest block the builder makes:
    5-byte matches back to back in sub-blocks 1-7."""
    for k in SEQ_COUNTS:
        def make(x, k=k):
            seed, planted = x
            buf = bg(BLOCK, seed, 48)
            for i in range(planted):
                plant(buf, _EXT_M + 320 * i, _EXT_M + 320 * i - 4096, 16)
            return buf
        yield Recipe(f"f/nseq{k}", f"a compressed block of exactly {k} sequences", make,
                     lambda v, x, k=k: len(v.parse()) == k and v.walk["blocks"][0]["type"] == 2
                     and v.walk["blocks"][0]["nseq"] == k,
                     [(seed, planted) for seed in (6000, 6001, 6002) for planted in range(k, min(k + 40, 170))])
    got = FOUND.get("f/dense", ())
    yield Recipe("f/dense/" + "-".join(str(c) for c in got), f"sequences per sub-block {got} (capacity kZSubSeq = {ZSUBSEQ})",
                 lambda _: dense_block(),
                 lambda v, x: tuple(v.per_sub()) == tuple(x) and max(x) <= ZSUBSEQ and max(x) >= 1400 and _visible(v),
                 lambda v: tuple(v.per_sub()), key="f/dense")


# ---- g. literals sections ------------------------------------------------------------

def punched(runs, lit, seed: int, piece: int = 10, lead: int = 2064, d: int = 8192, off16: bool = False) -> np.ndarray:
    """Two blocks.  Block 0 is background; every byte of block 1 copies the byte d before it,
    except the literal runs: sub-block by sub-block, after `lead` copied bytes (one match past
    the first round, which sets the repeat offset), runs of the given lengths `piece` copied
    bytes apart, each literal byte other than the byte it would copy.  Then the block's
    literals are exactly the runs: the matches between them are repeat-offset candidates in
    step-1 rounds and need no table entry.  off16: no literal at a block position divisible by 16
    (the positions of the encoder's first, sampled literal estimate)."""
    buf = np.concatenate([bg(BLOCK, seed), np.zeros(BLOCK, np.uint8)])
    lit = np.asarray(lit, dtype=np.uint8)
    runs, ri, li, at = list(runs), 0, 0, BLOCK

    def copy(a, e):
        nonlocal at
        assert a == at and e - a <= d
        buf[a:e] = buf[a - d:e - d]
        at = e
    for w in range(8):
        s0, se = BLOCK + sub_start(w), BLOCK + sub_start(w + 1)
        copy(s0, s0 + lead)
        while ri < len(runs) and at + runs[ri] + piece <= se:
            r = runs[ri]
            seg = lit[li:li + r].copy()
            same = seg == buf[at - d:at - d + r]
            if (same.any() and lit.min() == lit.max()) or (off16 and (-at) % 16 < r):
                # a constant literal where it would copy itself (or a sampled position): one byte on
                copy(at, at + 1)
                continue
            seg[same] ^= 1
            buf[at:at + r] = seg
            at, ri, li = at + r, ri + 1, li + r
            copy(at, at + piece)
        while at < se:
            copy(at, min(se, at + d))
    assert ri == len(runs), (ri, len(runs))
    return buf


def _runs(n: int, r: int) -> list:
    return [r] * (n // r) + ([n % r] if n % r else [])


def _lit_is(v: View, typ: int, fmt: int, n: int, b: int = 1) -> bool:
    lit = v.walk["blocks"][b]["lit"]
    return lit is not None and (lit["type"], lit["fmt"], lit["regen"]) == (typ, fmt, n) and _visible(v)


def _huf_depth(counts) -> int:
    """Depth of the unlimited Huffman code of a histogram."""
    import heapq
    h = [(int(c), i, 0) for i, c in enumerate(counts) if c]
    heapq.heapify(h)
    k = len(h)
    while len(h) > 1:
        a, b = heapq.heappop(h), heapq.heappop(h)
        heapq.heappush(h, (a[0] + b[0], k, max(a[2], b[2]) + 1))
        k += 1
    return h[0][2]


def stream_block(L: int, seed: int = 7200) -> np.ndarray:
    """One block: L bytes uniform over 64 symbols (6-bit codes: 3/4 byte of Huffman stream
    each), the rest copies of the bytes 8192 before."""
    buf = np.concatenate([bg(L, seed, 64), np.zeros(BLOCK - L, np.uint8)])
    for a in range(L, BLOCK, 8192):
        e = min(BLOCK, a + 8192)
        buf[a:e] = buf[a - 8192:e - 8192]
    return buf


def literal_recipes():
    """g. The literals section at every size-format edge -- raw and RLE at 31/32 and
    4095/4096 literals, Huffman at 255/256 (one stream / four), 1023/1024 and 16383/16384 --
    the Huffman streams at kEStreams, kEStreams + 1 and kHufStreams bytes and the first raw
    result past it, RLE literals beside matches, alphabets whose tree description is direct
    or FSE-coded, and a Fibonacci histogram whose unlimited code is deeper than kHufMax."""
    seeds = [(seed, d) for d in (8192, 8200, 8208, 8216) for seed in range(7000, 7016)]
    rng = np.random.default_rng(7001)
    raw, skew = rng.integers(0, 256, 20000, dtype=np.uint8), rng.integers(0, 16, 20000, dtype=np.uint8) * 7
    for n in (RAW_LIT_EDGES[0] - 1, RAW_LIT_EDGES[0], RAW_LIT_EDGES[1] - 1, RAW_LIT_EDGES[1]):
        fmt = 0 if n < RAW_LIT_EDGES[0] else 1 if n < RAW_LIT_EDGES[1] else 3
        yield Recipe(f"g/raw{n}", f"{n} raw literals, size format {fmt}", lambda s, n=n: punched(_runs(n, 4), raw, s[0], d=s[1]),
                     lambda v, s, n=n, fmt=fmt: _lit_is(v, 0, fmt, n), seeds)
        yield Recipe(f"g/rle{n}", f"{n} RLE literals beside matches, size format {fmt}"
                     + (" (none at a sampled position: 32 to 64 sampled literals of one byte stay raw)" if n < 64 else ""),
                     lambda s, n=n: punched(_runs(n, 2), np.full(n, 0xFF, np.uint8), s[0], d=s[1], off16=n < 64),
                     lambda v, s, n=n, fmt=fmt: _lit_is(v, 1, fmt, n), seeds)
    for n, fmt in ((HUF_FOUR - 1, 0), (HUF_FOUR, 1), (HUF_LIT_EDGES[0] - 1, 1), (HUF_LIT_EDGES[0], 2),
                   (HUF_LIT_EDGES[1] - 1, 2), (HUF_LIT_EDGES[1], 3)):
        yield Recipe(f"g/huf{n}", f"{n} Huffman-coded literals, size format {fmt} ({1 if fmt == 0 else 4} streams)",
                     lambda s, n=n: punched(_runs(n, 8), skew, s[0], d=s[1]), lambda v, s, n=n, fmt=fmt: _lit_is(v, 2, fmt, n), seeds)

    def streams(v, L=None):
        """Huffman stream bytes of the block (of stream_block(L)); BLOCK when the literals are not coded."""
        blk = (v if L is None else View(v.o, stream_block(L))).walk["blocks"][0]
        return huf_streams_bytes(blk) if blk["type"] == 2 and blk["lit"]["type"] == 2 else BLOCK
    for name, target in (("kEStreams", ESTREAMS), ("kHufStreams", HUFSTREAMS)):
        around = range(target * 4 // 3 - 40, min(BLOCK, target * 4 // 3 + 40))
        yield Recipe(f"g/streams<={name}", f"the largest Huffman streams at or under {target} bytes: a literal more passes it",
                     stream_block, lambda v, L, target=target: streams(v) <= target < streams(v, L + 1), around)
        yield Recipe(f"g/streams>{name}", f"the smallest Huffman streams over {target} bytes" if target == ESTREAMS else
                     "the first literal count past kHufStreams: the 7-byte copy is not found, all 65536 bytes are literals, "
                     "their streams would pass kHufStreams, they stay raw and so does the block",
                     stream_block, lambda v, L, target=target: streams(v, L - 1) <= target < streams(v)
                     and (streams(v) == BLOCK) == (target == HUFSTREAMS), around)

    def alphabet(k):
        return np.random.default_rng(7300 + k).permutation(np.repeat(np.arange(k, dtype=np.uint8) if k < 256 else
                                                                     np.arange(256).astype(np.uint8), 512 if k == 2 else 32))
    for k, direct in ((2, True), (128, True), (129, False), (256, False)):
        def make_alpha(_, k=k):
            a = alphabet(k)
            if k == 256:  # uniform bytes would stay raw: skew them
                a = np.minimum(a, np.random.default_rng(7399).integers(0, 256, a.size)).astype(np.uint8)
                a[:256] = np.arange(256)
            return a
        yield Recipe(f"g/alphabet{k}", f"Huffman weights {'direct' if direct else 'FSE-coded'}", make_alpha,
                     lambda v, _, direct=direct, k=k: v.walk["blocks"][0]["type"] == 2
                     and v.walk["blocks"][0]["lit"]["type"] == 2 and (v.walk["blocks"][0]["huf0"] >= 128) == direct
                     and np.unique(v.literals()).size == k)

    def fib(_):
        f = [1, 1]
        while len(f) < 22:
            f.append(f[-1] + f[-2])
        return np.random.default_rng(7400).permutation(np.repeat(np.arange(22, dtype=np.uint8) * 11, f))
    yield Recipe("g/fibonacci", "a literal histogram whose unlimited Huffman code is deeper than kHufMax", fib,
                 lambda v, _: v.walk["blocks"][0]["lit"]["type"] == 2
                 and _huf_depth(np.bincount(v.literals(), minlength=256)) > HUFMAX)


# ---- h. sequence table modes ---------------------------------------------------------

def mode_recipes():
    """h. Blocks whose LL / OF / ML tables are all predefined (few, varied sequences), all RLE
    (four sequences with one code each) and all FSE-compressed (hundreds of sequences with two
    codes each)."""
    def few(d):
        buf = bg(30000, 8000)
        for i, (m, L) in enumerate(((9984, 16), (10400, 40), (12000, 7), (14504, 100), (20000, 23), (27000, 64))):
            plant(buf, m, m - d - 264 * i * i, L)
        return buf
    yield Recipe("h/predefined", "mode byte: LL, OF and ML predefined", few,
                 lambda v, d: v.walk["blocks"][0]["modes"] == (0, 0, 0) and len(v.parse()) == 6, _OFFS8)

    def rle(seed):
        buf = bg(34648 + 40, seed)
        for i, m in enumerate((9984, 18200, 26416, 34632)):
            plant(buf, m, m - 4096 - 8 * i, 16)
        return buf
    yield Recipe("h/rle", "mode byte: LL, OF and ML RLE", rle,
                 lambda v, s: v.walk["blocks"][0]["modes"] == (1, 1, 1) and len(v.parse()) == 4, range(8100, 8120))
    lits = np.random.default_rng(8200).integers(0, 16, 4000, dtype=np.uint8)
    yield Recipe("h/fse", "mode byte: LL, OF and ML FSE-compressed",
                 lambda s: punched(_runs(900, 1) + _runs(1200, 3), lits, s),
                 lambda v, s: v.walk["blocks"][1]["modes"] == (2, 2, 2), range(8200, 8212))


# ---- i. shorter or not ---------------------------------------------------------------

def shorter_recipes():
    """i. 1000-byte chunks -- a random head, then k zero bytes -- whose frame is n + 1, n and
    n - 1 bytes: only the last becomes a compressed blob."""
    n = 1000

    def make(k):
        return np.concatenate([np.random.default_rng(9000).integers(0, 256, n - k, dtype=np.uint8), np.zeros(k, np.uint8)])
    for name, size in (("n+1", n + 1), ("n", n), ("n-1", n - 1)):
        yield Recipe(f"i/frame={name}", f"a frame of {size} bytes for a chunk of {n}", make,
                     lambda v, k, size=size: len(v.frame) == size, range(6, 64))


# ---- j. alignment --------------------------------------------------------------------

def alignment_recipes():
    """j. One chunk of two blocks and a tail (matches across the block starts, literal runs,
    zeros), which the GPU test encodes at all 16 start residues."""
    def make(seed):
        rng = np.random.default_rng(seed)
        buf = np.concatenate([punched(_runs(1500, 5), rng.integers(0, 32, 1500, dtype=np.uint8), seed), bg(777, seed + 1)])
        buf[2 * BLOCK + 300:2 * BLOCK + 700] = buf[2 * BLOCK - 8192 + 300:2 * BLOCK - 8192 + 700]
        buf[2 * BLOCK + 720:] = 0
        return buf
    yield Recipe("j/two-blocks-and-tail", "three blocks, the second and third with matches into the block before",
                 make, lambda v, s: len(v.parse(1)) > 100 and len(v.parse(2)) >= 2 and _visible(v), range(9500, 9510))


FAMILIES = {"a": seam_recipes, "b": window_recipes, "c": extension_recipes, "d": repeat_recipes, "e": end_recipes,
            "f": count_recipes, "g": literal_recipes, "h": mode_recipes, "i": shorter_recipes, "j": alignment_recipes}


_recipes = {}


def recipes(family: str) -> dict:
    if family not in _recipes:
        _recipes[family] = {r.label: r for r in FAMILIES[family]()}
    return _recipes[family]


def labels(family: str) -> list:
    return list(recipes(family))


def cases(family: str) -> list:
    return [_case(r) for r in recipes(family).values()]


def case(label: str) -> Case:
    return _case(recipes(label[0])[label])


# ---- the GPU side (test_gpu_zplanted.py) ---------------------------------------------

PAD, GUARD = 5, 4096
RESIDUES = tuple(range(16))


def layout_chunks(chunks):
    """The chunks back to back: (data, bounds)."""
    data = np.concatenate([np.zeros(0, np.uint8)] + list(chunks))
    return data, np.concatenate([[0], np.cumsum([c.size for c in chunks])]).astype(np.uint64)


def layout_spans(chunk: np.ndarray, pad: int = PAD):
    """Family j: 16 copies of the chunk, one at each residue mod 16 of its start address (the
    buffer starts `pad` bytes into its allocation), gaps of 1 to 23 bytes before them -- gap i
    is 1 + 7 i mod 23, or the next length in 1..23 that gives a residue not yet taken -- and
    the spans listed in reverse order: (data, spans, labels' residues)."""
    parts, spans, at, seen = [], [], 0, set()
    for i in range(16):
        gap = next(g for g in ((7 * i + j) % 23 + 1 for j in range(23)) if (pad + at + g) % 16 not in seen)
        seen.add((pad + at + gap) % 16)
        parts += [np.full(gap, 0xEE, np.uint8), chunk]
        spans.append((at + gap, at + gap + chunk.size))
        at += gap + chunk.size
    gaps = [spans[0][0]] + [spans[i][0] - spans[i - 1][1] for i in range(1, 16)]
    assert len(seen) == 16 and min(gaps) >= 1 and max(gaps) <= 23 and len(set(gaps)) >= 8, gaps
    spans = spans[::-1]
    return np.concatenate(parts), np.asarray(spans, dtype=np.uint64), [(pad + s) % 16 for s, _ in spans]


def span_labels(label: str, residues) -> list:
    return [f"{label}/residue{r}" for r in residues]


def gpu_encode(gpu, torch, data: np.ndarray, bounds=None, spans=None, pad: int = PAD):
    """One encode call over a device buffer that starts `pad` bytes into its allocation, into
    a zero-filled output with a guard tail: (blob bytes per chunk, crcs, comp, guard untouched)."""
    t = torch.zeros(pad + data.size, dtype=torch.uint8, device="cuda")
    t[pad:] = torch.from_numpy(data).to("cuda")
    if spans is None:
        cap = gpu.blob_stream_bound(bounds)
    else:
        cap = sum(gpu.blob_stream_bound(np.asarray([0, int(e - s)], np.uint64)) for s, e in spans)
    out = torch.zeros(cap + GUARD, dtype=torch.uint8, device="cuda")
    if spans is None:
        offs, crcs, comp, _ = gpu.blob_encode_chunks_device(t.data_ptr() + pad, data.size, bounds, out.data_ptr(), cap)
    else:
        offs, crcs, comp, _ = gpu.blob_encode_spans_device(t.data_ptr() + pad, data.size, spans, out.data_ptr(), cap)
    torch.cuda.synchronize()
    img = out.cpu().numpy()
    blobs = [img[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(len(offs) - 1)]
    return blobs, crcs, comp, not img[cap:].any()


def gpu_encode_family(gpu, torch, family: str):
    """(labels, chunks, gpu_encode's result) of one family: one call over all its chunks."""
    cs = cases(family)
    if family == "j":
        data, spans, res = layout_spans(cs[0].chunk)
        return span_labels(cs[0].label, res), [cs[0].chunk] * len(spans), gpu_encode(gpu, torch, data, spans=spans)
    data, bounds = layout_chunks([c.chunk for c in cs])
    return [c.label for c in cs], [c.chunk for c in cs], gpu_encode(gpu, torch, data, bounds=bounds)


def search(oracle, families=None) -> dict:
    """FOUND anew: per recipe the first candidate at which the twin shows the feature."""
    for fam in families or sorted(FAMILIES):
        for r in FAMILIES[fam]():
            key = r.key or r.label
            if r.cands is None:
                continue
            if callable(r.cands):
                FOUND[key] = r.cands(View(oracle, r.make(None)))
                continue
            FOUND.pop(key, None)
            for x in r.cands:
                if r.pred(View(oracle, np.ascontiguousarray(r.make(x))), x):
                    FOUND[key] = x
                    break
            else:
                raise AssertionError(f"{r.label}: no candidate shows the feature ({r.what})")
    return FOUND


# (python tests/zplanted.py search)
FOUND = {
    'f/dense': (0, 1253, 1610, 1618, 1312, 1329, 1348, 1340), 'a/seam1/start-L/2/L300': (8, 4096),
    'a/seam1/start-L/2/L33': (8, 4096), 'a/seam1/start-L/2/L12': (26, 4096), 'a/seam1/start-1/L300': (9, 4096),
    'a/seam1/start-1/L33': (9, 4096), 'a/seam1/start-1/L12': (9, 4096), 'a/seam1/start0/L300': (8, 4096),
    'a/seam1/start0/L33': (8, 4096), 'a/seam1/start0/L12': (8, 4096), 'a/seam1/start0/L5': (8, 4096),
    'a/seam1/end-L/2/L300': (8, 4096), 'a/seam1/end-L/2/L33': (8, 4096), 'a/seam1/end-L/2/L12': (8, 4096),
    'a/seam1/end-L/2/L5': (8, 4096), 'a/seam1/end-1/L300': (8, 4096), 'a/seam1/end-1/L33': (8, 4096),
    'a/seam1/end-1/L12': (8, 4096), 'a/seam1/end-1/L5': (8, 4096), 'a/seam1/end0/L300': (8, 4096),
    'a/seam1/end0/L33': (8, 4096), 'a/seam1/end0/L12': (8, 4096), 'a/seam1/end0/L5': (8, 4096),
    'a/seam2/start-L/2/L300': (5640, 4096), 'a/seam2/start-L/2/L33': (5640, 4096),
    'a/seam2/start-L/2/L12': (5640, 4096), 'a/seam2/start-1/L300': (5641, 4096),
    'a/seam2/start-1/L33': (5641, 4096), 'a/seam2/start-1/L12': (5641, 4096), 'a/seam2/start0/L300': (5640, 4096),
    'a/seam2/start0/L33': (5640, 4096), 'a/seam2/start0/L12': (5640, 4096), 'a/seam2/start0/L5': (5640, 4096),
    'a/seam2/end-L/2/L300': (5640, 4096), 'a/seam2/end-L/2/L33': (5640, 4096), 'a/seam2/end-L/2/L12': (5640, 4096),
    'a/seam2/end-L/2/L5': (5640, 4096), 'a/seam2/end-1/L300': (5640, 4096), 'a/seam2/end-1/L33': (5640, 4096),
    'a/seam2/end-1/L12': (5640, 4096), 'a/seam2/end-1/L5': (5640, 4096), 'a/seam2/end0/L300': (5640, 4096),
    'a/seam2/end0/L33': (5640, 4096), 'a/seam2/end0/L12': (5640, 4096), 'a/seam2/end0/L5': (5640, 4096),
    'a/seam3/start-L/2/L300': (14600, 4096), 'a/seam3/start-L/2/L33': (14600, 4096),
    'a/seam3/start-L/2/L12': (14600, 4096), 'a/seam3/start-1/L300': (14601, 4096),
    'a/seam3/start-1/L33': (14601, 4096), 'a/seam3/start-1/L12': (14601, 4096),
    'a/seam3/start0/L300': (14600, 4096), 'a/seam3/start0/L33': (14600, 4096), 'a/seam3/start0/L12': (14600, 4096),
    'a/seam3/start0/L5': (14600, 4096), 'a/seam3/end-L/2/L300': (14600, 4096), 'a/seam3/end-L/2/L33': (14600, 4096),
    'a/seam3/end-L/2/L12': (14600, 4096), 'a/seam3/end-L/2/L5': (14600, 4096), 'a/seam3/end-1/L300': (14600, 4096),
    'a/seam3/end-1/L33': (14600, 4096), 'a/seam3/end-1/L12': (14600, 4096), 'a/seam3/end-1/L5': (14600, 4096),
    'a/seam3/end0/L300': (14600, 4096), 'a/seam3/end0/L33': (14600, 4096), 'a/seam3/end0/L12': (14600, 4096),
    'a/seam3/end0/L5': (14600, 4096), 'a/seam4/start-L/2/L300': (23560, 4096),
    'a/seam4/start-L/2/L33': (23560, 4096), 'a/seam4/start-L/2/L12': (23568, 4096),
    'a/seam4/start-1/L300': (23561, 4096), 'a/seam4/start-1/L33': (23561, 4096),
    'a/seam4/start-1/L12': (23561, 4096), 'a/seam4/start0/L300': (23560, 4096), 'a/seam4/start0/L33': (23560, 4096),
    'a/seam4/start0/L12': (23560, 4096), 'a/seam4/start0/L5': (23560, 4096), 'a/seam4/end-L/2/L300': (23560, 4096),
    'a/seam4/end-L/2/L33': (23560, 4096), 'a/seam4/end-L/2/L12': (23560, 4096), 'a/seam4/end-L/2/L5': (23560, 4096),
    'a/seam4/end-1/L300': (23560, 4096), 'a/seam4/end-1/L33': (23560, 4096), 'a/seam4/end-1/L12': (23560, 4096),
    'a/seam4/end-1/L5': (23560, 4096), 'a/seam4/end0/L300': (23560, 4096), 'a/seam4/end0/L33': (23560, 4096),
    'a/seam4/end0/L12': (23560, 4096), 'a/seam4/end0/L5': (23560, 4096), 'a/seam5/start-L/2/L300': (30992, 4096),
    'a/seam5/start-L/2/L33': (30992, 4096), 'a/seam5/start-L/2/L12': (31000, 4096),
    'a/seam5/start-1/L300': (30985, 4096), 'a/seam5/start-1/L33': (30985, 4096),
    'a/seam5/start-1/L12': (30985, 4096), 'a/seam5/start0/L300': (30984, 4096), 'a/seam5/start0/L33': (30984, 4096),
    'a/seam5/start0/L12': (30984, 4096), 'a/seam5/start0/L5': (30986, 4096), 'a/seam5/end-L/2/L300': (30992, 4096),
    'a/seam5/end-L/2/L33': (30992, 4096), 'a/seam5/end-L/2/L12': (30993, 4096), 'a/seam5/end-L/2/L5': (31000, 4096),
    'a/seam5/end-1/L300': (30992, 4096), 'a/seam5/end-1/L33': (30992, 4096), 'a/seam5/end-1/L12': (30993, 4096),
    'a/seam5/end-1/L5': (31000, 4096), 'a/seam5/end0/L300': (30992, 4096), 'a/seam5/end0/L33': (30992, 4096),
    'a/seam5/end0/L12': (30993, 4096), 'a/seam5/end0/L5': (31000, 4096), 'a/seam6/start-L/2/L300': (38408, 4096),
    'a/seam6/start-L/2/L33': (38408, 4096), 'a/seam6/start-L/2/L12': (38416, 4096),
    'a/seam6/start-1/L300': (38409, 4096), 'a/seam6/start-1/L33': (38409, 4096),
    'a/seam6/start-1/L12': (38409, 4096), 'a/seam6/start0/L300': (38408, 4096), 'a/seam6/start0/L33': (38408, 4096),
    'a/seam6/start0/L12': (38408, 4096), 'a/seam6/start0/L5': (38410, 4096), 'a/seam6/end-L/2/L300': (38408, 4096),
    'a/seam6/end-L/2/L33': (38408, 4096), 'a/seam6/end-L/2/L12': (38409, 4096), 'a/seam6/end-L/2/L5': (38416, 4096),
    'a/seam6/end-1/L300': (38408, 4096), 'a/seam6/end-1/L33': (38408, 4096), 'a/seam6/end-1/L12': (38409, 4096),
    'a/seam6/end-1/L5': (38416, 4096), 'a/seam6/end0/L300': (38408, 4096), 'a/seam6/end0/L33': (38408, 4096),
    'a/seam6/end0/L12': (38409, 4096), 'a/seam6/end0/L5': (38416, 4096), 'a/seam7/start-L/2/L300': (45832, 4096),
    'a/seam7/start-L/2/L33': (45832, 4096), 'a/seam7/start-L/2/L12': (45832, 4096),
    'a/seam7/start-1/L300': (45833, 4096), 'a/seam7/start-1/L33': (45833, 4096),
    'a/seam7/start-1/L12': (45833, 4096), 'a/seam7/start0/L300': (45832, 4096), 'a/seam7/start0/L33': (45832, 4096),
    'a/seam7/start0/L12': (45832, 4096), 'a/seam7/start0/L5': (45832, 4096), 'a/seam7/end-L/2/L300': (45832, 4096),
    'a/seam7/end-L/2/L33': (45832, 4096), 'a/seam7/end-L/2/L12': (45832, 4096), 'a/seam7/end-L/2/L5': (45832, 4096),
    'a/seam7/end-1/L300': (45832, 4096), 'a/seam7/end-1/L33': (45832, 4096), 'a/seam7/end-1/L12': (45832, 4096),
    'a/seam7/end-1/L5': (45832, 4096), 'a/seam7/end0/L300': (45832, 4096), 'a/seam7/end0/L33': (45832, 4096),
    'a/seam7/end0/L12': (45832, 4096), 'a/seam7/end0/L5': (45832, 4096), 'b/blk0sub2/d=kZWin': 2032,
    'b/blk0sub2/d=kZWin-2': 2032, 'b/blk0sub2/d=kZWin-1': 2032, 'b/blk0sub2/d=kZWin+2': 2032,
    'b/blk0sub3/d=kZWin': 2048, 'b/blk0sub3/d=kZWin-2': 2048, 'b/blk0sub3/d=kZWin-1': 2048,
    'b/blk0sub3/d=kZWin+2': 2048, 'b/blk0sub4/d=kZWin': 2064, 'b/blk0sub4/d=kZWin-2': 2064,
    'b/blk0sub4/d=kZWin-1': 2064, 'b/blk0sub4/d=kZWin+2': 2064, 'b/blk0sub5/d=kZWin': 2080,
    'b/blk0sub5/d=kZWin-2': 2081, 'b/blk0sub5/d=kZWin-1': 2080, 'b/blk0sub5/d=kZWin+2': 2081,
    'b/blk0sub6/d=kZWin': 2096, 'b/blk0sub6/d=kZWin-2': 2096, 'b/blk0sub6/d=kZWin-1': 2096,
    'b/blk0sub6/d=kZWin+2': 2096, 'b/blk0sub7/d=kZWin': 2112, 'b/blk0sub7/d=kZWin-2': 2112,
    'b/blk0sub7/d=kZWin-1': 2112, 'b/blk0sub7/d=kZWin+2': 2114, 'b/blk1sub0/d=kZWin': 2128,
    'b/blk1sub0/d=kZWin-2': 2128, 'b/blk1sub0/d=kZWin-1': 2128, 'b/blk1sub0/d=kZWin+2': 2129,
    'b/blk1sub1/d=kZWin': 2144, 'b/blk1sub1/d=kZWin-2': 2144, 'b/blk1sub1/d=kZWin-1': 2144,
    'b/blk1sub1/d=kZWin+2': 2144, 'c/len1057': 4096, 'c/len1056': 4096, 'c/len1055': 4096, 'c/len289': 4096,
    'c/len288': 4096, 'c/len287': 4096, 'c/len49': 4096, 'c/len48': 4096, 'c/len47': 4096, 'c/len33': 4096,
    'c/len32': 4096, 'c/len31': 4096, 'c/len6': 4096, 'c/len5': 4096, 'c/to-subblock-end': 4096,
    'c/to-block-end': 4096, 'c/to-chunk-end': 4096, 'c/back0': 4096, 'c/back1': 4096, 'c/back7': 4096,
    'c/back8': 4096, 'c/back9': 4096, 'c/back-stops-at-previous-match': (5120, 4096), 'd/2offsets/ll0': 4000,
    'd/2offsets/ll1': 4000, 'd/3offsets/ll0': 4000, 'd/3offsets/ll1': 4000, 'd/rep0-1': 4096,
    'e/seam1-1': (8, 4096), 'e/seam1+0': (8, 4096), 'e/seam1+1': (8, 4096), 'e/seam1+5': (9, 4096),
    'e/seam2-1': (5640, 4096), 'e/seam2+0': (5640, 4096), 'e/seam2+1': (5640, 4096), 'e/seam2+5': (5641, 4096),
    'e/seam3-1': (14600, 4096), 'e/seam3+0': (14600, 4096), 'e/seam3+1': (14600, 4096), 'e/seam3+5': (14601, 4096),
    'e/seam4-1': (23560, 4096), 'e/seam4+0': (23560, 4096), 'e/seam4+1': (23560, 4096), 'e/seam4+5': (23561, 4096),
    'e/seam5-1': (30984, 4096), 'e/seam5+0': (30984, 4096), 'e/seam5+1': (30984, 4096), 'e/seam5+5': (30985, 4096),
    'e/seam6-1': (38408, 4096), 'e/seam6+0': (38408, 4096), 'e/seam6+1': (38408, 4096), 'e/seam6+5': (38409, 4096),
    'e/seam7-1': (45869, 4096), 'e/seam7+0': (45869, 4096), 'e/seam7+1': (45870, 4096), 'e/seam7+5': (45833, 4096),
    'e/seam8-1': (53256, 4096), 'e/seam8+0': (53256, 4096), 'e/block+5': 4096, 'e/block+6': 4096,
    'f/nseq0': (6000, 0), 'f/nseq1': (6000, 1), 'f/nseq63': (6000, 63), 'f/nseq64': (6000, 64),
    'f/nseq65': (6000, 65), 'f/nseq127': (6000, 128), 'f/nseq128': (6000, 129), 'g/raw31': (7002, 8192),
    'g/rle31': (7002, 8192), 'g/raw32': (7002, 8192), 'g/rle32': (7002, 8192), 'g/raw4095': (7000, 8192),
    'g/rle4095': (7010, 8192), 'g/raw4096': (7000, 8192), 'g/rle4096': (7010, 8192), 'g/huf255': (7002, 8192),
    'g/huf256': (7002, 8192), 'g/huf1023': (7002, 8192), 'g/huf1024': (7002, 8192), 'g/huf16383': (7007, 8200),
    'g/huf16384': (7007, 8200), 'g/streams<=kEStreams': 49832, 'g/streams>kEStreams': 49833,
    'g/streams<=kHufStreams': 65528, 'g/streams>kHufStreams': 65529, 'h/predefined': 4096, 'h/rle': 8100,
    'h/fse': 8200, 'i/frame=n+1': 18, 'i/frame=n': 19, 'i/frame=n-1': 20, 'j/two-blocks-and-tail': 9500,
}

if __name__ == "__main__":
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [os.path.join(_root, "oracle"), os.path.join(_root, "proxmox-backup_amd")]
    if sys.argv[1:2] == ["search"]:
        import oracle as _o
        search(_o, sys.argv[2:] or None)
        print("FOUND = {")
        for k, val in FOUND.items():
            print(f"    {k!r}: {val!r},")
        print("}")
