"""Chunks, IVs and keys that sit on the AES-256-GCM blob stage's own boundaries (helpers of
test_gplanted_cpu.py and test_gpu_gplanted.py; not a conftest).

The stage (proxmox-backup_amd/csrc/pbs_crypt.hip) encrypts a payload in 64 KiB segments
counted from the chunk's END, one 256-lane workgroup per segment and trip of a grid-stride
loop; lane t takes blocks t, t + 256, ... (16 rows), the counter of block k is J0's low word
plus k + 1 in 32-bit arithmetic, the last partial block moves byte by byte.  The geometry
below restates those values once, each beside the symbol it restates; test_gplanted_cpu.py
pins them to the library.

Every case is (label, key, iv, chunk, predicate).  The predicate is evaluated on the CPU and
states the feature the case exists for; a case whose predicate is false fails
test_gplanted_cpu.py -- none is skipped or dropped.  All data comes from seeded numpy
generators.  The expected blob of a case (compress off) is
aesgcm_ref.blob_encode_encrypted(chunk, key, iv), computed once per family (expected()).

The largest chunk is 1 MiB + 13 bytes (17 segments: the tag kernel's Horner by H^4096 runs
16 steps).  There is no 16 MiB chunk on purpose: no threshold of the stage lies between 17
and 256 segments of one chunk -- the items of a chunk are independent workgroup trips and the
tag kernel's loop has no path that depends on their count.
"""
import hashlib
from typing import Callable, NamedTuple

import numpy as np

import aesgcm_ref

# ---- geometry (pbs_crypt.hip unless stated) ------------------------------------------------
BLOCK = 16                        # the GCM block
LANES = 256                       # kThreads
WAVE = 64                         # the wave width (the __shfl_xor reduction, red[kThreads / 64])
ROWS = 16                         # kRows
SEG = 65536                       # PBS_GCM_SEGMENT_BYTES (include/pbs_blob.h)
SEGBLOCKS = 4096                  # kSegBlocks
HDR = 44                          # PBS_BLOB_ENC_HEADER_SIZE (include/pbs_blob.h)
GROUPS_PER_CU = 3                 # kGroupsPerCu
assert SEGBLOCKS == SEG // BLOCK == ROWS * LANES and LANES % WAVE == 0

KEY1 = bytes([1]) * 32            # the reference fixture's key (tests/blob_writer.rs)
KEYS = (bytes(32), bytes([255]) * 32, KEY1, np.random.default_rng(0x6B657973).integers(0, 256, 32, dtype=np.uint8).tobytes())
KEY_NAMES = ("zeros", "ones", "fixture", "random")
SPARE_KEY = np.random.default_rng(0x6B657974).integers(0, 256, 32, dtype=np.uint8).tobytes()  # family e's late config
ONES96 = (1 << 96) - 1


class Case(NamedTuple):
    label: str
    key: bytes
    iv: bytes
    chunk: np.ndarray
    pred: Callable[[], bool]


def geometry(n: int):
    """(m, nseg, first, rem) of a payload of n bytes as gcm_ctr_ghash_kernel computes them:
    blocks, segments, blocks of segment 0 (the ragged one), bytes of the last block (0: full)."""
    m = (n + 15) >> 4
    nseg = (m + SEGBLOCKS - 1) // SEGBLOCKS
    first = m - (nseg - 1) * SEGBLOCKS if nseg else 0
    return m, nseg, first, n % BLOCK


def segments(n: int) -> int:
    """Items of a payload of n bytes (gcm_encrypt_blobs)."""
    return (n + SEG - 1) // SEG


def where(n: int, at: int) -> str:
    """Blob byte `at` of a blob with n payload bytes, in the kernel's terms."""
    if at < HDR:
        return "header: " + ("magic" if at < 8 else "crc" if at < 12 else "iv" if at < 28 else "tag")
    kb = (at - HDR) // BLOCK
    m, nseg, first, rem = geometry(n)
    seg = 0 if kb < first else 1 + (kb - first) // SEGBLOCKS
    q = kb - (first + (seg - 1) * SEGBLOCKS)  # position in the segment's 4096 slots
    return (f"GCM block {kb} of {m} (byte {(at - HDR) % BLOCK}), segment {seg} of {nseg}, row {q // LANES}, "
            f"lane {q % LANES} (wave {q % LANES // WAVE})" + (", the partial last block" if kb == m - 1 and rem else ""))


def _bytes(seed: int, n: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8)


def _iv(seed: int) -> bytes:
    return np.random.default_rng([0x4956, seed]).integers(0, 256, 16, dtype=np.uint8).tobytes()


# ---- a. tail sweep ---------------------------------------------------------------------------

TAIL_LENGTHS = tuple(range(601))
TAIL_PADS = tuple(range(16))      # residue mod 16 of the blob buffer's first byte


def tail_starts(pad: int) -> list:
    """Payload start (relative to a 16-byte boundary) of every blob of the sweep when the blob
    buffer starts at residue `pad`: the blobs lie back to back, blob i is 44 + i bytes."""
    out, at = [], pad
    for n in TAIL_LENGTHS:
        out.append(at + HDR)
        at += HDR + n
    return out


def tail_pairs(pads=TAIL_PADS) -> set:
    """Every (rem, payload start mod 16) the sweep shows over the given buffer residues."""
    return {(n % BLOCK, s % 16) for pad in pads for n, s in zip(TAIL_LENGTHS, tail_starts(pad))}


def tail_cases() -> list:
    """a. Every length 0..600 back to back in one call.  Blob i is 44 + i bytes, so the payload
    start moves through the residues mod 16 -- but it depends on i mod 32 only, and rem is
    i mod 16: one call shows two residues per rem (32 of the 256 pairs).  The call is therefore
    run at the 16 buffer residues TAIL_PADS, and over all of them every pair occurs
    (tail_pairs; a case's predicate: its own rem meets all 16 residues)."""
    starts = [tail_starts(p) for p in TAIL_PADS]

    def pred(i):
        n = TAIL_LENGTHS[i]
        return n == i and {s[i] % 16 for s in starts} == set(range(16)) and geometry(n)[3] == n % BLOCK
    return [Case(f"a/len{n}", KEY1, _iv(1000 + n), _bytes(1000 + n, n), lambda i=i: pred(i))
            for i, n in enumerate(TAIL_LENGTHS)]


# ---- b. ragged first segment -----------------------------------------------------------------

RAGGED_2 = tuple((2, f, r) for f in (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095) for r in (0, 1, 15))
RAGGED_3 = tuple((3, f, 7) for f in (1, 256, 4095))
RAGGED_1 = tuple((1, m, r) for m in (1, 255, 256, 257, 511, 512, 513, 4095, 4096) for r in (0, 9))
LONG = (1 << 20) + 13             # 17 segments, first = 1, rem 13


def ragged_len(nseg: int, first: int, rem: int) -> int:
    return ((nseg - 1) * SEGBLOCKS + first) * BLOCK - ((BLOCK - rem) % BLOCK)


def _ragged_case(nseg: int, first: int, rem: int, key: bytes = KEY1, tag: str = "b") -> Case:
    n = ragged_len(nseg, first, rem)
    seed = 2000000 + n
    return Case(f"{tag}/nseg{nseg}/first{first}/rem{rem}", key, _iv(seed), _bytes(seed, n),
                lambda: geometry(n)[1:] == (nseg, first, rem) and segments(n) == nseg)


def ragged_cases() -> list:
    """b. Segment 0 holds `first` blocks: one and two, either side of the wave (64), of the
    workgroup row (256), of four rows (1024) and one short of a full segment, in chunks of two
    and three segments, with a full, a one-byte and a 15-byte last block; single-segment chunks
    whose block count sits on the same boundaries; one chunk of 17 segments."""
    cs = [_ragged_case(*x) for x in RAGGED_2 + RAGGED_3 + RAGGED_1]
    cs.append(Case("b/nseg17/first1/rem13", KEY1, _iv(2999), _bytes(2999, LONG),
                   lambda: geometry(LONG) == (65537, 17, 1, 13) and segments(LONG) == 17))
    return cs


# ---- c. counter ------------------------------------------------------------------------------

CTR_FIRST, CTR_REM = 300, 5
CTR_LEN = ragged_len(2, CTR_FIRST, CTR_REM)
CTR_M = SEGBLOCKS + CTR_FIRST
CTR_WRAPS = (0, 15, 255, 256, 299, 300, 301, CTR_M - 1)
# and where the kernel's own rows turn: block 0 is slot 4096 - 300 of segment 0 (row 14, lane 212), so
# row 15 starts at block 44; segment 1's row 1 starts at block 300 + 256
CTR_WRAPS_ROWS = (43, 44, CTR_FIRST + LANES - 1, CTR_FIRST + LANES)


def _counter_case(w, key: bytes = KEY1, tag: str = "c") -> Case:
    """J0 = 96 one bits || low; w: the block whose counter word is 0 (None: low = 0, no wrap)."""
    low = 0 if w is None else (1 << 32) - 1 - w
    j0 = ONES96 << 32 | low
    c = aesgcm_ref.cipher(key)
    iv = c.iv_for_j0(j0)
    seed = 3000 + (CTR_M if w is None else w)

    def pred():
        if c.j0(iv) != j0 or geometry(CTR_LEN) != (CTR_M, 2, CTR_FIRST, CTR_REM):
            return False
        if w is None:
            return low == 0 and low + CTR_M < 1 << 32
        return 0 <= w < CTR_M and (low + w + 1) % (1 << 32) == 0
    return Case(f"{tag}/low0" if w is None else f"{tag}/wrap{w}", key, iv, _bytes(seed, CTR_LEN), pred)


def counter_cases() -> list:
    """c. J0's upper 96 bits all ones (an add that carries past the low word shows in every
    block after the wrap), its low word 2^32 - 1 - w: the counter word is 0 at block w -- the
    chunk's first blocks (0, 15), blocks 255 and 256, segment 0's last block (299), segment 1's
    first two (300, 301) and the partial last block (m - 1) of a chunk of 300 + 4096 blocks,
    rem 5; the blocks either side of a lane's step from one row to the next in each segment
    (CTR_WRAPS_ROWS).  And one J0 whose low word is 0."""
    return [_counter_case(w) for w in CTR_WRAPS + CTR_WRAPS_ROWS + (None,)]


# ---- d. many items ---------------------------------------------------------------------------

MANY_NCU = 256                    # the CU count the CPU test proves the family for


def many_cases(ncu: int = MANY_NCU) -> list:
    """d. More items than two trips of the grid: the launch has min(items, ncu * kGroupsPerCu)
    workgroups, so with more than 2 * 3 * ncu + 7 segments every workgroup takes at least two
    items and some take three.  Single-segment chunks of lengths 1..200, cycled; every 64th
    chunk is a two- or three-segment chunk of family b; 32 chunks after each of those a
    zero-length chunk, which has no item (ifirst[i] == ifirst[i + 1] in the tag kernel)."""
    big = [x for x in RAGGED_2 + RAGGED_3 if x[1] <= 257 and x[2] != 0]  # (the short ones: ~1.9 MB in all)
    want = 2 * GROUPS_PER_CU * ncu + 7
    cs, nitems, i, small = [], 0, 0, 0
    while nitems <= want:
        if i % 64 == 0:
            nseg, first, rem = big[(i // 64) % len(big)]
            n, label = ragged_len(nseg, first, rem), f"d/{i}/nseg{nseg}/first{first}/rem{rem}"
        elif i % 64 == 32:
            nseg, n, label = 0, 0, f"d/{i}/empty"
        else:
            nseg, n = 1, 1 + small % 200
            small += 1
            label = f"d/{i}/len{n}"
        cs.append(Case(label, KEY1, _iv(4000000 + i), _bytes(4000000 + i, n),
                       lambda n=n, nseg=nseg: segments(n) == geometry(n)[1] == nseg))
        nitems += nseg
        i += 1
    return cs


def many_summary(cs) -> dict:
    """What the family as a whole must show: its item count and where its empty chunks sit."""
    sizes = [c.chunk.size for c in cs]
    return {"segments": sum(segments(n) for n in sizes), "bytes": sum(sizes),
            "empty_inside": [i for i, n in enumerate(sizes) if n == 0 and 0 < i < len(sizes) - 1],
            "multi": sum(1 for n in sizes if n > SEG)}


# ---- e. keys ---------------------------------------------------------------------------------

KEY_SUBSET_B = ((2, 1, 1), (2, 64, 0), (2, 257, 15), (2, 4095, 15), (3, 256, 7), (1, 257, 9))
KEY_SUBSET_C = (256, CTR_M - 1)


def key_cases(key: bytes, name: str) -> list:
    """Eight cases of families b and c under `key`."""
    return ([_ragged_case(*x, key=key, tag=f"e/{name}") for x in KEY_SUBSET_B]
            + [_counter_case(w, key=key, tag=f"e/{name}") for w in KEY_SUBSET_C])


def keys_cases() -> list:
    """e. The all-zero and all-ones keys, the fixture's and a seeded random one, eight cases
    each.  (The spare key of the GPU test's late config: key_cases(SPARE_KEY, "spare").)"""
    return [c for key, name in zip(KEYS, KEY_NAMES) for c in key_cases(key, name)]


# ---- f. compressed payloads ------------------------------------------------------------------

def compressed_cases() -> list:
    """f. Chunks whose encrypted payload is the zstd frame: zplanted's family i (frames of
    n + 1, n and n - 1 bytes: only the last is compressed), three blocks of text and 70 000
    zeros.  The predicate is on the chunk alone; what the payload is comes from the oracle
    (compressed_expected)."""
    import corpus_gen
    import zplanted

    cs = [(f"f/{c.label}", c.chunk) for c in zplanted.cases("i")]
    cs.append(("f/text-3-blocks", corpus_gen.text(3 * 65536 + 8192, 5)[:3 * 65536 - 5]))
    cs.append(("f/zeros70000", np.zeros(70000, np.uint8)))
    sizes = {"f/i/frame=n+1": 1000, "f/i/frame=n": 1000, "f/i/frame=n-1": 1000, "f/text-3-blocks": 3 * 65536 - 5,
             "f/zeros70000": 70000}
    return [Case(label, KEY1, _iv(6000 + i), np.ascontiguousarray(chunk, dtype=np.uint8),
                 lambda label=label, chunk=chunk: chunk.size == sizes[label])
            for i, (label, chunk) in enumerate(cs)]


def compressed_expected(oracle, cs) -> list:
    """(blob, payload is zstd) per case, from the oracle alone: the payload of the oracle's
    unencrypted blob, encrypted by the reference."""
    out = []
    for c in cs:
        plain = oracle.blob_compressed(c.chunk.tobytes())
        is_zstd = plain[:8] == oracle.COMPRESSED_BLOB_MAGIC
        out.append((aesgcm_ref.blob_encode_encrypted(plain[12:], c.key, c.iv, is_zstd), is_zstd))
    return out


FAMILIES = {"a": tail_cases, "b": ragged_cases, "c": counter_cases, "d": many_cases, "e": keys_cases,
            "e-spare": lambda: key_cases(SPARE_KEY, "spare"), "f": compressed_cases}
_cases, _expected = {}, {}


def cases(family: str, *args) -> list:
    """The family's cases, built once per process (the chunks are not to be written to)."""
    k = (family,) + args
    if k not in _cases:
        _cases[k] = FAMILIES[family](*args)
        for c in _cases[k]:
            c.chunk.setflags(write=False)
    return _cases[k]


def expected(family: str, *args) -> list:
    """aesgcm_ref.blob_encode_encrypted of every case of the family (compress off), once."""
    k = (family,) + args
    if k not in _expected:
        _expected[k] = [aesgcm_ref.blob_encode_encrypted(c.chunk.tobytes(), c.key, c.iv) for c in cases(family, *args)]
    return _expected[k]


def keyed_digest(c: Case) -> bytes:
    return hashlib.sha256(c.chunk.tobytes() + aesgcm_ref.id_key(c.key)).digest()


# ---- the GPU side (test_gpu_gplanted.py) -------------------------------------------------------

PAD, GUARD, FILL = 5, 4096, 0xA5
BASE = (1 << 33) + 12345


def layout_chunks(chunks):
    """The chunks back to back above BASE: (data, absolute bounds)."""
    data = np.concatenate([np.zeros(0, np.uint8)] + list(chunks))
    return data, (BASE + np.concatenate([[0], np.cumsum([c.size for c in chunks])])).astype(np.uint64)


def layout_spans(chunks):
    """The chunks with gaps of 1 to 23 bytes before them, the spans in reverse order:
    (data, absolute spans, order) -- span k is chunk order[k]."""
    parts, spans, at = [], [], 0
    for i, c in enumerate(chunks):
        gap = 1 + (7 * i) % 23
        parts += [np.full(gap, 0xEE, np.uint8), c]
        spans.append((BASE + at + gap, BASE + at + gap + c.size))
        at += gap + c.size
    order = list(range(len(chunks)))[::-1]
    return np.concatenate(parts), np.asarray([spans[i] for i in order], dtype=np.uint64), order


class Encoded(NamedTuple):
    blobs: list       # bytes per chunk
    crcs: np.ndarray
    comp: np.ndarray
    outside_clean: bool  # every byte outside [pad, pad + offs[-1]) as it was filled
    timing: dict


def gpu_upload(torch, data: np.ndarray, pad: int = 3):
    """(keep-alive tensor, device address of data[0]); the data starts `pad` bytes into it."""
    t = torch.zeros(pad + data.size, dtype=torch.uint8, device="cuda")
    if data.size:
        t[pad:] = torch.from_numpy(data).to("cuda")
    return t, t.data_ptr() + pad


def gpu_encode(gpu, torch, cfg, src, data_len: int, ivs, bounds=None, spans=None, pad: int = PAD, compress: bool = False,
               hip_stream: int = 0) -> Encoded:
    """One encrypted encode call into a buffer filled with FILL whose blob stream starts at an
    address that is `pad` mod 16, with GUARD bytes behind the bound."""
    if spans is None:
        cap = gpu.blob_stream_bound_encrypted(bounds)
    else:
        cap = HDR * len(spans) + int(sum(int(e) - int(s) for s, e in spans))
    out = torch.full((16 + pad + cap + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    lead = (-out.data_ptr()) % 16 + pad
    torch.cuda.synchronize()
    f, arg = (gpu.blob_encode_chunks_device, bounds) if spans is None else (gpu.blob_encode_spans_device, spans)
    offs, crcs, comp, t = f(src, data_len, arg, out.data_ptr() + lead, cap, base=BASE, compress=compress,
                            hip_stream=hip_stream, crypt=cfg, ivs=ivs)
    torch.cuda.synchronize()
    img = out.cpu().numpy()
    end = lead + int(offs[-1])
    assert int(offs[0]) == 0 and int(offs[-1]) <= cap
    blobs = [img[lead + int(offs[i]):lead + int(offs[i + 1])].tobytes() for i in range(len(offs) - 1)]
    return Encoded(blobs, crcs, comp, bool((img[:lead] == FILL).all() and (img[end:] == FILL).all()), t)
