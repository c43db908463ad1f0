"""Kind-0 and kind-2 blobs planted on the edges of the read path's copy kernel (helpers of
test_cplanted_cpu.py and test_gpu_cplanted.py; not a conftest).

segment_copy_kernel (proxmox-backup_amd/csrc/pbs_restore.hip, declared in dev_copy.h) moves the
payloads of pbs_blob_decode_device's unencrypted blobs into the packed output and the chunks of
kinds 0 and 2 of pbs_blob_decode_inflate_device into the caller's slots.  It works on items of at
most 64 KiB + 15 bytes: the up to 15 head bytes before the destination's first 16-byte boundary
and the up to 15 tail bytes after its last go byte by byte, everything between as 16-byte stores
on the destination's boundaries fed by unaligned 16-byte loads.  What can go wrong depends on the
item's length, on the destination's residue mod 16 and on the source's, so the stream below is
run at several (input pad, output pad) pairs; triples() says which combinations that shows.
"""
import numpy as np

import dplanted as d
import gplanted as g

PIECE = 65536
LENGTHS = (0, 1, 15, 16, 17, 31, 32, 33, 65535, 65536, 65537, 65536 + 15, 65536 + 16, 2 * 65536 + 5)
# the kind of each: the short ones 2 and 0 in turn (the 44- and the 12-byte header alternate), the
# long ones kind 0 but one -- the packed call copies kind 0 only, and only an item that ends on
# its 64 KiB cut or a length that suits the destination has no tail bytes
KINDS = (2, 0, 2, 0, 2, 0, 2, 0, 0, 0, 0, 2, 0, 0)
# one more blob, kind 2 with a flipped tag bit, between two intact neighbours: zeros over its
# whole slot (three zero items; at most pads the first has head bytes and the last tail bytes).
# Its place and length shift the residues of what follows: test_cplanted_cpu.py checks that
# the pads below still show every combination.
BAD_AT, BAD_LEN = 13, 2 * 65536 + 64
PLENS = LENGTHS[:BAD_AT] + (BAD_LEN,) + LENGTHS[BAD_AT:]
PKINDS = KINDS[:BAD_AT] + (2,) + KINDS[BAD_AT:]
ROOM = 9          # bytes the roomier slots of the inflate call are longer than their chunks
SHORT_AT, SHORT_BY = PLENS.index(65536 + 16), 21   # the slot cut under its payload in the last inflate run
# (input pad, output pad): residues mod 16 of the blob stream's and of the output's first byte
IN_PADS, OUT_PADS = tuple(range(8)), tuple(range(16))
PADS = tuple((ip, op) for op in OUT_PADS for ip in IN_PADS)
MODES = ("exact", "roomy", "short")
SCRATCH_ALIGN = 256   # the inflate call's packed payloads start on an allocation's boundary
BAD_TAG = d.BAD_TAG


def payloads() -> list:
    return [np.random.default_rng([0x63706C, i]).integers(1, 256, n, dtype=np.uint8).tobytes()
            for i, n in enumerate(PLENS)]


_items = []


def items(oracle) -> list:
    """The stream as dplanted Items (built once per process).  No payload byte is zero, so a
    zeroed byte never passes for a copied one."""
    if not _items:
        for i, (k, p) in enumerate(zip(PKINDS, payloads())):
            it = d.good(f"c/{i}/kind{k}/len{len(p)}", d.make_blob(oracle, k, p, g.KEY1, g._iv(9500 + i)), g.KEY1, p)
            if i == BAD_AT:
                it = d.bad(f"c/{i}/kind2/tag-bit", it, d._flip(it.blob, 28 + 9, 2), BAD_TAG)
            _items.append(it)
    return _items


def slot_sizes(mode: str) -> list:
    if mode == "exact":
        return list(PLENS)
    if mode == "roomy":
        return [n + ROOM for n in PLENS]
    return [n - SHORT_BY if i == SHORT_AT else n for i, n in enumerate(PLENS)]


def copy_items(src: int, dst: int, n: int) -> list:
    """add_items (dev_copy.h): the (source, destination, length) of the kernel's items for one
    segment; the first ends on the destination's first boundary + 64 KiB."""
    out, at, m = [], 0, min(n, (-dst) % 16 + PIECE)
    while at < n:
        out.append((src + at, dst + at, m))
        at += m
        m = min(n - at, PIECE)
    return out


def segments(in_pad: int, out_pad: int) -> list:
    """(source, destination, length), addresses relative to a 16-byte boundary, of every segment
    with a source that the GPU test's calls copy at one pad pair: the kind-0 payloads of the
    packed call; for the inflate call the same into its packed scratch, then the chunks of both
    kinds from there into the slots of each mode (the blob with the bad tag is not copied)."""
    hdr = [(d.HDR, d.EHDR)[k // 2] for k in PKINDS]
    boff = np.concatenate([[0], np.cumsum([h + n for h, n in zip(hdr, PLENS)])])
    poff = np.concatenate([[0], np.cumsum(PLENS)])
    out = []
    for base in (out_pad, SCRATCH_ALIGN):
        out += [(in_pad + int(boff[i]) + hdr[i], base + int(poff[i]), n) for i, n in enumerate(PLENS) if PKINDS[i] == 0]
    for mode in MODES:
        sizes = slot_sizes(mode)
        ooff = np.concatenate([[0], np.cumsum(sizes)])
        out += [(SCRATCH_ALIGN + int(poff[i]), out_pad + int(ooff[i]), min(n, sizes[i]))
                for i, n in enumerate(PLENS) if i != BAD_AT]
    return out


def triples(pads=PADS) -> set:
    """Every (length, source mod 16, destination mod 16) of the kernel's items over the given
    pad pairs, the length mod 16 for items of 16 bytes and more (shorter ones as they are: they
    may end before the destination's first boundary)."""
    return {(m if m < 16 else 16 + m % 16, s % 16, t % 16)
            for ip, op in pads for seg in segments(ip, op) for s, t, m in copy_items(*seg)}


def tail_of(m: int, t: int) -> int:
    """Bytes after the last 16-byte store of an item of length class m (a triple's first member,
    16 and up) at destination residue t."""
    return (m - (-t) % 16) % 16
