"""Planted inputs of the fixed-size chunk path (include/pbs_fixed.h): the .fidx image built by
hand from the layout, the numpy model of the dirty map and the byte positions at which the dirty
kernel's tiling can go wrong.  No GPU, no library: the CPU and the GPU tests share these."""
import hashlib
import struct

import numpy as np

FIDX_MAGIC = bytes([47, 127, 65, 237, 145, 253, 15, 205])  # file_formats.rs:20-21
ITEM = 256 * 1024          # bytes one workgroup of the dirty kernel compares per item
LANE, WAVE, ROW = 16, 1024, 4096  # a lane's load, a wave's, the 256-lane workgroup's row

assert hashlib.sha256(b"Proxmox Backup fixed sized chunk index v1.0").digest()[:8] == FIDX_MAGIC


def digests_of(n: int, seed: int = 0) -> np.ndarray:
    """n digests that are no hash of anything (the index does not care)."""
    return np.random.default_rng([0x66696478, seed]).integers(0, 256, (n, 32), dtype=np.uint8)


def count(size: int, chunk_size: int) -> int:
    return (size + chunk_size - 1) // chunk_size


def model_image(digests: np.ndarray, size: int, chunk_size: int, uuid: bytes, ctime: int) -> bytes:
    """fixed_index.rs:20-32: magic, uuid, ctime, index_csum, size, chunk_size, zeros to 4096; the
    digests.  index_csum = SHA-256 over the digests (:341-362)."""
    body = np.ascontiguousarray(digests, dtype=np.uint8).tobytes()
    assert len(body) == 32 * count(size, chunk_size) and len(uuid) == 16
    head = FIDX_MAGIC + uuid + struct.pack("<q", ctime) + hashlib.sha256(body).digest() + struct.pack("<QQ", size, chunk_size)
    assert len(head) == 80
    return head + bytes(4096 - 80) + body


def model_chunk_alignment(size: int, chunk_size: int, offset: int, chunk_len: int):
    """check_chunk_alignment, fixed_index.rs:364-392, transcribed: the index, or the bail's text."""
    if offset < chunk_len:                                                   # :365
        return "small offset"
    pos = offset - chunk_len                                                 # :369
    if offset > size:                                                        # :371
        return "exceeds size"
    if (offset != size and chunk_len != chunk_size) or chunk_len > chunk_size or chunk_len == 0:  # :376-378
        return "unexpected length"
    if pos & (chunk_size - 1):                                               # :387
        return "unaligned"
    return pos // chunk_size                                                 # :391


def model_dirty(prev: np.ndarray, cur: np.ndarray, chunk_size: int) -> np.ndarray:
    """1 per chunk in which any byte differs."""
    diff = np.flatnonzero(prev != cur)
    flags = np.zeros(count(prev.size, chunk_size), dtype=np.uint8)
    flags[np.unique(diff // chunk_size)] = 1
    return flags


def image_pair(size: int, seed: int = 0):
    a = np.random.default_rng([0x64697274, seed]).integers(0, 256, size, dtype=np.uint8)
    return a, a.copy()


def flip_positions(size: int, chunk_size: int) -> dict:
    """label -> byte position: one flip per run, each alone in its chunk's flag.  The boundaries
    are measured from the start of the item that holds them (items tile every chunk from its
    start, min(chunk_size, ITEM) bytes each)."""
    item = min(chunk_size, ITEM)
    n = count(size, chunk_size)
    mid = (n // 2) * chunk_size               # a middle chunk's start
    out = {"mid-chunk-first": mid, "mid-chunk-last": min(mid + chunk_size, size) - 1,
           "image-first": 0, "image-last": size - 1}
    tail = size % LANE                        # the image's last item ends with < 16 loose bytes
    if tail:
        out["tail-first"] = size - tail
        if tail > 2:
            out["tail-inside"] = size - tail + tail // 2
    for name, step in (("lane", LANE), ("wave", WAVE), ("row", ROW)):
        if step < item:
            out[f"{name}-boundary-before"] = mid + step - 1
            out[f"{name}-boundary-after"] = mid + step
            out[f"last-{name}-boundary-before"] = mid + item - step - 1
            out[f"last-{name}-boundary-after"] = mid + item - step
    if chunk_size > ITEM:                     # an item boundary inside a chunk
        out["item-boundary-before"] = mid + ITEM - 1
        out["item-boundary-after"] = mid + ITEM
        out["last-item-first"] = mid + chunk_size - ITEM
    return {k: v for k, v in out.items() if 0 <= v < size}


def planted_dirty_sets(chunk_size: int = 4096):
    """(label, prev, cur) over small images: equal, all different, and every flip position."""
    out = []
    for r in (0, 1, 15, 16, 17, chunk_size - 1):
        size = 5 * chunk_size + r
        a, b = image_pair(size, r)
        out.append((f"r{r}/equal", a, b))
        out.append((f"r{r}/all-different", a, a ^ np.uint8(0xFF)))
        for label, at in flip_positions(size, chunk_size).items():
            for bit in (0x01, 0x80):
                c = a.copy()
                c[at] ^= bit
                out.append((f"r{r}/{label}/x{bit:02x}", a, c))
    return out
