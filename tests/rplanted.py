"""Indexes, digest sets and restatements of the reference for the restore tests (helpers of
test_restore_cpu.py, test_restore_mirror_cpp.py and test_gpu_restore.py; not a conftest)."""
import hashlib
import struct

import numpy as np

MISSING = 0xFFFFFFFF  # PBS_LOOKUP_MISSING


def make_index(n, seed=1, zero_runs=False):
    rng = np.random.default_rng([0x726573, seed, n])
    lens = rng.integers(1, 5000, n).astype(np.uint64)
    if zero_runs and n:
        lens[rng.random(n) < 0.4] = 0
        lens[n // 2] = 17  # (at least one byte in the archive)
    return np.cumsum(lens).astype(np.uint64), rng.integers(0, 256, (n, 32), dtype=np.uint8)


def csum_of(ends, digests):
    h = hashlib.sha256()
    for e, d in zip(ends, digests):
        h.update(struct.pack("<Q", int(e)) + bytes(d))
    return h.digest()


def ref_binary_search(ends, start_idx, start, end_idx, end, offset):
    """DynamicIndexReader::binary_search, dynamic_index.rs:172-195."""
    if offset >= end or offset < start:
        raise ValueError("offset out of range")
    if end_idx == start_idx:
        return start_idx
    middle_idx = (start_idx + end_idx) // 2
    middle_end = ends[middle_idx]
    if offset < middle_end:
        return ref_binary_search(ends, start_idx, start, middle_idx, middle_end, offset)
    return ref_binary_search(ends, middle_idx + 1, middle_end, end_idx, end, offset)


def ref_chunk_from_offset(ends, offset):
    """chunk_from_offset, :258-274 (an empty index panics there: None here)."""
    if not ends:
        return None
    end_idx = len(ends) - 1
    try:
        found = ref_binary_search(ends, 0, 0, end_idx, ends[end_idx], offset)
    except ValueError:
        return None
    return found, offset - (ends[found - 1] if found else 0)


def planted_lookup_sets():
    """(index digests, store digests): repeats on both sides, misses, an unsorted store, and
    digests that share their first 8 bytes and differ in byte 8 or in byte 31 only."""
    rng = np.random.default_rng(0x6C6F6F6B)
    base = rng.integers(0, 256, (40, 32), dtype=np.uint8)
    twins8 = np.repeat(base[:1], 4, axis=0)      # same 8-byte prefix, byte 8 differs
    twins8[:, 8] = [1, 2, 3, 4]
    twins31 = np.repeat(base[1:2], 4, axis=0)    # 31 bytes shared, the last differs
    twins31[:, 31] = [9, 8, 7, 6]
    store = np.concatenate([base[5:30], twins8[[2, 0]], twins31[[3, 1]], base[10:14], twins31[[1]]])
    store = store[rng.permutation(store.shape[0])]
    index = np.concatenate([base[0:12], twins8, base[8:20], twins31, twins8[::-1], base[35:40], base[7:9], twins31[[1, 1, 0]]])
    return index, store


def model_lookup(index, store):
    where, first_of = {}, {}
    for j, d in enumerate(store):
        where.setdefault(d.tobytes(), j)
    pos, first = [], []
    for i, d in enumerate(index):
        pos.append(where.get(d.tobytes(), MISSING))
        first.append(first_of.setdefault(d.tobytes(), i))
    return (np.array(pos, np.uint32), np.array(first, np.uint32), sum(p == MISSING for p in pos), len(first_of))


# ---- the round trip of test_gpu_restore.py ------------------------------------------------------

# The prose cuts into chunks of up to 256 KiB at a 64 KiB average, so a 512 KiB window holds
# five to nine of them and the two copies of a chunk lie 300 KiB apart: at 384 KiB (and for
# 40 KiB either side of it) the second window holds two chunks twice, by the CPU chunker.
ROUNDTRIP_LEN, ROUNDTRIP_REPEAT, ROUNDTRIP_AT, ROUNDTRIP_WINDOW = 2 << 20, 300 << 10, 384 << 10, 512 << 10


def roundtrip_stream() -> np.ndarray:
    """2 MiB of prose in which the 300 KiB at ROUNDTRIP_AT come twice, back to back: the
    chunker finds the same cuts in both copies, so the index names some digests twice."""
    import corpus_gen

    t = corpus_gen.text(ROUNDTRIP_LEN, 11)
    a, r = ROUNDTRIP_AT, ROUNDTRIP_REPEAT
    return np.concatenate([t[:a + r], t[a:a + r], t[a + r:]])[:ROUNDTRIP_LEN].copy()


def stream_windows(ends, window):
    """The (first entry, last entry) of every window restore_stream_device makes: each ends on
    the last chunk end within `window` bytes of its start, or after one chunk longer than that."""
    ends = [int(e) for e in ends]
    out, pos, i = [], 0, 0
    while i < len(ends):
        j = i
        while j + 1 < len(ends) and ends[j + 1] <= pos + window:
            j += 1
        out.append((i, j))
        pos, i = ends[j], j + 1
    return out
