"""GPU parity of the zstd blob stage (csrc/pbs_zstd.hip) on the planted cases of
tests/zplanted.py: matches on the sub-block seams, the window edge and the block and chunk
ends, match extension and repeat codes at their edges, sequence counts and literal sizes at
every header and kernel threshold, the frame one byte either side of the chunk's length,
every start residue mod 16 -- through the chunks entry point, small batches dealt statically
and the spans entry point.

Every blob must equal oracle.blob_compressed(chunk) -- the host twin's frame -- byte for
byte, carry zlib's CRC and the right compressed flag, and decode with libzstd back to the
chunk.  test_zplanted_cpu.py proves on the CPU that each case holds the feature it is named
for.

Run on an MI355X:  python -m pytest tests/test_gpu_zplanted.py -m gpu -x -q
"""
import struct
import zlib

import numpy as np
import pytest

import zplanted as z

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_dev(gpu):
    import torch

    torch.cuda.set_device(0)
    return torch


def _check(oracle, labels, chunks, result):
    blobs, crcs, comp, guard_clean = result
    assert len(blobs) == len(labels)
    bad = []
    for label, chunk, blob, crc, c in zip(labels, chunks, blobs, crcs, comp):
        raw = chunk.tobytes()
        exp = oracle.blob_compressed(raw)
        if blob != exp:
            a, b = np.frombuffer(blob, np.uint8), np.frombuffer(exp, np.uint8)
            n = min(a.size, b.size)
            d = np.flatnonzero(a[:n] != b[:n])
            at = int(d[0]) if d.size else n
            bad.append(f"{label}: blob differs from the twin's at byte {at} (frame byte {at - 12}); "
                       f"{len(blob)} bytes, the twin's {len(exp)}")
            continue
        if struct.unpack("<I", blob[8:12])[0] != int(crc) or int(crc) != zlib.crc32(blob[12:]):
            bad.append(f"{label}: CRC field {blob[8:12].hex()}, returned {int(crc):#x}, zlib {zlib.crc32(blob[12:]):#x}")
        if bool(c) != (blob[:8] == oracle.COMPRESSED_BLOB_MAGIC):
            bad.append(f"{label}: comp flag {int(c)} against magic {blob[:8].hex()}")
        if c and oracle.zstd_decompress(blob[12:], len(raw)) != raw:
            bad.append(f"{label}: the payload does not decode to the chunk")
    assert not bad, f"{len(bad)} of {len(labels)} cases:\n" + "\n".join(bad[:20])
    assert guard_clean, "bytes past the output capacity were written"


@pytest.mark.parametrize("family", [f for f in sorted(z.FAMILIES) if f != "j"])
def test_family(gpu, oracle, torch_dev, family):
    """One blob_encode_chunks_device call over all the family's chunks back to back."""
    labels, chunks, result = z.gpu_encode_family(gpu, torch_dev, family)
    _check(oracle, labels, chunks, result)
    if family == "i":  # n + 1 and n stay uncompressed, n - 1 is compressed
        assert [int(c) for c in result[2]] == [0, 0, 1]


def test_family_j_spans_at_every_residue(gpu, oracle, torch_dev):
    """blob_encode_spans_device (compress, no crypt config): the same three-block chunk at each
    of the 16 residues mod 16 of its start address, gaps of 1 to 23 bytes, the spans in reverse order."""
    labels, chunks, result = z.gpu_encode_family(gpu, torch_dev, "j")
    assert len(labels) == 16
    _check(oracle, labels, chunks, result)
    assert len(set(result[0])) == 1 and all(result[2])


@pytest.mark.parametrize("family", ["f", "g", "h"])
def test_family_in_small_static_batches(gpu, oracle, torch_dev, monkeypatch, family):
    """The entropy-stage families in parse / entropy launch pairs of three items each, dealt
    statically: one family's items land in different launches."""
    monkeypatch.setenv("PBS_ZSTD_BATCH", "3")
    monkeypatch.setenv("PBS_ZSTD_DEAL", "0")
    labels, chunks, result = z.gpu_encode_family(gpu, torch_dev, family)
    _check(oracle, labels, chunks, result)
