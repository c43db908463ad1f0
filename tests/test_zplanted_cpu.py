"""The planted zstd cases (tests/zplanted.py) proven on the CPU: for every case the twin
(oracle/zstd_twin.cpp) shows the feature the case exists for -- its predicate holds -- the
twin's frame decodes with libzstd back to the chunk and stays within zstd_twin_bound.  A
case whose predicate fails is a failure here, never a skip: test_gpu_zplanted.py compares
the GPU encoder with the twin on exactly these chunks, and a case that lost its feature
would compare nothing of interest.

Two geometry pins tie zplanted's restated constants to the twin's behaviour, so a change of
the sub-block sizes or of the match window fails here first.

The densest block (f/dense) reaches 1618 sequences in one sub-block, 90 % of the capacity
kZSubSeq = 1794: a 5-byte match is only found while its source is still in the sub-block's
4096-entry table, and one copy in ten has lost it to a later position with the same hash.
"""
import numpy as np
import pytest

import zplanted as z

# the cases whose blob is the uncompressed one on purpose: chunks of 1 to 6 bytes, the frames
# of n + 1 and n bytes, and the all-literal block past kHufStreams
UNCOMPRESSED = ({f"e/len{n}" for n in range(1, 7)} | {f"e/len{n}-same" for n in range(1, 7)}
                | {"i/frame=n+1", "i/frame=n", "g/streams>kHufStreams"})
_LABELS = [(f, lab) for f in sorted(z.FAMILIES) for lab in z.labels(f)]


@pytest.mark.parametrize("label", [lab for _, lab in _LABELS])
def test_case_shows_its_feature(oracle, label):
    c = z.case(label)
    v = z.View(oracle, c.chunk)
    assert c.pred(v), f"{label}: the twin does not show: {c.what}"
    assert oracle.zstd_decompress(v.frame, c.chunk.size) == c.chunk.tobytes(), label
    assert len(v.frame) <= oracle.zstd_twin_bound(c.chunk.size), label
    # the GPU test compares the blob: unless the case is about an uncompressed one, the twin's
    # frame must be shorter than the chunk, or only the chunk's own bytes would be compared
    assert (len(v.frame) < c.chunk.size) == (label not in UNCOMPRESSED), (label, len(v.frame), c.chunk.size)
    w = v.walk
    assert w["content_size"] == c.chunk.size and len(w["blocks"]) == max(1, -(-c.chunk.size // z.BLOCK)), label


def test_case_inventory(capsys):
    """Every family has its cases, every label is unique, and the count is printed."""
    per = {f: len(z.labels(f)) for f in sorted(z.FAMILIES)}
    labs = [lab for _, lab in _LABELS]
    assert len(set(labs)) == len(labs)
    assert per["a"] == 7 * len(z.SEAM_PLACES) * len(z.SEAM_L) and per["b"] == 5 * len(z.WINDOW_SUBS)
    assert per["c"] == len(z.EXT_LENGTHS) + 3 + len(z.EXT_BACK) + 1 and per["d"] == 5
    assert per["e"] == 7 * len(z.END_DELTAS) + 2 + 12 + 6 + 5 and per["f"] == len(z.SEQ_COUNTS) + 1
    assert per["g"] == 8 + 6 + 4 + 4 + 1 and per["h"] == 3 and per["i"] == 3 and per["j"] == 1
    with capsys.disabled():
        print(f"\nzplanted: {len(labs)} cases " + " ".join(f"{f}={n}" for f, n in per.items()))


def test_cases_are_deterministic():
    """A case is the same bytes whenever it is built: the GPU test's child process builds its
    own copies."""
    for f in sorted(z.FAMILIES):
        for a, b in zip(z.cases(f), z.cases(f)):
            assert a.label == b.label and np.array_equal(a.chunk, b.chunk), a.label


def test_modes_cover_all_nine(oracle):
    """Family h shows predefined, RLE and FSE-compressed for each of LL, OF and ML."""
    seen = set()
    for c in z.cases("h"):
        for blk in z.View(oracle, c.chunk).walk["blocks"]:
            if blk["modes"]:
                seen |= {(i, m) for i, m in enumerate(blk["modes"])}
    assert seen >= {(i, m) for i in range(3) for m in range(3)}, sorted(seen)


def test_pin_seam_table(oracle):
    """A 300-byte match planted across each seam comes out of the twin as two sequences
    split exactly at zplanted.SEAMS[w - 1], and no sequence of any sub-block crosses a seam."""
    for w in range(1, 8):
        c = z.case(f"a/seam{w}/start-L/2/L300")
        seam, v = z.SEAMS[w - 1], z.View(oracle, c.chunk)
        s = v.parse()
        ends = [o for p, m, o in s if p + m == seam]
        starts = [o for p, m, o in s if p == seam]
        assert ends and starts and set(ends) & set(starts), (w, seam, s[-4:])
        assert not [x for x in s for e in z.SEAMS if x[0] < e < x[0] + x[1]], w


def test_pin_window(oracle):
    """A source exactly zplanted.ZWIN before a sub-block's first byte is found there; one two
    bytes further back only from the sub-block's third byte on (its source is then the
    window's first byte); one byte further back than the window not at all."""
    for blk, w in z.WINDOW_SUBS:
        pos = z.sub_start(w)
        at = z.View(oracle, z.case(f"b/blk{blk}sub{w}/d=kZWin").chunk).with_off(z.ZWIN, blk)
        assert (pos, 24) in at, (blk, w, at)
        past = z.View(oracle, z.case(f"b/blk{blk}sub{w}/d=kZWin+2").chunk).with_off(z.ZWIN + 2, blk)
        assert past == [(pos + 2, 22)], (blk, w, past)
        assert not z.View(oracle, z.case(f"b/blk{blk}sub{w}/d=kZWin+1").chunk).with_off(z.ZWIN + 1, blk)


def test_walker_reads_libzstd_frames(oracle):
    """The frame walker on frames it did not see written: libzstd level 1's of three inputs
    (raw, RLE and compressed blocks; it reads sizes and counts that add up to each frame)."""
    L = oracle.libzstd()
    for data in (z.bg(300, 1, 256), np.zeros(70000, np.uint8), z.bg(3 * z.BLOCK // 2, 2, 16)):
        dst = np.empty(L.ZSTD_compressBound(data.size), np.uint8)
        n = L.ZSTD_compress(dst.ctypes.data, dst.size, data.ctypes.data, data.size, 1)
        w = z.walk_frame(dst[:n].tobytes())
        assert w["content_size"] == data.size
