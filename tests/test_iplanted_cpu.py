"""The frame corpus of tests/iplanted.py on the CPU: that it holds every feature of the format
the decoder must read (a block walker counts them), that libzstd reads every hand-assembled
frame as its writer meant it, and that the host mirror pbs_zstd_inflate_host -- the format code
the GPU kernel shares (csrc/zstd_dec.h) -- equals libzstd on every intact frame and obeys the
corruption rule on every bad one."""
import hashlib

import numpy as np
import pytest

import iplanted as ip


@pytest.fixture(scope="module")
def corpus():
    return ip.corpus()


def test_corpus_holds_every_feature(corpus):
    seen = set()
    for it in corpus["good"]:
        w = ip.walk(it.frame)
        assert w["end_of_blocks"] + (4 if w["checksum"] else 0) == len(it.frame), it.label
        seen.add("single-segment" if w["single"] else "window-descriptor")
        seen.add(f"fcs-{w['fcs_len']}")
        if w["checksum"]:
            seen.add("checksum")
        if w["blocks"][-1]["size"] == 0:
            seen.add("last-block-empty")
        for b in w["blocks"]:
            seen.add(f"block-type-{b['type']}")
            if b["type"] != 2:
                continue
            seen.add(f"lit-type-{b['lit_type']}")
            if b["lit_type"] < 2:
                seen.add(f"lit-raw-rle-sf-{b['lit_sf']}")
            else:
                seen.add(f"streams-{b['streams']}")
                seen.add(f"lit-huf-sf-{b['lit_sf']}")
            if "weights_fse" in b:
                seen.add("weights-fse" if b["weights_fse"] else "weights-direct")
            seen.add(f"nbseq-form-{b['nbseq_form']}")
            if b["nbseq"]:
                for name, mode in zip(("ll", "of", "ml"), b["modes"]):
                    seen.add(f"{name}-mode-{mode}")
    want = {"single-segment", "window-descriptor", "checksum", "last-block-empty", "fcs-0", "fcs-1", "fcs-2", "fcs-4",
            "fcs-8", "block-type-0", "block-type-1", "block-type-2", "lit-type-0", "lit-type-1", "lit-type-2",
            "lit-type-3", "streams-1", "streams-4", "weights-direct", "weights-fse", "nbseq-form-1", "nbseq-form-2",
            "nbseq-form-3", "lit-raw-rle-sf-0", "lit-raw-rle-sf-1", "lit-raw-rle-sf-2", "lit-raw-rle-sf-3"}
    want |= {f"{t}-mode-{m}" for t in ("ll", "of", "ml") for m in range(4)}
    assert not want - seen, f"the corpus lacks {sorted(want - seen)}"


def test_libzstd_reads_every_intact_frame_as_stated(oracle, corpus):
    """The wanted bytes of every frame are libzstd's -- for the hand-assembled frames that is the
    proof that the writer assembled what it meant."""
    for it in corpus["good"]:
        assert oracle.zstd_decompress(it.frame, it.cap) == it.want, it.label
        assert oracle.zstd_decode_stream(it.frame, 1 << 17) == it.want, it.label
    assert sum(it.family == "hand" for it in corpus["good"]) >= 20


def test_corruptions_cover_both_outcomes(corpus):
    bad = corpus["bad"]
    assert sum(it.want is None for it in bad) > 100
    assert sum(it.want is not None for it in bad) > 5  # flips libzstd reads through: the bytes must agree
    assert set(ip.RFC_FORBIDDEN_BUT_ACCEPTED) <= {it.label for it in bad}


def test_host_mirror_equals_libzstd_on_intact_frames(pbschunk, corpus):
    for it in corpus["good"]:
        got, st = pbschunk.zstd_inflate_host(it.frame, it.cap)
        assert st == ip.OK and got == it.want, (it.label, ip.STATUS_NAMES[st], len(got), len(it.want))
        # a larger slot changes nothing
        got, st = pbschunk.zstd_inflate_host(it.frame, it.cap + 77)
        assert st == ip.OK and got == it.want, it.label


def test_host_mirror_obeys_the_corruption_rule(pbschunk, corpus):
    wrong = []
    for it in corpus["bad"]:
        got, st = pbschunk.zstd_inflate_host(it.frame, it.cap)
        msg = ip.check(it, st, got)
        if msg:
            wrong.append(msg)
    assert not wrong, f"{len(wrong)} of {len(corpus['bad'])}:\n" + "\n".join(wrong[:20])


def test_named_statuses(pbschunk, corpus):
    by = {it.label: it for it in corpus["bad"]}
    v = "text300k-L1-nosize"
    for label, st in ((f"{v}/dict-id", ip.UNSUPPORTED), (f"{v}/window-log-28", ip.UNSUPPORTED),
                      (f"{v}/second-frame", ip.UNSUPPORTED), (f"{v}/skippable-frame", ip.UNSUPPORTED),
                      (f"{v}/slot-one-short", ip.TOO_LARGE), (f"{v}/trailing-byte", ip.BAD_FRAME),
                      (f"{v}/block0-type3", ip.BAD_FRAME), (f"{v}/reserved-bit", ip.BAD_FRAME),
                      ("text300k-L1/slot-one-short" if "text300k-L1/slot-one-short" in by else
                       "twin-text/slot-one-short", ip.TOO_LARGE)):
        it = by[label]
        got, status = pbschunk.zstd_inflate_host(it.frame, it.cap)
        assert status == st, (label, ip.STATUS_NAMES[status])
    # a content size above the slot is found before anything is written
    it = by["twin-text/slot-one-short"]
    got, status = pbschunk.zstd_inflate_host(it.frame, it.cap)
    assert status == ip.TOO_LARGE and got == b""


def test_frame_content_size(pbschunk, corpus):
    for it in corpus["good"]:
        w = ip.walk(it.frame)
        size = pbschunk.zstd_frame_content_size(it.frame)
        assert size == (len(it.want) if w["fcs_len"] else None), it.label
    with pytest.raises(ValueError):
        pbschunk.zstd_frame_content_size(b"\x28\xb5\x2f")
    with pytest.raises(ValueError):
        pbschunk.zstd_frame_content_size(b"not a frame at all")


def test_blob_decode_host_is_unchanged(pbschunk, oracle):
    """pbs_blob_decode_host still hands the frame of a compressed blob back, with status OK."""
    chunk = ip.text(50_000, 31)
    blob = oracle.blob_compressed(chunk)
    assert blob[:8] == oracle.COMPRESSED_BLOB_MAGIC
    pay, kind, st = pbschunk.blob_decode_host(blob, expect_digest=hashlib.sha256(chunk).digest(), expect_size=len(chunk))
    assert (kind, st) == (1, 0) and pay == blob[12:]
    got, zst = pbschunk.zstd_inflate_host(pay, len(chunk))
    assert zst == ip.OK and got == chunk
    raw = oracle.blob_uncompressed(chunk)
    pay, kind, st = pbschunk.blob_decode_host(raw, expect_digest=hashlib.sha256(chunk).digest(), expect_size=len(chunk))
    assert (kind, st) == (0, 0) and pay == chunk
