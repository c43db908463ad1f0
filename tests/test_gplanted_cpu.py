"""The planted AES-256-GCM cases (tests/gplanted.py) proven on the CPU: every case's predicate
holds -- a case that lost its feature is a failure here, never a skip -- the restated geometry
is the library's, and at every case the library's host AES-GCM, the kernels' own GHASH
decomposition run on the host (pbs_test_gcm_tag_segments_host: same tables and mul_tab,
segments from the end) and live libcrypto agree with the reference (tests/aesgcm_ref.py) that
test_gpu_gplanted.py holds the GPU against.  No GPU.
"""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import aesgcm_ref
import gplanted as g

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAIN = ("a", "b", "c", "e")      # families whose expected blob is the encrypted chunk itself
LONG_TAGS = ("b", "c", "e")       # families of more than one segment


@pytest.mark.parametrize("family", sorted(g.FAMILIES))
def test_every_case_shows_its_feature(family):
    cs = g.cases(family)
    labels = [c.label for c in cs]
    assert len(set(labels)) == len(labels)
    bad = [c.label for c in cs if not c.pred()]
    assert not bad, f"{len(bad)} of {len(cs)} cases of family {family} do not hold their feature: {bad[:10]}"
    for c in cs:
        assert len(c.key) == 32 and len(c.iv) == 16 and c.chunk.dtype == np.uint8 and c.chunk.ndim == 1, c.label


def test_case_inventory(capsys):
    per = {f: len(g.cases(f)) for f in sorted(g.FAMILIES)}
    assert per["a"] == 601 and per["b"] == 36 + 3 + 18 + 1 and per["c"] == len(g.CTR_WRAPS) + len(g.CTR_WRAPS_ROWS) + 1 == 13
    assert per["e"] == 4 * 8 and per["e-spare"] == 8 and per["f"] == 5
    assert len(set(g.KEYS + (g.SPARE_KEY,))) == 5
    for f in per:  # no call reuses an IV under a key
        assert len({(c.key, c.iv) for c in g.cases(f)}) == per[f], f
    with capsys.disabled():
        print(f"\ngplanted: {sum(per.values())} cases " + " ".join(f"{f}={n}" for f, n in per.items()))


def test_cases_are_deterministic():
    for f in sorted(g.FAMILIES):
        for a, b in zip(g.cases(f), g.FAMILIES[f]()):
            assert a.label == b.label and a.iv == b.iv and a.key == b.key and np.array_equal(a.chunk, b.chunk), a.label


def test_tail_sweep_meets_every_pair():
    """Over the 16 buffer residues every (rem, payload start mod 16) pair occurs; one call
    alone shows 32 of the 256."""
    assert g.tail_pairs() == {(r, s) for r in range(16) for s in range(16)}
    assert len(g.tail_pairs((0,))) == 32
    assert [c.chunk.size for c in g.cases("a")] == list(range(601))


def test_ragged_lengths():
    """Family b's lengths hit the values of `first` and rem they are named for, the existing
    test's lengths (tests/test_gpu_crypt.py) only first in {1, 2154}."""
    seen = {g.geometry(c.chunk.size)[1:] for c in g.cases("b")}
    for nseg, first, rem in g.RAGGED_2 + g.RAGGED_3 + g.RAGGED_1:
        assert (nseg, first, rem) in seen
    assert (17, 1, 13) in seen
    S = g.SEG
    old = [0, 1, 15, 16, 17, 777, 4105, 65536, 100000, S - 16, S, S + 1, 2 * S + 15, 3 * S + 5]
    assert {g.geometry(n)[2] for n in old if g.geometry(n)[1] > 1} == {1, 2154}


def test_many_items_family():
    """Family d for 256 CUs: more than two trips of the 768 workgroups and seven items over,
    zero-length chunks in the middle, multi-segment chunks among the single ones."""
    cs = g.cases("d")
    s = g.many_summary(cs)
    assert s["segments"] >= 1544 and s["segments"] > 2 * g.GROUPS_PER_CU * g.MANY_NCU + 7
    assert s["empty_inside"] and s["multi"] >= 20 and s["bytes"] < 2 << 20
    assert {c.chunk.size for c in cs if c.chunk.size <= 200} == set(range(201))
    # and at another CU count the list is built for that count
    assert g.many_summary(g.many_cases(8))["segments"] > 2 * g.GROUPS_PER_CU * 8 + 7


def test_geometry_is_the_librarys(pbschunk):
    assert pbschunk.GCM_SEGMENT_BYTES == g.SEG == g.SEGBLOCKS * g.BLOCK
    assert pbschunk.blob_stream_bound_encrypted([7, 7]) == g.HDR == pbschunk.BLOB_ENC_HEADER_SIZE == aesgcm_ref.ENC_HEADER
    assert pbschunk.blob_stream_bound_encrypted([0, 5, 5, 30]) == 3 * g.HDR + 30
    # the constants that no call returns, where pbs_crypt.hip and pbs_blob.h define them
    with open(os.path.join(ROOT, "proxmox-backup_amd", "csrc", "pbs_crypt.hip")) as f:
        src = f.read()
    with open(os.path.join(ROOT, "include", "pbs_blob.h")) as f:
        hdr = f.read()

    def const(text, name):
        m = re.search(r"\b%s\b\s*=?\s*\(?\s*(\d+)" % name, text)
        assert m, name
        return int(m.group(1))
    assert const(src, "kThreads") == g.LANES and const(src, "kGroupsPerCu") == g.GROUPS_PER_CU
    assert const(hdr, "PBS_GCM_SEGMENT_BYTES") == g.SEG and const(hdr, "PBS_BLOB_ENC_HEADER_SIZE") == g.HDR
    assert g.ROWS == g.SEG // g.BLOCK // g.LANES  # kRows


def _split(blob: bytes):
    return blob[12:28], blob[28:44], blob[44:]  # iv, tag, ciphertext


@pytest.fixture(scope="module")
def configs(pbschunk):
    cfgs = {k: pbschunk.CryptConfig(k) for k in g.KEYS + (g.SPARE_KEY,)}
    yield cfgs
    for c in cfgs.values():
        c.close()


@pytest.mark.parametrize("family", PLAIN + ("e-spare",))
def test_host_encrypt_equals_reference(configs, family):
    for c, exp in zip(g.cases(family), g.expected(family)):
        iv, tag, ct = _split(exp)
        assert iv == c.iv and len(exp) == g.HDR + c.chunk.size
        assert configs[c.key].encrypt_host(c.iv, c.chunk) == (ct, tag), c.label


@pytest.mark.parametrize("family", LONG_TAGS + ("e-spare",))
def test_segmented_tag_equals_reference(pbschunk, configs, family):
    """The kernels' decomposition at every planted `first`: the ragged segment's leading
    zeros, the lane powers and the Horner by H^4096 (16 steps for the 17-segment chunk)."""
    f = pbschunk.lib().pbs_test_gcm_tag_segments_host
    for c, exp in zip(g.cases(family), g.expected(family)):
        _, tag, ct = _split(exp)
        a = np.frombuffer(ct, dtype=np.uint8)
        got = (ctypes.c_uint8 * 16)()
        assert f(configs[c.key].handle, c.iv, a.ctypes.data if a.size else None, a.size, got) == pbschunk.PBS_OK
        assert bytes(got) == tag, c.label


@pytest.fixture(scope="module")
def evp():
    sys.path.insert(0, GOLDEN)
    try:
        import make_aesgcm_golden as gen

        L = gen.libcrypto()
        L.EVP_aes_256_gcm
    except (OSError, AttributeError, TypeError):
        pytest.skip("no loadable libcrypto")
    finally:
        sys.path.remove(GOLDEN)
    return lambda key, iv, data: gen.evp_encrypt(L, key, iv, data)


@pytest.mark.parametrize("family", LONG_TAGS + ("e-spare",))
def test_reference_equals_live_libcrypto(evp, family):
    """A second implementation at every case of b, c and e: the one place the all-ones upper
    counter words meet one."""
    for c, exp in zip(g.cases(family), g.expected(family)):
        _, tag, ct = _split(exp)
        assert evp(c.key, c.iv, c.chunk.tobytes()) == (ct, tag), c.label


def test_compressed_expected_blobs_decode(oracle):
    cs = g.cases("f")
    exp = g.compressed_expected(oracle, cs)
    assert [z for _, z in exp] == [False, False, True, True, True]
    for c, (blob, is_zstd) in zip(cs, exp):
        assert blob[:8] == (aesgcm_ref.ENCR_COMPR_BLOB_MAGIC if is_zstd else aesgcm_ref.ENCRYPTED_BLOB_MAGIC), c.label
        assert (len(blob) < g.HDR + c.chunk.size) == is_zstd, c.label
        assert aesgcm_ref.blob_load_decode_encrypted(blob, c.key, g.keyed_digest(c)) == c.chunk.tobytes(), c.label
    # the text chunk's frame is more than one GCM segment
    assert len(exp[3][0]) - g.HDR > g.SEG
