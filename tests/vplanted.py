"""Planted inputs for the verify job (include/pbs_verify.h) and a Python model of the reference
(helpers of test_verify_cpu.py and test_gpu_verify.py; not a conftest).

The model is a transliteration of `verify_index_chunks` (src/backup/verify.rs:108-270) with its
`skip_chunk` (:163-188), `get_chunks_in_order` with ChunkOrder::None
(pbs-datastore/src/datastore.rs:1249-1293), `verify_fixed_index` / `verify_dynamic_index`
(:272-314) and `verify_blob` (:48-70) over a dict store with a sequential decoder: a set of
verified and a set of corrupt digests, one index after the other.  The verdict on a blob comes
from the reference functions of the oracle and of tests/aesgcm_ref.py (through
dplanted.reference_outcome for everything but the zstd kinds), never from the library.

A planted case is a store (a list of (digest, blob or None): the listing in its order, None for a
file that cannot be read) and a sequence of indexes that one worker verifies.  Blobs come from
dplanted.make_blob (four kinds) and its corruptions; chunks are 1 byte to 128 KiB.
"""
import hashlib
import struct
import zlib
from typing import NamedTuple, Optional

import numpy as np

import aesgcm_ref
import dplanted as d
import gcplanted
import gplanted as g

UNKNOWN, VERIFIED, CORRUPT = 0, 1, 2
MODE_NONE, MODE_ENCRYPT = 0, 1
BAD_FRAME, LOAD_FAILED = 8, 32
INDEX_OK, WRONG_SIZE, WRONG_CSUM = 0, 1, 2
BOUNDARY = (0, 1, 63, 64, 65, 255, 256, 257, 4097)
RESULT_KEYS = ("entries", "skipped_verified", "skipped_corrupt", "loaded", "newly_verified", "newly_corrupt",
               "mode_mismatch", "missing", "read_bytes", "decoded_bytes", "errors", "ok", "index_check")
ENC_MAGICS = (aesgcm_ref.ENCRYPTED_BLOB_MAGIC, aesgcm_ref.ENCR_COMPR_BLOB_MAGIC)


class Index(NamedTuple):
    name: str
    digests: list           # n digests of 32 bytes
    sizes: list             # n chunk sizes
    mode: int
    info: Optional[tuple]   # None, or (size or None, csum or None) as the manifest states them


class Case(NamedTuple):
    label: str
    store: list             # [(digest, blob bytes or None)]
    indexes: list


# ---- the model ------------------------------------------------------------------------------------

def verdict(oracle, blob: bytes, digest: bytes, size: int):
    """(kind, status) of load_chunk + verify_unencrypted for one chunk file, by the reference
    functions.  A chunk LONGER than the index's size reports BAD_DIGEST (the slot rule of
    pbs_blob_decode_inflate_device, pbs_blob.h) where the reference says "wrong length": the
    chunk is corrupt in both."""
    kind = d.kind_of(blob)
    if len(blob) >= d.HDR and blob[:8] in ENC_MAGICS:
        kind = 2 + ENC_MAGICS.index(blob[:8])  # (from_raw knows the magic before it asks for 44 bytes)
        st, _ = d.reference_outcome(oracle, d.Item("", blob, digest, size, kind, 0, b""), None)
        return kind, d.OK if st == d.NO_CONFIG else st  # verify_unencrypted: Ok for encrypted chunks
    try:
        data = oracle.blob_load_decode(blob, None, read_sizes=(64 * 1024,))
    except ValueError as e:
        try:
            return kind, d._status_of(e)
        except ValueError:
            return kind, BAD_FRAME  # decode_all failed
    if len(data) > size or hashlib.sha256(data).digest() != digest:
        return kind, d.BAD_DIGEST
    return kind, d.OK if len(data) == size else d.BAD_SIZE


def index_image(oracle, ix: Index):
    """The .didx image of an index and what an honest manifest says of it: (image, (size, csum))."""
    ends = np.cumsum(np.asarray(ix.sizes, dtype=np.uint64)) if ix.sizes else []
    image, csum = oracle.didx_image(ends, ix.digests)
    return image, (int(ends[-1]) if len(ix.sizes) else 0, csum)


class Model:
    """One VerifyWorker over a store."""

    def __init__(self, oracle, store):
        self.oracle = oracle
        self.store = store
        self.lowest = {}
        for j, (dig, _) in enumerate(store):
            self.lowest.setdefault(dig, j)
        self.verified, self.corrupt = set(), set()

    def states(self):
        s = np.zeros(len(self.store), dtype=np.uint8)
        for dig, j in self.lowest.items():
            s[j] = VERIFIED if dig in self.verified else CORRUPT if dig in self.corrupt else UNKNOWN
        return s

    def verify_index(self, ix: Index, image_info=None):
        """verify_dynamic_index: dict(result, todo_store, todo_entry, kinds, status, corrupt_store,
        missing_pos).  `image_info`: what compute_csum gives for the image, (size, csum)."""
        res = dict.fromkeys(RESULT_KEYS, 0)
        res["entries"] = len(ix.digests)
        out = dict(result=res, todo_store=[], todo_entry=[], kinds=[], status=[], corrupt_store=[], missing_pos=[])
        if ix.info is not None and image_info is not None:
            if ix.info[0] is not None and ix.info[0] != image_info[0]:  # :305-307
                res["index_check"] = WRONG_SIZE
                return out
            if ix.info[1] is not None and ix.info[1] != image_info[1]:  # :309-311
                res["index_check"] = WRONG_CSUM
                return out
        errors = 0
        loads = []  # (store position, index position, kind, status)

        def skip_chunk(dig, first_pass):
            nonlocal errors
            if dig in self.verified:
                res["skipped_verified"] += first_pass
                return True
            if dig in self.corrupt:
                errors += 1  # "was marked as corrupt"
                if first_pass and dig in self.lowest:
                    res["skipped_corrupt"] += 1
                return True
            return False

        chunk_list = [pos for pos, dig in enumerate(ix.digests) if not skip_chunk(dig, True)]  # get_chunks_in_order
        for pos in chunk_list:
            dig, size = ix.digests[pos], ix.sizes[pos]
            if skip_chunk(dig, False):  # "we must always recheck this here"
                continue
            j = self.lowest.get(dig)
            blob = self.store[j][1] if j is not None else None
            if blob is None:  # load_chunk: no such file, or it cannot be read
                self.corrupt.add(dig)
                errors += 1
                if j is not None:
                    loads.append((j, pos, d.KIND_NONE, LOAD_FAILED))
                continue
            kind, st = verdict(self.oracle, blob, dig, size)
            loads.append((j, pos, kind, st))
            if st in (d.TOO_SMALL, d.BAD_MAGIC, d.BAD_CRC):  # load_chunk fails
                self.corrupt.add(dig)
                errors += 1
                continue
            res["loaded"] += 1
            res["read_bytes"] += len(blob)
            res["decoded_bytes"] += size
            if (kind >= 2) != (ix.mode == MODE_ENCRYPT):  # :140-148
                res["mode_mismatch"] += 1
                errors += 1
            if st != d.OK:
                self.corrupt.add(dig)
                errors += 1
            else:
                self.verified.add(dig)
        out["missing_pos"] = [pos for pos, dig in enumerate(ix.digests) if dig not in self.lowest]
        res["missing"] = len(out["missing_pos"])
        loads.sort()  # the plan reads in the listing's order
        out["todo_store"] = [l[0] for l in loads]
        out["todo_entry"] = [l[1] for l in loads]
        out["kinds"] = [l[2] for l in loads]
        out["status"] = [l[3] for l in loads]
        out["corrupt_store"] = [l[0] for l in loads if l[3] != d.OK]
        res["newly_corrupt"] = len(out["corrupt_store"])
        res["newly_verified"] = len(loads) - res["newly_corrupt"]
        res["errors"] = errors
        res["ok"] = int(errors == 0)
        return out


def model_verify_blob(oracle, raw: bytes, size: int, csum: bytes) -> str:
    """verify_blob (:48-70): "" or the error's class."""
    if len(raw) != size:
        return "wrong size"
    if hashlib.sha256(raw).digest() != csum:
        return "wrong index checksum"
    if len(raw) >= d.HDR and raw[:8] in ENC_MAGICS:
        try:
            aesgcm_ref.blob_decrypt_payload(raw, g.KEY1)
        except ValueError as e:
            if "tag mismatch" not in str(e):
                return "load"
        return ""
    try:
        oracle.blob_load_decode(raw, None, read_sizes=(64 * 1024,))
    except ValueError as e:
        try:
            d._status_of(e)
            return "load"
        except ValueError:
            return "decode"
    return ""


# ---- planted cases --------------------------------------------------------------------------------

_metas = {}  # case label -> {digest: the chunk size an honest index states}


def _rnd_bytes(tag: int, n: int) -> bytes:
    return np.random.default_rng([0x766572, tag]).integers(0, 256, n, dtype=np.uint8).tobytes()


_goods = {}


def _good(oracle, kind: int, n: int, seed: int):
    """(digest, blob, chunk length) of an intact chunk of `kind` (built once per process)."""
    if (kind, n, seed) not in _goods:
        _goods[kind, n, seed] = _make_good(oracle, kind, n, seed)
    return _goods[kind, n, seed]


def _make_good(oracle, kind: int, n: int, seed: int):
    chunk = d._chunk(seed, n, kind in (1, 3))
    blob = d.make_blob(oracle, kind, chunk, g.KEY1, g._iv(90000 + seed))
    if kind in (1, 3):
        assert d.kind_of(blob) == kind, (kind, n)
    dig = d.keyed_digest(chunk, g.KEY1) if kind >= 2 else d.plain_digest(chunk)
    return dig, blob, len(chunk)


def specials(oracle):
    """Every status at least once: [(label, digest, blob or None, index size, kind, status)]."""
    if "specials" not in _goods:
        _goods["specials"] = _make_specials(oracle)
    return _goods["specials"]


def _make_specials(oracle):
    out = []
    s0 = _good(oracle, 0, 100, 1)
    s1 = _good(oracle, 1, 5000, 2)
    s2 = _good(oracle, 2, 100, 3)
    s3 = _good(oracle, 3, 5000, 4)
    for k, s in enumerate((s0, s1, s2, s3)):
        out.append((f"good-kind{k}", s[0], s[1], s[2], k, d.OK))
    big = _good(oracle, 1, 128 * 1024, 5)
    out.append(("good-kind1-128k", big[0], big[1], big[2], 1, d.OK))
    one = _good(oracle, 0, 1, 6)
    out.append(("good-kind0-1byte", one[0], one[1], 1, 0, d.OK))

    def other(tag):
        return _rnd_bytes(tag, 32)

    out.append(("too-small-0", other(10), b"", 100, d.KIND_NONE, d.TOO_SMALL))
    out.append(("too-small-11", other(11), s0[1][:11], 100, d.KIND_NONE, d.TOO_SMALL))
    out.append(("too-small-enc-43", other(12), s2[1][:43], 100, 2, d.TOO_SMALL))
    out.append(("bad-magic", other(13), d._flip(s0[1], 0, 3), 100, d.KIND_NONE, d.BAD_MAGIC))
    out.append(("bad-crc-plain", other(14), d._flip(s0[1], d.HDR + 5, 1), 100, 0, d.BAD_CRC))
    out.append(("bad-crc-enc", other(15), d._flip(s2[1], d.EHDR + 5, 1), 100, 2, d.BAD_CRC))
    out.append(("bad-crc-encr-compr", other(16), d._flip(s3[1], d.EHDR + 9, 2), 5000, 3, d.BAD_CRC))
    out.append(("bad-frame", other(17), d._with_crc(d._flip(s1[1], d.HDR, 0)), 5000, 1, BAD_FRAME))  # the frame's magic
    out.append(("bad-frame-cut", other(18), d._with_crc(s1[1][:-7]), 5000, 1, BAD_FRAME))
    out.append(("bad-digest-kind0", other(19), s0[1], 100, 0, d.BAD_DIGEST))
    out.append(("bad-digest-kind1", other(20), s1[1], 5000, 1, d.BAD_DIGEST))
    t0, t1 = _good(oracle, 0, 300, 7), _good(oracle, 1, 6000, 8)
    out.append(("bad-size-kind0", t0[0], t0[1], 301, 0, d.BAD_SIZE))
    out.append(("bad-size-kind1", t1[0], t1[1], 6001, 1, d.BAD_SIZE))
    u0, u1 = _good(oracle, 0, 300, 9), _good(oracle, 1, 6000, 10)
    out.append(("longer-than-index-kind0", u0[0], u0[1], 299, 0, d.BAD_DIGEST))
    out.append(("longer-than-index-kind1", u1[0], u1[1], 5999, 1, d.BAD_DIGEST))
    out.append(("load-failed", other(21), None, 100, d.KIND_NONE, LOAD_FAILED))
    # encrypted chunks are verified by the CRC alone: a digest that is not theirs, a size that is
    # not theirs, a wrong key -- all VERIFIED
    out.append(("enc-any-digest", other(22), s2[1], 7, 2, d.OK))
    wk = d.make_blob(oracle, 2, d._chunk(23, 64, False), g.SPARE_KEY, g._iv(90023))
    out.append(("enc-other-key", other(23), wk, 64, 2, d.OK))
    return out


def specials_hold(oracle) -> list:
    """The planted statuses by the reference functions: the labels that do not hold."""
    bad = []
    for label, dig, blob, size, kind, st in specials(oracle):
        got = (d.KIND_NONE, LOAD_FAILED) if blob is None else verdict(oracle, blob, dig, size)
        if got != (kind, st):
            bad.append((label, got, (kind, st)))
    return bad


def planted(oracle, m: int, n: int, seed: int = 1, mode: int = MODE_NONE) -> Case:
    """A store of exactly m entries and one index of exactly n entries on the kernels' edges, as
    many of the groups as fit:
      specials   every status once (specials())
      dup        one digest twice in the store: a good blob at the lower position and garbage at
                 the higher (VERIFIED; the higher entry stays UNKNOWN), and the reverse (CORRUPT)
      wrap       four digests with home slots among the table's last four (good encrypted blobs:
                 their digest is not checked)
      cluster    six digests with the same first 8 bytes, good encrypted and BAD_DIGEST in turn
      fill       small good chunks of kind 0, among the first 128 now and then kinds 1, 2, 3
    The index names store entries in random order with repeats, absent digests (random ones, and
    ones equal to a present digest except in byte 8 or 31), one digest at 0 and n - 1 and one at
    255 and 256, and two digests twice with a right and a wrong size, the right one first for
    one and the wrong one first for the other."""
    rng = np.random.default_rng([seed, m, n])
    L = gcplanted.table_log2(m)
    store, meta = [], {}  # meta: digest -> index size

    def add(dig, blob, size):
        store.append((dig, blob))
        meta.setdefault(dig, size)

    sp = specials(oracle)
    if m >= len(sp):
        for _, dig, blob, size, _, _ in sp:
            add(dig, blob, size)
    enc_small = _good(oracle, 2, 40, 30)[1]
    if m - len(store) >= 4:
        a, b = _good(oracle, 0, 50, 31), _good(oracle, 0, 60, 32)
        add(a[0], a[1], a[2])
        add(b[0], d._flip(b[1], d.HDR + 1, 0), b[2])
        add(a[0], b"garbage", a[2])
        add(b[0], b[1], b[2])
    if m - len(store) >= 4:
        for dig in gcplanted._wrap_digests(rng, L, 4):
            add(dig, enc_small, 40)
    if m - len(store) >= 6:
        pre = rng.bytes(8)
        c0 = _good(oracle, 0, 20, 33)
        for k in range(6):
            add(pre + rng.bytes(24), enc_small if k % 2 == 0 else c0[1], 40 if k % 2 == 0 else 20)
    k, goods = 0, []
    while len(store) < m:
        kind = (0, 0, 0, 0, 0, 0, 0, 2, 0, 0, 0, 1, 0, 0, 0, 3)[k % 16] if k < 128 else 0
        c = _good(oracle, kind, 4200 + 37 * k if kind in (1, 3) else 1 + (k * 7919) % 199,
                  1000 + k)
        add(c[0], c[1], c[2])
        if kind in (0, 1):
            goods.append(c[0])
        k += 1
    assert len(store) == m
    present = list(dict.fromkeys(dig for dig, _ in store))
    entries = []  # (digest, size)
    for dig in present:
        if len(entries) < n:
            entries.append((dig, meta[dig]))
    j = 0
    while len(entries) < n:
        if present and j % 5 != 4:
            dig = present[int(rng.integers(0, len(present)))]
            entries.append((dig, meta[dig]))
        elif present and j % 10 == 4:
            p = present[int(rng.integers(0, len(present)))]
            entries.append((p[:8] + bytes([p[8] ^ 1]) + p[9:] if j % 20 == 4 else p[:31] + bytes([p[31] ^ 0x80]), 10))
        else:
            entries.append((rng.bytes(32), 10))
        j += 1
    order = rng.permutation(n)
    entries = [entries[i] for i in order]
    # the representative across a block boundary and across the whole index
    if n >= 257:
        entries[256] = entries[255]
    if n >= 2 and present:
        entries[n - 1] = entries[0]
        if n == 257:  # (one digest at 0, 255 and 256)
            entries[255] = entries[0]
    # the first size decides
    fills = [dig for dig in goods if dig not in (entries[0][0], entries[255][0] if n >= 257 else None)] if n >= 8 else []
    if len(fills) >= 2:
        a, b = fills[0], fills[-1]
        free = [i for i in range(1, n - 1) if i not in (255, 256) and entries[i][0] not in (a, b)][:4]
        if len(free) == 4:
            for i in range(n):  # (the planted pairs are their digests' only occurrences)
                if entries[i][0] in (a, b) and i not in free:
                    entries[i] = (rng.bytes(32), 10)
            entries[free[0]], entries[free[1]] = (a, meta[a]), (a, meta[a] + 1)      # OK
            entries[free[2]], entries[free[3]] = (b, meta[b] + 1), (b, meta[b])      # BAD_SIZE
    ix = Index(f"m{m}-n{n}.didx", [e[0] for e in entries], [e[1] for e in entries], mode, None)
    case = Case(f"planted/m{m}/n{n}/seed{seed}/mode{mode}", store, [ix])
    _metas[case.label] = meta
    return case


def sequence(oracle, m: int = 300, n: int = 200) -> Case:
    """Three indexes on one worker: the second names what the first verified (nothing is loaded
    for those) and what it found corrupt (every occurrence counts), plus some chunks the first did
    not name; the third has a wrong info size, and a fourth a wrong checksum: no state changes."""
    base = planted(oracle, m, n, seed=3)
    first = base.indexes[0]
    named = set(first.digests)
    rest = [(dig, blob) for dig, blob in base.store if dig not in named]
    sizes = {dig: s for dig, s in zip(first.digests, first.sizes)}
    second_d = list(first.digests[:n // 2]) + list(first.digests[:n // 4])
    second_s = [sizes[x] for x in second_d]
    assert len(rest) >= 8
    for dig, _ in rest[:8]:
        second_d.append(dig)
        second_s.append(_metas[base.label][dig])
    second = Index("second.didx", second_d, second_s, MODE_NONE, None)
    third = Index("third.didx", list(first.digests), list(first.sizes), MODE_NONE, ("size+1", None))
    fourth = Index("fourth.didx", list(first.digests), list(first.sizes), MODE_NONE, (None, "csum^1"))
    return Case("sequence", base.store, [first, second, third, fourth])


def encrypted_store(oracle, m: int = 70) -> Case:
    """An all-encrypted store under an index of mode ENCRYPT: verified with no key."""
    store, digs, sizes = [], [], []
    for k in range(m):
        kind = 2 if k % 3 else 3
        c = _good(oracle, kind, 4500 + k if kind == 3 else 1 + 37 * k, 5000 + k)
        store.append((c[0], c[1]))
        digs.append(c[0])
        sizes.append(c[2])
    return Case("all-encrypted", store, [Index("enc.didx", digs, sizes, MODE_ENCRYPT, None)])


def mismatch_cases(oracle) -> list:
    """Mode mismatch in both directions: good chunks end VERIFIED and the index fails."""
    plain = [_good(oracle, k % 2, 4300 + k if k % 2 else 10 + k, 6000 + k) for k in range(5)]
    enc = [_good(oracle, 2 + k % 2, 4300 + k if k % 2 else 10 + k, 6100 + k) for k in range(5)]
    bad = _good(oracle, 0, 77, 6200)
    a = Case("mismatch/plain-chunks-encrypt-index", [(c[0], c[1]) for c in plain] + [(bad[0], d._flip(bad[1], 20, 0))],
             [Index("a.didx", [c[0] for c in plain] + [bad[0], plain[0][0]], [c[2] for c in plain] + [77, plain[0][2]],
                    MODE_ENCRYPT, None)])
    b = Case("mismatch/encrypted-chunks-none-index", [(c[0], c[1]) for c in enc],
             [Index("b.didx", [c[0] for c in enc], [c[2] for c in enc], MODE_NONE, None)])
    mixed = plain[:2] + enc[:2]
    c = Case("mismatch/mixed", [(x[0], x[1]) for x in mixed],
             [Index("c.didx", [x[0] for x in mixed], [x[2] for x in mixed], MODE_NONE, None)])
    return [a, b, c]


_cases = {}


def cases(oracle) -> list:
    """Every planted case, built once per process."""
    if "all" not in _cases:
        out = []
        for m in BOUNDARY:
            out.append(planted(oracle, m, 257 if m < 257 else 300, seed=1))
        for n in BOUNDARY:
            out.append(planted(oracle, 300, n, seed=2))
        out.append(planted(oracle, 0, 0, seed=4))
        out.append(planted(oracle, 4097, 4097, seed=5))
        out.append(sequence(oracle))
        out.append(encrypted_store(oracle))
        out += mismatch_cases(oracle)
        _cases["all"] = out
    return _cases["all"]


def resolve_info(ix: Index, honest):
    """The (size, csum) a test passes for an index: the planted wrong values made concrete."""
    if ix.info is None:
        return None
    size, csum = ix.info
    if size == "size+1":
        size = honest[0] + 1
    if csum == "csum^1":
        csum = honest[1][:31] + bytes([honest[1][31] ^ 1])
    return size, csum


_expected = {}


def expected(oracle, case: Case, resident: bool = False) -> list:
    """The model's outcome of every index of a case, with the states after it: computed once.
    `resident`: the store as store_stream lays it out, where a file that cannot be read is an
    empty one (TOO_SMALL instead of LOAD_FAILED)."""
    key = (case.label, resident)
    if key not in _expected:
        mdl = Model(oracle, [(dg, b"" if resident and b is None else b) for dg, b in case.store])
        outs = []
        for ix in case.indexes:
            image, honest = index_image(oracle, ix)
            o = mdl.verify_index(ix._replace(info=resolve_info(ix, honest)), honest)
            o["states"] = mdl.states()
            o["image"], o["honest"] = image, honest
            outs.append(o)
        _expected[key] = outs
    return _expected[key]


# ---- driving a worker -----------------------------------------------------------------------------

def listing(case: Case):
    """(paths None, digests (m, 32)) as VerifyWorker takes it."""
    dg = np.frombuffer(b"".join(x[0] for x in case.store), dtype=np.uint8).reshape(-1, 32).copy()
    return None, dg


def store_stream(case: Case):
    """(bytes of all chunk files back to back, m + 1 offsets); an unreadable file is empty here."""
    blobs = [b if b is not None else b"" for _, b in case.store]
    off = np.concatenate([[0], np.cumsum([len(b) for b in blobs])]).astype(np.uint64)
    return np.frombuffer(b"".join(blobs), dtype=np.uint8), off


def has_unreadable(case: Case) -> bool:
    return any(b is None for _, b in case.store)


def digest_rows(digests):
    return np.frombuffer(b"".join(digests), dtype=np.uint8).reshape(-1, 32).copy()


def result_diff(got: dict, want: dict) -> list:
    return [(k, got[k], want[k]) for k in RESULT_KEYS if int(got[k]) != int(want[k])]


def by_hand(worker, case: Case, ix: Index, upload, batch: int = 0):
    """plan / submit / finish with the blobs of the case's store: `upload(bytes array)` returns
    what submit takes (a device address or the array) and something to keep alive.  `batch`: items
    per submit (0: all in one).  Returns dict like the model's."""
    ts, te = worker.plan(digest_rows(ix.digests) if ix.digests else np.zeros((0, 32), np.uint8), ix.sizes, ix.mode)
    kinds, status = [], []
    step = batch or max(1, ts.size)
    for t0 in range(0, ts.size, step):
        part = ts[t0:t0 + step]
        blobs = [case.store[int(j)][1] for j in part]
        failed = [1 if b is None else 0 for b in blobs]
        raw = b"".join(b or b"" for b in blobs)
        off = np.concatenate([[0], np.cumsum([len(b or b"") for b in blobs])]).astype(np.uint64)
        ptr, keep = upload(np.frombuffer(raw, dtype=np.uint8))
        k, s = worker.submit(ptr, off, failed)
        del keep
        kinds += [int(x) for x in k]
        status += [int(x) for x in s]
    res, cs, mp = worker.finish(len(ix.digests))
    return dict(result=res, todo_store=[int(x) for x in ts], todo_entry=[int(x) for x in te], kinds=kinds, status=status,
                corrupt_store=[int(x) for x in cs], missing_pos=[int(x) for x in mp], states=worker.states())


def outcome_diff(got: dict, want: dict, lists=("todo_store", "todo_entry", "kinds", "status", "corrupt_store",
                                                 "missing_pos")) -> list:
    """What differs between an outcome of by_hand / verify_index and the model's."""
    bad = result_diff(got["result"], want["result"])
    for k in lists:
        if k in got and list(got[k]) != list(want[k]):
            a, b = list(got[k]), list(want[k])
            i = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            bad.append((k, f"differs at {i}: {a[i:i + 4]} / {b[i:i + 4]} (lengths {len(a)}, {len(b)})"))
    if not np.array_equal(got["states"], want["states"]):
        j = int(np.flatnonzero(got["states"] != want["states"])[0])
        bad.append(("states", f"entry {j}: {int(got['states'][j])}, wanted {int(want['states'][j])}"))
    return bad


# ---- a real datastore ----------------------------------------------------------------------------

def build_snapshot(oracle, pbschunk, base):
    """A datastore under `base` with one snapshot: a .didx archive of 40 chunks (all four kinds;
    one chunk file damaged behind a recomputed CRC, one absent), a .fidx archive of four chunks
    (the last one clipped), a .blob file and the manifest.  Returns (snapshot_dir, dict(corrupt
    path, absent digest)).  Every csum and size of the manifest is an honest one."""
    import json
    import os

    snap = os.path.join(base, "vm", "100", "2024-01-01T00:00:00Z")
    os.makedirs(snap)

    def put(dig, blob):
        h = dig.hex()
        os.makedirs(os.path.join(base, ".chunks", h[:4]), exist_ok=True)
        path = os.path.join(base, ".chunks", h[:4], h)
        with open(path, "wb") as f:
            f.write(blob)
        return path

    digs, sizes, paths = [], [], []
    for k in range(40):
        kind = (0, 1)[k % 2]
        c = _good(oracle, kind, 4200 + 37 * k if kind else 1 + 50 * k, 7000 + k)
        digs.append(c[0])
        sizes.append(c[2])
        paths.append(put(c[0], c[1]) if k != 11 else None)
    bad = _good(oracle, 0, 1 + 50 * 6, 7006)
    with open(paths[6], "wb") as f:
        f.write(d._with_crc(d._flip(bad[1], d.HDR + 3, 4)))
    digs += digs[:5]  # repeats
    sizes += sizes[:5]
    ends = np.cumsum(np.asarray(sizes, dtype=np.uint64))
    dimg, dcsum = oracle.didx_image(ends, digs)
    with open(os.path.join(snap, "root.pxar.didx"), "wb") as f:
        f.write(dimg)

    cs, fsize = 4096, 3 * 4096 + 100
    data = d._chunk(7100, fsize, True)
    fdigs = []
    for i in range(4):
        chunk = data[i * cs:(i + 1) * cs]
        fdigs.append(d.plain_digest(chunk))
        put(fdigs[-1], d.make_blob(oracle, i % 2, chunk, g.KEY1, g._iv(1)))
    fimg, fcsum = pbschunk.fidx_build(np.frombuffer(b"".join(fdigs), np.uint8).reshape(-1, 32), fsize, cs)
    with open(os.path.join(snap, "drive-scsi0.img.fidx"), "wb") as f:
        f.write(bytes(fimg))

    conf = oracle.blob_uncompressed(b"memory: 2048\n")
    with open(os.path.join(snap, "qemu-server.conf.blob"), "wb") as f:
        f.write(conf)
    files = [
        {"filename": "qemu-server.conf.blob", "size": len(conf), "csum": hashlib.sha256(conf).hexdigest(), "crypt-mode": "none"},
        {"filename": "root.pxar.didx", "size": int(ends[-1]), "csum": dcsum.hex(), "crypt-mode": "none"},
        {"filename": "drive-scsi0.img.fidx", "size": fsize, "csum": bytes(fcsum).hex(), "crypt-mode": "none"},
    ]
    manifest = {"backup-type": "vm", "backup-id": "100", "backup-time": 1704067200, "files": files, "unprotected": {}}
    with open(os.path.join(snap, "index.json.blob"), "wb") as f:
        f.write(oracle.blob_uncompressed(json.dumps(manifest).encode()))
    return snap, dict(corrupt_path=paths[6], absent=digs[11], files=files)
