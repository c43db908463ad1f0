"""Planted inputs for the backup session (include/pbs_backup.h) and a Python model of the reference
(helpers of test_backup_cpu.py and test_gpu_backup.py; not a conftest).

The model is written from the rules that include/pbs_backup.h states -- `UploadChunk`
(src/api2/backup/upload_chunk.rs), `ChunkStore::insert_chunk` (pbs-datastore/src/chunk_store.rs:
457-497), `BackupEnvironment` (src/api2/backup/environment.rs) and the append handlers of
src/api2/backup/mod.rs -- over dicts and lists, one request after the other.  It takes nothing from
the library: blob verdicts come the way vplanted.verdict gets them (the oracle's reference
functions) on the blob with its CRC put right, CRCs from zlib, checksums and index images from
hashlib and struct.

A planted case is a listing and a script that drives a session -- the `Model` here, or a library
session behind the same methods (`Session`) -- and logs everything the calls give back; the tests
run it on the model, the host mirror and the device and compare the logs.
"""
import hashlib
import struct
import zlib

import numpy as np

import aesgcm_ref
import dplanted as d
import vplanted as v

KIND_NONE, KIND_NOT_FILE = 255, 254
BAD_PARAM, WRONG_LENGTH = 33, 34
INS_NONE, INS_NEW, INS_DUP_SAME, INS_OVERWRITE_EMPTY, INS_DUP_KEEP_FIRST, INS_DUP_KEEP_SMALLER, INS_REPLACE_BIGGER = range(7)
INS_ERR_TYPE, INS_ERR_READ, INS_ERR_UNENC_TO_ENC, INS_ERR_ENC_UNCOMPRESSED = 16, 17, 18, 19
ACT_NONE, ACT_WRITE, ACT_TOUCH = 0, 1, 2
REG_NONE, REG_OK, REG_ERR_LARGE, REG_ERR_MULTI_SMALL = 0, 1, 2, 3
(E_FINISHED, E_NO_WRITER, E_NO_SUCH_CHUNK, E_STRANGE_OFFSET, E_INDEX_RANGE, E_CHUNK_COUNT, E_SIZE, E_EXPECTED_COUNT,
 E_CSUM, E_OPEN_WRITER, E_NO_FILES, E_REUSE_NO_IMAGE, E_REUSE_CSUM, E_REUSE_LENGTH, E_TOO_MANY_WRITERS) = range(64, 79)
ERR_INVALID, ERR_NOT_POW2 = -6, -1
NONE = (1 << 64) - 1
MAX_CHUNK = 16 << 20
DIDX_MAGIC = bytes([28, 145, 78, 165, 25, 186, 179, 205])
FIDX_MAGIC = bytes([47, 127, 65, 237, 145, 253, 15, 205])
UPLOAD_KEYS = ("status", "crc", "ins", "action", "is_duplicate", "compressed_size", "reg")
BOUNDARY = (0, 1, 63, 64, 65, 255, 256, 257, 1000)


# ---- blobs ----------------------------------------------------------------------------------------

def rnd(tag, n: int) -> bytes:
    return np.random.default_rng([0x626B70, *np.atleast_1d(tag)]).integers(0, 256, n, dtype=np.uint8).tobytes()


def plain_blob(chunk: bytes) -> bytes:
    """DataBlob of kind 0."""
    return d.UNCOMPRESSED_MAGIC + struct.pack("<I", zlib.crc32(chunk)) + chunk


def frame_blob(chunk: bytes, blocks: int = 1) -> bytes:
    """DataBlob of kind 1 whose zstd frame stores the chunk in `blocks` raw blocks: a valid encoding
    of the chunk that is 9 + 3 (blocks - 1) bytes longer than the kind-0 blob (chunks under 256 bytes)."""
    assert 0 < len(chunk) < 256 and 1 <= blocks <= len(chunk)
    frame = struct.pack("<IBB", 0xFD2FB528, 0x20, len(chunk))  # single segment, 1-byte content size
    cuts = [len(chunk) * i // blocks for i in range(blocks + 1)]
    for i in range(blocks):
        part = chunk[cuts[i]:cuts[i + 1]]
        frame += struct.pack("<I", len(part) << 3 | (1 if i == blocks - 1 else 0))[:3] + part
    return d.COMPRESSED_MAGIC + struct.pack("<I", zlib.crc32(frame)) + frame


def enc_blob(kind: int, n: int, tag) -> bytes:
    """Something with an encrypted magic, 32 bytes of IV and tag and n payload bytes: all the
    session ever looks at (an encrypted chunk is accepted after from_raw)."""
    body = rnd(tag, 32 + n)
    return d.MAGICS[kind] + struct.pack("<I", zlib.crc32(body[32:])) + body


def upload_verdict(oracle, blob: bytes, digest: bytes, size: int):
    """(kind, status, crc) of UploadChunk for one blob whose length passed the schema: from_raw,
    then verify_unencrypted for the unencrypted kinds; the stored CRC is never judged and the one
    the store must write comes out."""
    kind = d.kind_of(blob)
    if len(blob) >= d.HDR and blob[:8] in v.ENC_MAGICS:
        kind = 2 + v.ENC_MAGICS.index(blob[:8])
        if len(blob) < d.EHDR:
            return kind, d.TOO_SMALL, 0
        return kind, d.OK, zlib.crc32(blob[d.EHDR:])
    if len(blob) < d.HDR:
        return KIND_NONE, d.TOO_SMALL, 0
    if kind == KIND_NONE:
        return kind, d.BAD_MAGIC, 0
    k2, st = v.verdict(oracle, d._with_crc(blob), digest, size)
    assert k2 == kind and st != d.BAD_CRC
    return kind, st, zlib.crc32(blob[d.HDR:])


def didx_image(ends, digests, uuid=bytes(16), ctime=0):
    body = b"".join(struct.pack("<Q", e) + dg for e, dg in zip(ends, digests))
    csum = hashlib.sha256(body).digest()
    head = DIDX_MAGIC + uuid + struct.pack("<q", ctime) + csum
    return head + bytes(4096 - len(head)) + body, csum


def fidx_image(digests, size, chunk_size, uuid=bytes(16), ctime=0):
    body = b"".join(digests)
    csum = hashlib.sha256(body).digest()
    head = FIDX_MAGIC + uuid + struct.pack("<q", ctime) + csum + struct.pack("<QQ", size, chunk_size)
    return head + bytes(4096 - len(head)) + body, csum


def check_chunk_alignment(size, chunk_size, end, chunk_len):
    """fixed_index.rs:364-392: (code, idx)."""
    if chunk_size & (chunk_size - 1):
        return ERR_NOT_POW2, 0
    end &= NONE  # (usize arithmetic wraps in a release build)
    if end < chunk_len or end > size:
        return ERR_INVALID, 0
    if (end != size and chunk_len != chunk_size) or chunk_len > chunk_size or chunk_len == 0:
        return ERR_INVALID, 0
    pos = end - chunk_len
    if pos & (chunk_size - 1):
        return ERR_INVALID, 0
    return 0, pos // chunk_size


# ---- the model ------------------------------------------------------------------------------------

def _log2_for(m):
    l = 6
    while (1 << l) < 2 * m:
        l += 1
    return l


class Model:
    """One session over a listing [(digest, file length, magic)]."""

    def __init__(self, oracle, listing, reserve=0):
        self.oracle = oracle
        self.entries = [dict(digest=dg, present=1, size=sz, kind=kd, known=0, known_size=0) for dg, sz, kd in listing]
        self.pos = {}
        for j, e in enumerate(self.entries):
            self.pos.setdefault(e["digest"], j)
        self.L = _log2_for(len(listing) + reserve)
        self.finished, self.uid, self.files, self.size = False, 0, 0, 0
        self.stat = dict(count=0, size=0, compressed_size=0, duplicates=0)
        self.writers = {}

    def _grow(self, n):
        c = len(self.entries)
        if 2 * (c + n) > (1 << self.L):
            self.L = _log2_for(c + n) + 1

    def _entry(self, dg):
        if dg not in self.pos:
            self.pos[dg] = len(self.entries)
            self.entries.append(dict(digest=dg, present=0, size=0, kind=KIND_NONE, known=0, known_size=0))
        return self.entries[self.pos[dg]]

    def state(self):
        return (len(self.entries), self.L,
                [(e["digest"], e["present"], e["size"], e["kind"], e["known"], e["known_size"]) for e in self.entries])

    def stats(self):
        return dict(file_counter=self.files, backup_size=self.size, **self.stat, open_writers=len(self.writers),
                    finished=int(self.finished))

    def lookup(self, dg):
        if self.finished:
            return None
        e = self.entries[self.pos[dg]] if dg in self.pos else None
        return e["known_size"] if e and e["known"] else None

    def register(self, digests, sizes):
        if self.finished:
            return E_FINISHED
        if digests:
            self._grow(len(digests))
        for dg, sz in zip(digests, sizes):
            e = self._entry(dg)
            e["known"], e["known_size"] = 1, sz
        return 0

    def register_image(self, image):
        """download_previous: every chunk of the index with its chunk_info length; None for an
        image the index readers refuse."""
        if len(image) < 4096:
            return None
        body = image[4096:]
        if image[:8] == DIDX_MAGIC:
            if len(body) % 40:
                return None
            ends = [struct.unpack("<Q", body[i:i + 8])[0] for i in range(0, len(body), 40)]
            if any(a > b for a, b in zip(ends, ends[1:])):
                return None
            digests = [body[i + 8:i + 40] for i in range(0, len(body), 40)]
            sizes = [e - p for p, e in zip([0] + ends, ends)]
        elif image[:8] == FIDX_MAGIC:
            size, cs = struct.unpack("<QQ", image[64:80])
            if cs == 0 or size == 0 or cs & (cs - 1) or -(-size // cs) * 32 != len(body):
                return None
            digests = [body[i:i + 32] for i in range(0, len(body), 32)]
            sizes = [min(cs, size - i * cs) for i in range(len(digests))]
        else:
            return None
        return self.register(digests, sizes), len(digests)

    def upload(self, wid, items):
        """items: [(digest, size, blob, encoded size or None)]."""
        out = {k: [0] * len(items) for k in UPLOAD_KEYS}
        out["first_failed"] = NONE
        if self.finished:
            return E_FINISHED, out
        if wid not in self.writers:
            return E_NO_WRITER, out
        w = self.writers[wid]
        if items:
            self._grow(len(items))
        for t, (dg, size, blob, enc) in enumerate(items):
            enc = len(blob) if enc is None else enc
            if not 1 <= size <= MAX_CHUNK or not 13 <= enc <= MAX_CHUNK + 44:
                st, kind, crc = BAD_PARAM, KIND_NONE, 0
            elif len(blob) != enc:
                st, kind, crc = WRONG_LENGTH, KIND_NONE, 0
            else:
                kind, st, crc = upload_verdict(self.oracle, blob, dg, size)
            out["status"][t], out["crc"][t] = st, crc
            ok = False
            if st == d.OK:
                e, n = self._entry(dg), len(blob)
                if not e["present"]:
                    ins = INS_NEW
                elif e["kind"] == KIND_NOT_FILE:
                    ins = INS_ERR_TYPE
                elif n == e["size"]:
                    ins = INS_DUP_SAME
                elif e["size"] == 0:
                    ins = INS_OVERWRITE_EMPTY
                elif kind >= 2:
                    if e["kind"] == KIND_NONE:
                        ins = INS_ERR_READ
                    elif e["kind"] in (0, 1):
                        ins = INS_ERR_UNENC_TO_ENC
                    elif e["kind"] == 2 and kind == 2:
                        ins = INS_ERR_ENC_UNCOMPRESSED
                    else:
                        ins = INS_DUP_KEEP_FIRST
                elif e["size"] < n:
                    ins = INS_DUP_KEEP_SMALLER
                else:
                    ins = INS_REPLACE_BIGGER
                out["ins"][t] = ins
                if ins in (INS_NEW, INS_OVERWRITE_EMPTY, INS_REPLACE_BIGGER):
                    e["present"], e["size"], e["kind"] = 1, n, kind
                    out["action"][t], out["compressed_size"][t] = ACT_WRITE, n
                elif ins in (INS_DUP_SAME, INS_DUP_KEEP_FIRST, INS_DUP_KEEP_SMALLER):
                    out["action"][t], out["is_duplicate"][t] = ACT_TOUCH, 1
                    out["compressed_size"][t] = e["size"] & 0xFFFFFFFF
                if ins < 16:  # register_fixed_chunk / register_dynamic_chunk
                    reg = REG_OK
                    if w["fixed"]:
                        if size > w["chunk_size"]:
                            reg = REG_ERR_LARGE
                        elif size < w["chunk_size"]:
                            w["small"] += 1
                            if w["small"] > 1:
                                reg = REG_ERR_MULTI_SMALL
                    out["reg"][t] = reg
                    if reg == REG_OK:
                        ok = True
                        s = w["stat"]
                        s["count"] += 1
                        s["size"] += size
                        s["compressed_size"] += out["compressed_size"][t]
                        s["duplicates"] += out["is_duplicate"][t]
                        e["known"], e["known_size"] = 1, size
            if not ok and out["first_failed"] == NONE:
                out["first_failed"] = t
        return 0, out

    def _new_writer(self, w):
        if self.uid >= 256:
            return E_TOO_MANY_WRITERS, 0
        self.uid += 1
        w.update(chunk_count=0, stat=dict(count=0, size=0, compressed_size=0, duplicates=0))
        self.writers[self.uid] = w
        return 0, self.uid

    def create_dynamic(self):
        if self.finished:
            return E_FINISHED, 0
        return self._new_writer(dict(fixed=False, offset=0, ends=[], digests=[]))

    def create_fixed(self, size, chunk_size, reuse_image=None, reuse_csum=None):
        if self.finished:
            return E_FINISHED, 0
        n = -(-size // chunk_size)
        w = dict(fixed=True, size=size, chunk_size=chunk_size, n=n, digests=[bytes(32)] * n, small=0,
                 incremental=reuse_csum is not None)
        if reuse_csum is not None:
            img = reuse_image
            if img is None or len(img) < 4096 or img[:8] != FIDX_MAGIC:
                return E_REUSE_NO_IMAGE, 0
            psize, pcs = struct.unpack("<QQ", img[64:80])
            if pcs == 0 or psize == 0 or pcs & (pcs - 1) or -(-psize // pcs) * 32 != len(img) - 4096:
                return E_REUSE_NO_IMAGE, 0
            if hashlib.sha256(img[4096:]).digest() != reuse_csum:
                return E_REUSE_CSUM, 0
            if -(-psize // pcs) != n:
                return E_REUSE_LENGTH, 0
            w["digests"] = [img[4096 + 32 * i:4128 + 32 * i] for i in range(n)]
        return self._new_writer(w)

    def _writer(self, wid, fixed):
        w = self.writers.get(wid)
        return w if w is not None and w["fixed"] == fixed else None

    def dynamic_append(self, wid, digests, offsets):
        if self.finished:
            return E_FINISHED, 0, 0
        w = self._writer(wid, False)
        if w is None:
            return E_NO_WRITER, 0, 0
        for i, (dg, off) in enumerate(zip(digests, offsets)):
            e = self.entries[self.pos[dg]] if dg in self.pos else None
            if e is None or not e["known"]:
                return 0, i, E_NO_SUCH_CHUNK
            if off != w["offset"]:
                return 0, i, E_STRANGE_OFFSET
            w["offset"] += e["known_size"]
            w["chunk_count"] += 1
            w["ends"].append(w["offset"])
            w["digests"].append(dg)
        return 0, len(digests), 0

    def fixed_append(self, wid, digests, offsets):
        if self.finished:
            return E_FINISHED, 0, 0
        w = self._writer(wid, True)
        if w is None:
            return E_NO_WRITER, 0, 0
        for i, (dg, off) in enumerate(zip(digests, offsets)):
            e = self.entries[self.pos[dg]] if dg in self.pos else None
            if e is None or not e["known"]:
                return 0, i, E_NO_SUCH_CHUNK
            code, idx = check_chunk_alignment(w["size"], w["chunk_size"], off + e["known_size"], e["known_size"])
            if code:
                return 0, i, code
            if idx >= w["n"]:
                return 0, i, E_INDEX_RANGE
            w["chunk_count"] += 1
            w["digests"][idx] = dg
        return 0, len(digests), 0

    def _close(self, wid, fixed, chunk_count, size, csum):
        if self.finished:
            return E_FINISHED, 0, None, None
        w = self._writer(wid, fixed)
        if w is None:
            return 0, E_NO_WRITER, None, None
        del self.writers[wid]
        if w["chunk_count"] != chunk_count:
            return 0, E_CHUNK_COUNT, None, None
        if fixed:
            if not w["incremental"]:
                if chunk_count != w["n"]:
                    return 0, E_EXPECTED_COUNT, None, None
                if size != w["size"]:
                    return 0, E_SIZE, None, None
            image, expect = fidx_image(w["digests"], w["size"], w["chunk_size"])
        else:
            if w["offset"] != size:
                return 0, E_SIZE, None, None
            image, expect = didx_image(w["ends"], w["digests"])
        if csum != expect:
            return 0, E_CSUM, None, None
        s = w["stat"]
        st = dict(s, chunk_count=chunk_count, archive_size=size, upload_percent=0, client_duplicates=0,
                  server_duplicates=0, duplicate_percent=0, compression_percent=0, logged=0)
        if size != 0 and chunk_count != 0:  # log_upload_stat
            st["logged"] = 1
            st["upload_percent"] = s["size"] * 100 // size
            st["client_duplicates"] = max(chunk_count - s["count"], 0)
            st["server_duplicates"] = s["duplicates"]
            dups = st["client_duplicates"] + st["server_duplicates"]
            if dups > 0:
                st["duplicate_percent"] = dups * 100 // chunk_count
            if s["size"] > 0:
                st["compression_percent"] = s["compressed_size"] * 100 // s["size"]
        self.files += 1
        self.size += size
        for k in self.stat:
            self.stat[k] += s[k]
        return 0, 0, image, st

    def dynamic_close(self, wid, chunk_count, size, csum):
        return self._close(wid, False, chunk_count, size, csum)

    def fixed_close(self, wid, chunk_count, size, csum):
        return self._close(wid, True, chunk_count, size, csum)

    def add_blob(self, raw):
        if self.finished:
            return E_FINISHED, d.TOO_SMALL
        if len(raw) < d.HDR:
            return 0, d.TOO_SMALL
        if raw[:8] not in d.MAGICS:
            return 0, d.BAD_MAGIC
        h = d.EHDR if d.MAGICS.index(raw[:8]) >= 2 else d.HDR
        if len(raw) < h:
            return 0, d.TOO_SMALL
        if struct.unpack("<I", raw[8:12])[0] != zlib.crc32(raw[h:]):
            return 0, d.BAD_CRC
        self.files += 1
        self.size += len(raw)
        self.stat["size"] += len(raw)
        return 0, d.OK

    def finish(self):
        if self.finished:
            return E_FINISHED
        if self.writers:
            return E_OPEN_WRITER
        if self.files == 0:
            return E_NO_FILES
        self.finished = True
        return 0


# ---- a library session behind the model's interface ------------------------------------------------

def rows(digests):
    return np.frombuffer(b"".join(digests), dtype=np.uint8).reshape(-1, 32).copy() if digests else np.zeros((0, 32), np.uint8)


class Session:
    """pbschunk.BackupSession with the model's arguments and plain Python results.  `upload`: from
    a uint8 array to (what BackupSession.upload takes, something to keep alive)."""

    def __init__(self, pbschunk, listing, reserve=0, device=False, upload=None):
        lst = (rows([x[0] for x in listing]), [x[1] for x in listing], [x[2] for x in listing])
        self.s = pbschunk.BackupSession(lst, reserve=reserve, device=device)
        self.up = upload or (lambda arr: (arr, None))

    def close(self):
        self.s.close()

    def state(self):
        l = self.s.listing()
        ents = [(l["digests"][j].tobytes(), int(l["present"][j]), int(l["size"][j]), int(l["kind"][j]), int(l["known"][j]),
                 int(l["known_size"][j])) for j in range(l["present"].size)]
        return self.s.count, self.s.table_log2, ents

    def stats(self):
        return self.s.stats()

    def lookup(self, dg):
        return self.s.lookup(dg)

    def register(self, digests, sizes):
        return self.s.register_previous(rows(digests), sizes)

    def register_image(self, image):
        try:
            return self.s.register_index_image(image)
        except Exception as e:
            if getattr(e, "code", 0) not in (ERR_INVALID, ERR_NOT_POW2):
                raise
            return None

    def upload(self, wid, items):
        raw = np.frombuffer(b"".join(x[2] for x in items), dtype=np.uint8)
        off = np.concatenate([[0], np.cumsum([len(x[2]) for x in items])]).astype(np.uint64)
        enc = None
        if any(x[3] is not None for x in items):
            enc = [len(x[2]) if x[3] is None else x[3] for x in items]
        ptr, keep = self.up(raw)
        rc, out = self.s.upload(wid, rows([x[0] for x in items]), [x[1] for x in items], ptr, off, enc)
        del keep
        res = {k: [int(y) for y in out[k]] for k in UPLOAD_KEYS}
        res["first_failed"] = out["first_failed"]
        return rc, res

    def create_dynamic(self):
        return self.s.create_dynamic()

    def create_fixed(self, size, chunk_size, reuse_image=None, reuse_csum=None):
        return self.s.create_fixed(size, chunk_size, reuse_image=reuse_image, reuse_csum=reuse_csum)

    def dynamic_append(self, wid, digests, offsets):
        return self.s.dynamic_append(wid, rows(digests), offsets)

    def fixed_append(self, wid, digests, offsets):
        return self.s.fixed_append(wid, rows(digests), offsets)

    def dynamic_close(self, wid, chunk_count, size, csum):
        return self.s.dynamic_close(wid, chunk_count, size, csum)

    def fixed_close(self, wid, chunk_count, size, csum):
        return self.s.fixed_close(wid, chunk_count, size, csum)

    def add_blob(self, raw):
        return self.s.add_blob(raw)

    def finish(self):
        return self.s.finish()


# ---- planted cases --------------------------------------------------------------------------------
# Each case: (label, listing, reserve, script).  script(oracle, s, log) drives `s` (a Model or a
# Session) and calls log(name, value) with everything it gets back.

_chunks = {}


def chunk(tag, n=68):
    """(digest, chunk) of a small incompressible chunk."""
    if (tag, n) not in _chunks:
        c = rnd([7, tag], n)
        _chunks[tag, n] = (hashlib.sha256(c).digest(), c)
    return _chunks[tag, n]


def item(tag, n=68, blocks=0):
    """An upload item of chunk (tag, n): kind 0, or kind 1 in `blocks` raw blocks."""
    dg, c = chunk(tag, n)
    return dg, n, frame_blob(c, blocks) if blocks else plain_blob(c), None


def enc_item(tag, kind=2, n=1, size=4096):
    """An encrypted upload under a digest of its own: a 44 + n byte blob."""
    return rnd([8, tag], 32), size, enc_blob(kind, n, [9, tag, kind, n]), None


def _listing(m, dup=True):
    """m listed chunks (random digests, lengths 50 + j, kinds 0 1 2 3 in turn); with `dup` the last
    entry repeats the digest of entry 0 with another state: the lowest position is the chunk."""
    out = [(rnd([1, j], 32), 50 + j, j % 4) for j in range(m)]
    if dup and m >= 2:
        out[m - 1] = (out[0][0], 999, 2)
    return out


def _sizes_script(k, m):
    def script(oracle, s, log):
        log("wid", s.create_dynamic())
        lst = _listing(m)
        items = []
        for t in range(k):
            if t % 7 == 3 and lst:  # a listed digest: kinds 2 / 3 against the listing's kinds
                dg = lst[t % len(lst)][0]
                items.append((dg, 4096, enc_blob(2 + t % 2, 1 + t % 5, [2, t]), None))
            elif t % 5 == 0:
                items.append(item(1000 + t % 11))  # repeats every 55 items
            else:
                items.append(enc_item(t, 2 + t % 2, 1 + t % 3))
        log("upload", s.upload(1, items))
        log("state", s.state())
        digs = [x[0] for x in items]
        log("register", s.register(digs[::-1], list(range(1, k + 1))))
        log("state2", s.state())
        # an append of the same k entries: the length of a digest is what its highest i registered
        ks = dict(zip(digs[::-1], range(1, k + 1)))
        offs = [0]
        for dg in digs:
            offs.append(offs[-1] + ks[dg])
        log("wid2", s.create_dynamic())
        log("append", s.dynamic_append(2, digs, offs[:k]))
        log("close", s.dynamic_close(2, k, offs[k], didx_image(offs[1:], digs)[1]))
        log("wid3", s.create_fixed(max(1, 16 * k), 16))
        log("fixed-append", s.fixed_append(3, digs, [16 * (k - 1 - i) for i in range(k)]))
    return script


def _matrix_script(kind_in):
    """Every entry state against one incoming kind: each state under a chunk of its own."""
    states = ["absent", "equal", "empty", "k0-bigger", "k0-smaller", "k1-bigger", "k1-smaller", "k2-bigger", "k2-smaller",
              "k3-bigger", "k3-smaller", "none", "not-file"]

    def incoming(j):
        dg, c = chunk(2000 + j)
        if kind_in == 0:
            return dg, len(c), plain_blob(c), None
        if kind_in == 1:
            return dg, len(c), frame_blob(c, 2), None
        return dg, len(c), enc_blob(kind_in, 60, [3, j]), None

    def listing():
        out = []
        for j, name in enumerate(states):
            dg, _, blob, _ = incoming(j)
            n = len(blob)
            if name == "absent":
                continue
            size = {"equal": n, "empty": 0, "none": n + 1, "not-file": n}.get(name)
            kind = {"equal": kind_in, "empty": KIND_NONE, "none": KIND_NONE, "not-file": KIND_NOT_FILE}.get(name)
            if size is None:
                kind = int(name[1])
                size = n + 5 if name.endswith("bigger") else n - 5
            out.append((dg, size, kind))
        return out

    def script(oracle, s, log):
        log("wid", s.create_dynamic())
        log("upload", s.upload(1, [incoming(j) for j in range(len(states))]))
        log("state", s.state())
    return listing(), script


def _chain_script(copies, k):
    """One digest `copies` times in a batch of k: at t = 0, 63, 64, 255, 256 and k - 1 as far as they
    exist, then wherever there is room; lengths 98 / 80 / 89 in turn, in both orders."""
    def script(oracle, s, log):
        for order in ((4, 0, 1), (0, 4, 1)):
            log("wid", s.create_dynamic())
            wid = 1 if order == (4, 0, 1) else 2
            tag = 3000 + copies * 10 + order[0]
            spots = [t for t in (0, 63, 64, 255, 256, k - 1) if t < k]
            spots = sorted(set(spots + list(range(1, k, max(1, k // (copies + 1))))))[:copies] if copies > len(spots) \
                else spots[:copies - 1] + [k - 1]
            spots = sorted(set(spots))
            items = [enc_item(40000 + copies * 1000 + t, 3, 1) for t in range(k)]
            for q, t in enumerate(spots):
                items[t] = item(tag, 68, order[q % 3])
            log("spots", spots)
            log("upload", s.upload(wid, items))
            log("state", s.state())
    return script


def _chain_special(oracle, s, log):
    """A failed item in the middle of a chain that changes nothing; an encrypted copy after an
    unencrypted one in the same batch; two encrypted uploads of one digest with different sizes; a
    wrong stored CRC that is accepted."""
    log("wid", s.create_dynamic())
    dg, c = chunk(3500)
    good0, good1 = plain_blob(c), frame_blob(c, 3)
    bad = plain_blob(c[:-1] + bytes([c[-1] ^ 1]))           # BAD_DIGEST
    short = plain_blob(c[:-1])                              # BAD_DIGEST or BAD_SIZE by the verdict
    wrong_crc = d._flip(good0, 9, 2)                        # accepted: the CRC is recomputed
    items = [(dg, 68, good1, None), (dg, 68, bad, None), (dg, 68, wrong_crc, None), (dg, 68, short, None),
             (dg, 68, enc_blob(2, 10, [4, 1]), None), (dg, 68, good1, None), (dg, 69, good0, None),
             (dg, 68, good0, len(good0) + 1), (dg, 0, good0, None), (dg, 68, d._flip(good0, 0, 1), None),
             (dg, 68, frame_blob(c, 1)[:-3], None)]
    log("upload", s.upload(1, items))
    e = rnd([4, 2], 32)
    log("enc-sizes", s.upload(1, [(e, 100, enc_blob(2, 7, [4, 3]), None), (e, 200, enc_blob(2, 7, [4, 4]), None),
                                  (e, 300, enc_blob(3, 9, [4, 5]), None), (e, 400, enc_blob(2, 9, [4, 6]), None),
                                  (e, 500, enc_blob(2, 3, [4, 7])[:43], None)]))
    log("lookup", [s.lookup(dg), s.lookup(e), s.lookup(rnd([4, 8], 32))])
    log("state", s.state())


def _fixed_small(oracle, s, log):
    """Small chunks of a fixed writer: at t = 255 and 256 of one batch; one in an earlier batch and
    one later; a large chunk; the count keeps rising after a failure."""
    cs = 64
    log("wid", s.create_fixed(64 * 300, cs))
    log("wid", s.create_fixed(64 * 300, cs))
    full = lambda t: item(5000 + t, 64)
    items = [full(t) for t in range(300)]
    items[255], items[256] = item(5300, 63), item(5301, 10)
    items[10] = item(5302, 65)                               # large
    items[299] = (items[5][0], 64, items[5][2], None)        # a repeat
    log("batch", s.upload(1, items))
    log("earlier", s.upload(2, [full(400), item(5303, 5), full(401)]))
    log("later", s.upload(2, [full(402), item(5304, 6), item(5305, 65), item(5306, 7), full(403)]))
    log("lookup", [s.lookup(item(5300 + j, n)[0]) for j, n in ((0, 63), (1, 10), (2, 65), (3, 5), (4, 6), (6, 7))])
    log("state", s.state())


def _known(oracle, s, log):
    """known_chunks: the highest i wins across the 255 / 256 edge; a later call overwrites; chunks
    known but absent from the store are appended to an index."""
    digs = [rnd([6, i], 32) for i in range(300)]
    digs[256] = digs[255]
    digs[299] = digs[0]
    digs[64] = digs[63]
    digs[150] = _listing(33)[0][0]                           # a listed digest (twice in the listing)
    log("register", s.register(digs, [1000 + i for i in range(300)]))
    log("lookup", [s.lookup(digs[i]) for i in (0, 63, 64, 150, 255, 256, 299)])
    log("again", s.register(digs[250:260], [7] * 10))
    log("lookup2", [s.lookup(digs[i]) for i in (249, 250, 255, 259, 260)])
    log("empty", s.register([], []))
    # the same from index images: a .didx with a repeat and a zero-length chunk, a .fidx with a clipped last chunk
    dd = [digs[10], rnd([6, 1000], 32), digs[10], rnd([6, 1001], 32)]
    log("didx", s.register_image(didx_image([500, 500, 1700, 1701], dd)[0]))
    ff = [rnd([6, 1002 + i], 32) for i in range(3)] + [digs[11]]
    log("fidx", s.register_image(fidx_image(ff, 3 * 64 + 9, 64)[0]))
    log("lookup3", [s.lookup(x) for x in dd + ff])
    for name, img in (("cut", didx_image([5], [dd[0]])[0][:-1]), ("magic", b"x" + didx_image([5], [dd[0]])[0][1:]),
                      ("descending", didx_image([9, 5], dd[:2])[0]), ("short", fidx_image(ff, 64 * 4, 64)[0][:-32]),
                      ("empty-didx", didx_image([], [])[0])):
        log("bad-" + name, s.register_image(img))
    log("wid", s.create_dynamic())
    log("append", s.dynamic_append(1, [digs[1], digs[2], digs[255]], [0, 1001, 2003]))
    log("state", s.state())


def _dynamic_append(oracle, s, log):
    """Each error at i in {0, 63, 64, 255, 256, n - 1}, both in one call, offsets over several calls,
    and 1000 entries of 16 MiB: the running sum passes 2^32."""
    n = 300
    digs = [rnd([10, i], 32) for i in range(n)]
    sizes = [1 + (i * 37) % 500 for i in range(n)]
    log("register", s.register(digs, sizes))
    unknown = rnd([10, 9999], 32)
    offs = [0]
    for x in sizes:
        offs.append(offs[-1] + x)
    w = 0
    for at in (0, 63, 64, 255, 256, n - 1):
        for what in ("chunk", "offset", "both", "two"):
            w += 1
            log("wid", s.create_dynamic())
            dd, oo = list(digs), list(offs[:n])
            if what in ("chunk", "both"):
                dd[at] = unknown
            if what in ("offset", "both"):
                oo[at] += 1
            if what == "two":                                # the lowest wins
                oo[at] += 1
                for later in (at + 1, at + 70, n - 1):
                    if at < later < n:
                        dd[later] = unknown
            log(f"append-{at}-{what}", s.dynamic_append(w, dd, oo))
            # the entries before the failure stay appended: the close says so
            log("close", s.dynamic_close(w, at, offs[at], didx_image(offs[1:at + 1], digs[:at])[1]))
    w += 1
    log("wid", s.create_dynamic())
    log("part1", s.dynamic_append(w, digs[:100], offs[:100]))
    log("part-empty", s.dynamic_append(w, [], []))
    log("part2", s.dynamic_append(w, digs[100:257], offs[100:257]))
    log("part3", s.dynamic_append(w, digs[257:], offs[257:n]))
    log("close", s.dynamic_close(w, n, offs[n], didx_image(offs[1:], digs)[1]))
    big = rnd([10, 5], 32)
    log("register-big", s.register([big], [MAX_CHUNK]))
    w += 1
    log("wid", s.create_dynamic())
    log("big", s.dynamic_append(w, [big] * 1000, [i * MAX_CHUNK for i in range(1000)]))
    log("big-more", s.dynamic_append(w, [big, big, big], [1000 * MAX_CHUNK, 1001 * MAX_CHUNK, 1002 * MAX_CHUNK + 1]))
    ends = [(i + 1) * MAX_CHUNK for i in range(1002)]
    log("big-close", s.dynamic_close(w, 1002, 1002 * MAX_CHUNK, didx_image(ends, [big] * 1002)[1]))
    log("wrong-kind", s.fixed_append(w, [big], [0]))
    log("no-writer", s.dynamic_append(99, [big], [0]))
    log("stats", s.stats())


def _fixed_append(oracle, s, log):
    """Every clause of check_chunk_alignment, offsets out of order, one idx twice, and the
    incremental writer with a matching checksum, a wrong one and a wrong length."""
    cs, size = 4096, 4096 * 9 + 100
    full = [rnd([11, i], 32) for i in range(12)]
    last, tiny, zero, big = rnd([11, 100], 32), rnd([11, 101], 32), rnd([11, 102], 32), rnd([11, 103], 32)
    log("register", s.register(full + [last, tiny, zero, big], [cs] * 12 + [100, 50, 0, cs + 1]))
    log("wid", s.create_fixed(size, cs))
    order = [5, 0, 8, 3, 3, 1]
    log("out-of-order", s.fixed_append(1, [full[i] for i in order[:4]] + [full[9], full[1]], [i * cs for i in order]))
    for name, dg, off in (("small-offset", full[0], NONE - 10), ("exceeds", full[0], 9 * cs), ("short-not-last", tiny, 0),
                          ("long", big, 0), ("zero", zero, cs), ("unaligned", full[0], 100), ("last-unaligned", last, 9 * cs - 1),
                          ("unknown", rnd([11, 200], 32), 0)):
        log(name, s.fixed_append(1, [full[2], dg, full[4]], [2 * cs, off, 4 * cs]))
    log("last", s.fixed_append(1, [last], [9 * cs]))
    want = [full[0], full[1], full[2], full[9], bytes(32), full[5], bytes(32), bytes(32), full[8], last]
    image, csum = fidx_image(want, size, cs)
    log("close-count", s.fixed_close(1, 10, size, csum))       # 15 appended: chunk count
    log("wid", s.create_fixed(size, cs))
    log("fill", s.fixed_append(2, [full[i] for i in range(9)] + [last], [i * cs for i in range(10)]))
    image, csum = fidx_image(full[:9] + [last], size, cs)
    log("close", s.fixed_close(2, 10, size, csum))
    # incremental
    log("reuse-csum", s.create_fixed(size, cs, image, bytes(32)))
    log("reuse-length", s.create_fixed(size + cs, cs, image, csum))
    log("reuse-cut", s.create_fixed(size, cs, image[:-1], csum))
    log("reuse-none", s.create_fixed(size, cs, None, csum))
    log("reuse", s.create_fixed(size, cs, image, csum))
    log("inc-append", s.fixed_append(3, [full[10], full[11], full[6]], [3 * cs, 7 * cs, 3 * cs]))
    inc = list(full[:9]) + [last]
    inc[3], inc[7] = full[6], full[11]                         # one idx twice: the higher i wins
    log("inc-close", s.fixed_close(3, 3, 12345, fidx_image(inc, size, cs)[1]))   # no count or size check
    log("wid", s.create_fixed(1000, 3))                        # no power of two: the append says so
    log("not-pow2", s.fixed_append(4, [full[0]], [0]))
    log("stats", s.stats())


def _growth(oracle, s, log):
    """Uploads and registers beyond the reserve: L as the mirror's."""
    log("wid", s.create_dynamic())
    for step in range(4):
        n = 40 << step
        log(f"upload{step}", s.upload(1, [enc_item(60000 + step * 1000 + t, 2, 1) for t in range(n)])[1]["first_failed"])
        log(f"L{step}", s.state()[:2])
        log(f"register{step}", s.register([rnd([12, step, i], 32) for i in range(n + 3)], [5] * (n + 3)))
        log(f"L'{step}", s.state()[:2])
    log("state", s.state())


def _close_finish(oracle, s, log):
    """Every failing check of the closes in its order, an unknown wid, finish with an open writer
    and with no files, add_blob, and every call after finish."""
    a, b = item(7000), item(7001)
    log("finish-empty", s.finish())
    log("wid", s.create_dynamic())
    log("finish-open", s.finish())
    log("upload", s.upload(1, [a, b, a]))
    log("append", s.dynamic_append(1, [a[0], b[0], a[0]], [0, 68, 136]))
    ends, digs = [68, 136, 204], [a[0], b[0], a[0]]
    csum = didx_image(ends, digs)[1]
    log("close-count", s.dynamic_close(1, 2, 204, csum))
    log("close-gone", s.dynamic_close(1, 3, 204, csum))
    for wid, (cnt, size, cs) in enumerate(((3, 203, csum), (3, 204, bytes(32)), (3, 204, csum)), start=2):
        log("wid", s.create_dynamic())
        log("append", s.dynamic_append(wid, digs, [0, 68, 136]))
        log(f"close{wid}", s.dynamic_close(wid, cnt, size, cs))
    log("close-unknown", s.fixed_close(77, 0, 0, bytes(32)))
    log("wid", s.create_fixed(128, 64))
    log("fixed-close-dynamic", s.dynamic_close(5, 0, 0, bytes(32)))
    log("fixed-upload", s.upload(5, [item(7002, 64), item(7003, 64)]))
    log("fixed-append", s.fixed_append(5, [item(7002, 64)[0]], [0]))
    f2 = fidx_image([item(7002, 64)[0], bytes(32)], 128, 64)[1]
    log("fixed-expected", s.fixed_close(5, 1, 128, f2))
    log("wid", s.create_fixed(128, 64))
    log("fixed-append", s.fixed_append(6, [item(7002, 64)[0], item(7003, 64)[0]], [0, 64]))
    f3 = fidx_image([item(7002, 64)[0], item(7003, 64)[0]], 128, 64)[1]
    log("fixed-size", s.fixed_close(6, 2, 127, f3))
    log("wid", s.create_fixed(128, 64))
    log("fixed-append", s.fixed_append(7, [item(7002, 64)[0], item(7003, 64)[0]], [0, 64]))
    log("fixed-csum", s.fixed_close(7, 2, 128, f2))
    log("wid", s.create_fixed(128, 64))
    log("fixed-append", s.fixed_append(8, [item(7002, 64)[0], item(7003, 64)[0]], [0, 64]))
    log("fixed-ok", s.fixed_close(8, 2, 128, f3))
    log("empty-dynamic", s.create_dynamic())
    log("empty-close", s.dynamic_close(9, 0, 0, hashlib.sha256(b"").digest()))
    manifest = plain_blob(b'{"files": []}')
    log("blob-bad-crc", s.add_blob(d._flip(manifest, 20, 0)))
    log("blob-short", s.add_blob(manifest[:7]))
    log("blob-magic", s.add_blob(d._flip(manifest, 1, 0)))
    log("blob-enc-short", s.add_blob(enc_blob(2, 4, [13, 1])[:40]))
    log("blob", s.add_blob(manifest))
    log("blob-enc", s.add_blob(enc_blob(3, 9, [13, 2])))
    log("stats", s.stats())
    log("finish", s.finish())
    log("after", [s.finish(), s.register([a[0]], [1]), s.upload(1, [a])[0], s.create_dynamic(), s.create_fixed(10, 2),
                  s.dynamic_append(1, [a[0]], [0]), s.fixed_append(1, [a[0]], [0]), s.dynamic_close(1, 0, 0, bytes(32))[:2],
                  s.fixed_close(1, 0, 0, bytes(32))[:2], s.add_blob(manifest)[0], s.lookup(a[0])])
    log("stats-after", s.stats())
    log("state", s.state())


def _compressed(oracle, s, log):
    """Real zstd frames (the oracle's encoder) of 5000 and 70001 bytes beside kind 0, and a frame
    the inflater must refuse, through the upload."""
    log("wid", s.create_dynamic())
    items = []
    for seed, n in ((1, 5000), (2, 70001), (3, 4097)):
        c = d._chunk(8000 + seed, n, True)
        blob = oracle.blob_compressed(c)
        assert d.kind_of(blob) == 1
        items.append((hashlib.sha256(c).digest(), n, blob, None))
        items.append((hashlib.sha256(c).digest(), n, plain_blob(c), None))       # REPLACE? no: bigger, the smaller stays
        items.append((hashlib.sha256(c).digest(), n + 1, blob, None))            # BAD_SIZE
        items.append((hashlib.sha256(c).digest(), n - 1, blob, None))            # longer than announced: BAD_DIGEST
    items.append((items[0][0], 5000, d._flip(items[0][2], d.HDR, 0), None))      # the frame's magic: BAD_FRAME
    log("upload", s.upload(1, items))
    log("state", s.state())


def cases():
    out = []
    for k in BOUNDARY:
        out.append((f"sizes/k{k}/m33", _listing(33), 0, _sizes_script(k, 33)))
    for m in (0, 1, 31, 32, 33):
        out.append((f"sizes/k257/m{m}", _listing(m), 0, _sizes_script(257, m)))
    for kind_in in range(4):
        lst, script = _matrix_script(kind_in)
        out.append((f"matrix/kind{kind_in}", lst, 0, script))
    for copies, k in ((2, 2), (3, 65), (3, 3), (64, 257), (65, 300), (6, 1000)):
        out.append((f"chain/{copies}-in-{k}", _listing(5), 0, _chain_script(copies, k)))
    out.append(("chain/special", _listing(3), 0, _chain_special))
    out.append(("fixed-small", [], 8, _fixed_small))
    out.append(("known", _listing(33), 0, _known))
    out.append(("dynamic-append", _listing(31), 400, _dynamic_append))
    out.append(("fixed-append", _listing(4), 0, _fixed_append))
    out.append(("growth", _listing(3), 10, _growth))
    out.append(("close-finish", [], 0, _close_finish))
    out.append(("compressed", [], 0, _compressed))
    return out


def case(label):
    return next(c for c in cases() if c[0] == label)


_expected = {}


def expected(oracle, c):
    """The model's log of a case, computed once."""
    if c[0] not in _expected:
        _expected[c[0]] = run(oracle, c, Model(oracle, c[1], c[2]))
    return _expected[c[0]]


def run(oracle, c, s):
    log = []
    c[3](oracle, s, lambda name, value: log.append((name, _plain(value))))
    return log


def _plain(x):
    """Tuples, lists, dicts, ints and bytes all the way down, so the logs compare with ==."""
    if isinstance(x, dict):
        return {k: _plain(y) for k, y in x.items()}
    if isinstance(x, (list, tuple)):
        return [_plain(y) for y in x]
    if isinstance(x, (bytes, bytearray)):
        return bytes(x)
    if isinstance(x, np.ndarray):
        return [_plain(y) for y in x.tolist()]
    return x if x is None else int(x)


def diff(got, want):
    """The first entries of two logs that differ, shortened: [] when they agree."""
    out = []
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            out.append((i, g[0], _where(g[1], w[1])))
    if len(got) != len(want):
        out.append(("length", len(got), len(want)))
    return out[:5]


def _where(g, w, path=""):
    if type(g) is not type(w):
        return f"{path}: {str(g)[:80]} / {str(w)[:80]}"
    if isinstance(g, dict):
        for k in w:
            if g.get(k) != w[k]:
                return _where(g.get(k), w[k], f"{path}.{k}")
    if isinstance(g, list):
        if len(g) != len(w):
            return f"{path}: lengths {len(g)} / {len(w)}"
        for i, (a, b) in enumerate(zip(g, w)):
            if a != b:
                return _where(a, b, f"{path}[{i}]")
    return f"{path}: {str(g)[:80]} / {str(w)[:80]}"
