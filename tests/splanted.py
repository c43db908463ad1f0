"""Planted inputs for the sync job (include/pbs_sync.h) and a Python model of the reference
(helpers of test_sync_cpu.py and test_gpu_sync.py; not a conftest).

The model is a transliteration of `pull_index_chunks` (src/server/pull.rs:605-705) over sets and
dicts with a chunk reader that answers at once: the `downloaded_chunks` filter (:616-630),
`cond_touch_chunk` (:657-663), `read_raw_chunk` with its counters (:665-674), `verify_unencrypted`
and `insert_chunk` (:639-642); `verify_archive` (:707-722) in front.  The verdict on a blob comes
from vplanted.verdict, that is from the reference functions of the oracle and tests/aesgcm_ref.py,
never from the library.  Where the reference bails at the first failing chunk the model goes on
(the library reports `first_failed`, the place of the bail, and handles every item).

A planted case is a local listing (digests, all present), a source store (digest -> blob, None for
a blob that cannot be fetched, absent likewise) and a sequence of steps on one worker: an index
to pull, or the start of a new group.
"""
import hashlib
import json
import os
from typing import NamedTuple

import numpy as np

import dplanted as d
import gcplanted
import vplanted as v

DUP, EXISTS, FETCH = 0, 1, 2
LOAD_FAILED = 32
NONE = (1 << 64) - 1
N_SET = (0, 1, 63, 64, 65, 255, 256, 257, 1000)
M_SET = (0, 1, 31, 32, 33)
RESULT_KEYS = ("entries", "dup", "exists", "fetch", "appended", "inserted", "failed", "load_failed", "chunk_count",
               "bytes", "first_failed", "ok")
Index = v.Index  # (name, digests, sizes, mode (unused: the reference has no crypt-mode check here), info)


class Case(NamedTuple):
    label: str
    listing: list   # the local store's digests in listing order (duplicates allowed); every file is there
    reserve: int
    remote: dict    # the source store: digest -> blob bytes, or None
    steps: list     # Index, or None for the start of a new group


# ---- the sizes of the table (the rule of the issue, restated) ---------------------------------------

def begin_log2(m: int, reserve: int) -> int:
    return gcplanted.table_log2(m + reserve)


def plan_log2(count: int, n: int, L: int) -> int:
    """Growth runs before the plan: 2 (count + n) > 2^L rebuilds at table_log2_for(count + n) + 1."""
    return L if 2 * (count + n) <= (1 << L) else gcplanted.table_log2(count + n) + 1


# ---- the model ------------------------------------------------------------------------------------

class Model:
    """One sync worker: `store` is the local chunk store, `downloaded` the set of the group."""

    def __init__(self, oracle, listing, reserve=0):
        self.oracle = oracle
        self.order = list(listing)              # entry position -> digest
        self.m = len(self.order)
        self.pos = {}
        for j, dg in enumerate(self.order):
            self.pos.setdefault(dg, j)          # the lowest position is the chunk
        self.store = set(self.order)
        self.downloaded = set()
        self.L = begin_log2(len(self.order), reserve)

    def new_group(self):
        self.downloaded = set()                 # pull.rs:1134

    def pull_index(self, ix: Index, remote: dict, honest=None):
        out = dict(index_check=0, verdict=[], fetch_store=[], fetch_entry=[], touch_store=[], kinds=[], status=[],
                   inserted=[], result=None)
        if ix.info is not None and honest is not None:  # verify_archive: nothing is pulled
            if ix.info[0] is not None and ix.info[0] != honest[0]:
                out["index_check"] = v.WRONG_SIZE
                return out
            if ix.info[1] is not None and ix.info[1] != honest[1]:
                out["index_check"] = v.WRONG_CSUM
                return out
        res = dict.fromkeys(RESULT_KEYS, 0)
        res["entries"], res["first_failed"] = len(ix.digests), NONE
        self.L = plan_log2(len(self.order), len(ix.digests), self.L)
        for i, (dg, size) in enumerate(zip(ix.digests, ix.sizes)):
            if dg in self.downloaded:                                   # :619-627
                out["verdict"].append(DUP)
                continue
            self.downloaded.add(dg)
            if dg not in self.pos:                                      # (positions are the library's: first met, first numbered)
                self.pos[dg] = len(self.order)
                self.order.append(dg)
                res["appended"] += 1
            if dg in self.store:                                        # cond_touch_chunk: true
                out["verdict"].append(EXISTS)
                out["touch_store"].append(self.pos[dg])
                continue
            out["verdict"].append(FETCH)
            out["fetch_store"].append(self.pos[dg])
            out["fetch_entry"].append(i)
            blob = remote.get(dg)
            if blob is None:                                            # read_raw_chunk fails
                kind, st = d.KIND_NONE, LOAD_FAILED
                res["load_failed"] += 1
            else:
                res["chunk_count"] += 1                                 # :673-674
                res["bytes"] += len(blob)
                kind, st = v.verdict(self.oracle, blob, dg, size)       # verify_unencrypted
                if st == d.OK:
                    self.store.add(dg)                                  # insert_chunk
                    out["inserted"].append(dg)
                    res["inserted"] += 1
                else:
                    res["failed"] += 1
            if st != d.OK and res["first_failed"] == NONE:
                res["first_failed"] = len(out["status"])
            out["kinds"].append(kind)
            out["status"].append(st)
        res["dup"], res["exists"], res["fetch"] = (out["verdict"].count(x) for x in (DUP, EXISTS, FETCH))
        res["ok"] = int(res["failed"] == 0 and res["load_failed"] == 0)
        out["result"] = res
        return out

    def listing(self):
        """(digests in position order, present per position: every listed file is there)."""
        return list(self.order), [int(j < self.m or dg in self.store) for j, dg in enumerate(self.order)]


# ---- planted cases --------------------------------------------------------------------------------

_fills = {}


def fill(oracle, k: int):
    """(digest, blob, size) of the k-th small good chunk of kind 0 (built once per process)."""
    if k not in _fills:
        chunk = np.random.default_rng([0x73796E63, k]).integers(0, 256, 1 + (k * 7919) % 97, dtype=np.uint8).tobytes()
        _fills[k] = (hashlib.sha256(chunk).digest(), oracle.blob_uncompressed(chunk), len(chunk))
    return _fills[k]


def _entries_index(name, entries, info=None):
    return Index(name, [e[0] for e in entries], [e[1] for e in entries], 0, info)


def planted(oracle, m: int, n: int, seed: int = 1) -> Case:
    """A listing of exactly m chunks and one index of exactly n entries: in turn a new chunk the
    source has, a listed chunk, a repeat of an earlier entry, and now and then a chunk the source
    lacks; every special of vplanted (all four kinds good, every corruption, a load failure,
    encrypted blobs verified by CRC alone) where n has room; equal digests at 63/64, 255/256 and at
    0 and n - 1."""
    rng = np.random.default_rng([seed, m, n])
    listing = [fill(oracle, 100000 + j)[0] for j in range(m)]
    remote, entries, k = {}, [], 0

    def new_chunk():
        nonlocal k
        dg, blob, size = fill(oracle, 1000 * seed + k)
        k += 1
        remote[dg] = blob
        return dg, size

    for i in range(n):
        r = i % 4
        if r == 1 and m:
            j = int(rng.integers(0, m))
            entries.append((listing[j], fill(oracle, 100000 + j)[2]))
        elif r == 2 and entries:
            entries.append(entries[int(rng.integers(0, len(entries)))])
        elif i % 16 == 7:
            entries.append((rng.bytes(32), 10))  # the source lacks it
        else:
            entries.append(new_chunk())
    sp = v.specials(oracle)
    if n >= 70 + len(sp):
        for t, (_, dg, blob, size, _, _) in enumerate(sp):
            entries[66 + t] = (dg, size)
            remote[dg] = blob
    for a, b in ((63, 64), (255, 256)):
        if n > b:
            entries[b] = entries[a]
    if n >= 2:
        entries[n - 1] = entries[0]
        if n in (65, 257):  # (one digest at 0 and on both sides of the block's edge)
            entries[n - 2] = entries[0]
    return Case(f"planted/m{m}/n{n}/seed{seed}", listing, 0, remote, [_entries_index(f"m{m}-n{n}.didx", entries)])


def repeated(oracle, present: bool) -> Case:
    """One digest a thousand times: one claiming entry, the lowest."""
    dg, blob, size = fill(oracle, 200)
    listing = [fill(oracle, 300 + j)[0] for j in range(5)] + ([dg] if present else [])
    return Case(f"repeat1000/{'present' if present else 'absent'}", listing, 0, {dg: blob},
                [_entries_index("r.didx", [(dg, size)] * 1000)])


CHAIN_L = 10


def chain(oracle) -> Case:
    """300 distinct digests with the same first 8 bytes -- one probe chain -- whose home slot is
    capacity - 3 of the 2^10 table that 150 listed + 300 reserved entries get, so the chain wraps
    round the table's end.  Every second one is listed, the others are new (the source has every
    fourth of those: the rest are load failures), interleaved in the index."""
    rng = np.random.default_rng(0x636861)
    while True:
        pre = rng.bytes(8)
        if gcplanted.home_slot(pre + bytes(24), CHAIN_L) == (1 << CHAIN_L) - 3:
            break
    digs = [pre + rng.bytes(24) for _ in range(300)]
    listing = [digs[t] for t in range(0, 300, 2)]
    rng.shuffle(listing)
    remote = {}
    for t in range(1, 300, 4):
        chunk = rng.bytes(20)
        remote[digs[t]] = d.make_blob(oracle, 2, chunk, v.g.KEY1, v.g._iv(t))  # (encrypted: any digest verifies)
    assert begin_log2(len(listing), 300) == CHAIN_L
    return Case("chain300", listing, 300, remote, [_entries_index("chain.didx", [(dg, 20) for dg in digs])])


def triple(oracle) -> Case:
    """A listing with one digest at three positions: the lowest is the chunk."""
    a, b = fill(oracle, 400), fill(oracle, 401)
    listing = [fill(oracle, 410 + j)[0] for j in range(12)]
    for j in (3, 7, 11):
        listing[j] = a[0]
    listing[9] = listing[1]
    return Case("triple", listing, 0, {b[0]: b[1]},
                [_entries_index("t.didx", [(b[0], b[2]), (a[0], a[2]), (listing[1], 5), (a[0], a[2]), (listing[0], 5)])])


def growth(oracle) -> Case:
    """reserve 0, 40 listed chunks, an index of 100 new ones (the table grows), then one mixing
    listed, new and the first index's; a new group; the second index again."""
    listing = [fill(oracle, 500 + j)[0] for j in range(40)]
    remote = {}
    first = []
    for k in range(100):
        dg, blob, size = fill(oracle, 600 + k)
        if k % 9 != 4:
            remote[dg] = blob  # (the others cannot be fetched: they stay absent)
        first.append((dg, size))
    second = []
    for k in range(120):
        if k % 3 == 0:
            second.append((listing[k % 40], fill(oracle, 500 + k % 40)[2]))
        elif k % 3 == 1:
            second.append(first[(7 * k) % 100])
        else:
            dg, blob, size = fill(oracle, 800 + k)
            remote[dg] = blob
            second.append((dg, size))
    return Case("growth", listing, 0, remote,
                [_entries_index("a.didx", first), _entries_index("b.didx", second), None, _entries_index("c.didx", second)])


def two_groups(oracle) -> Case:
    """A fetched chunk whose blob is corrupt stays absent: DUP within its group, FETCH again at the
    same position after new_group (nothing appended); a good chunk is EXISTS after new_group.  The
    last two indexes have a lying manifest: nothing is claimed."""
    good, bad, other = fill(oracle, 900), fill(oracle, 901), fill(oracle, 902)
    listing = [fill(oracle, 910 + j)[0] for j in range(3)]
    remote = {good[0]: good[1], bad[0]: d._flip(bad[1], d.HDR + 2, 1), other[0]: other[1]}
    e = [(good[0], good[2]), (bad[0], bad[2]), (listing[0], 4), (bad[0], bad[2])]
    return Case("two-groups", listing, 0, remote,
                [_entries_index("g1a.didx", e), _entries_index("g1b.didx", e + [(other[0], other[2])]), None,
                 _entries_index("g2a.didx", e), _entries_index("g2-size.didx", e, ("size+1", None)),
                 _entries_index("g2-csum.didx", e, (None, "csum^1"))])


_cases = {}


def cases(oracle) -> list:
    """Every planted case, built once per process."""
    if "all" not in _cases:
        out = [planted(oracle, 33, n, seed=1) for n in N_SET]
        out += [planted(oracle, m, n, seed=2) for m in M_SET for n in (1, 65)]
        out += [repeated(oracle, False), repeated(oracle, True), chain(oracle), triple(oracle), growth(oracle),
                two_groups(oracle)]
        _cases["all"] = out
    return _cases["all"]


def case(oracle, label: str) -> Case:
    return next(c for c in cases(oracle) if c.label == label)


_expected = {}


def expected(oracle, c: Case) -> list:
    """The model's outcome of every step of a case (None for a new group), with the listing, the
    present bytes and the table's L after it: computed once."""
    if c.label not in _expected:
        mdl = Model(oracle, c.listing, c.reserve)
        outs = []
        for ix in c.steps:
            if ix is None:
                mdl.new_group()
                outs.append(None)
                continue
            image, honest = v.index_image(oracle, ix)
            o = mdl.pull_index(ix._replace(info=v.resolve_info(ix, honest)), c.remote, honest)
            o["image"], o["honest"] = image, honest
            o["digests"], o["present"] = mdl.listing()
            o["table_log2"], o["count"] = mdl.L, len(mdl.order)
            outs.append(o)
        _expected[c.label] = outs
    return _expected[c.label]


# ---- driving a worker -----------------------------------------------------------------------------

def listing(c: Case):
    """(paths None, digests (m, 32)) as SyncWorker takes it."""
    return None, v.digest_rows(c.listing) if c.listing else np.zeros((0, 32), np.uint8)


def remote_stream(c: Case):
    """The source store resident: (digests (M, 32), bytes of all blobs back to back, M + 1 offsets)
    of the blobs that can be fetched."""
    have = [(dg, b) for dg, b in c.remote.items() if b is not None]
    off = np.concatenate([[0], np.cumsum([len(b) for _, b in have])]).astype(np.uint64)
    rows = v.digest_rows([dg for dg, _ in have]) if have else np.zeros((0, 32), np.uint8)
    return rows, np.frombuffer(b"".join(b for _, b in have), dtype=np.uint8), off


def _state(worker, out):
    dg, pr = worker.listing()
    out["digests"], out["present"] = [bytes(r) for r in dg], [int(x) for x in pr]
    out["table_log2"], out["count"] = worker.table_log2, worker.count
    return out


def by_hand(worker, c: Case, ix: Index, upload, batch: int = 0, image=None, info=None):
    """plan (plan_index with `image`) / submit / finish with the blobs of the case's source:
    `upload(bytes array)` returns what submit takes (a device address or the array) and something
    to keep alive.  `batch`: items per submit (0: all in one).  Returns a dict like the model's."""
    if image is not None:
        chk, vd, fs, fe, ts = worker.plan_index(image, info)
    else:
        chk = 0
        vd, fs, fe, ts = worker.plan(v.digest_rows(ix.digests) if ix.digests else np.zeros((0, 32), np.uint8), ix.sizes)
    out = dict(index_check=chk, verdict=[int(x) for x in vd], fetch_store=[int(x) for x in fs],
               fetch_entry=[int(x) for x in fe], touch_store=[int(x) for x in ts], kinds=[], status=[], result=None)
    if chk:
        return _state(worker, out)
    step = batch or max(1, fe.size)
    for t0 in range(0, fe.size, step):
        blobs = [c.remote.get(ix.digests[int(i)]) for i in fe[t0:t0 + step]]
        failed = [1 if b is None else 0 for b in blobs]
        raw = b"".join(b or b"" for b in blobs)
        off = np.concatenate([[0], np.cumsum([len(b or b"") for b in blobs])]).astype(np.uint64)
        ptr, keep = upload(np.frombuffer(raw, dtype=np.uint8))
        k, s = worker.submit(ptr, off, failed)
        del keep
        out["kinds"] += [int(x) for x in k]
        out["status"] += [int(x) for x in s]
    out["result"] = worker.finish()
    return _state(worker, out)


def through_pull_index(worker, c: Case, image, info, remote, budget: int = 0):
    chk, res, o = worker.pull_index(image, info, remote, budget)
    out = {k: [int(x) for x in o[k]] for k in ("verdict", "fetch_store", "fetch_entry", "touch_store", "kinds", "status")}
    out["index_check"], out["result"] = chk, res
    return _state(worker, out)


LISTS = ("verdict", "fetch_store", "fetch_entry", "touch_store", "kinds", "status", "digests", "present")


def outcome_diff(got: dict, want: dict) -> list:
    """What differs between an outcome of by_hand / through_pull_index and the model's (or the mirror's)."""
    bad = []
    if got["index_check"] != want["index_check"]:
        bad.append(("index_check", got["index_check"], want["index_check"]))
    if (got["result"] is None) != (want["result"] is None):
        bad.append(("result", got["result"], want["result"]))
    elif got["result"] is not None:
        bad += [(k, got["result"][k], want["result"][k]) for k in RESULT_KEYS if int(got["result"][k]) != int(want["result"][k])]
    for k in LISTS:
        a, b = list(got[k]), list(want[k])
        if a != b:
            i = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            bad.append((k, f"differs at {i}: {a[i:i + 3]} / {b[i:i + 3]} (lengths {len(a)}, {len(b)})"))
    for k in ("table_log2", "count"):
        if got[k] != want[k]:
            bad.append((k, got[k], want[k]))
    return bad


def run_case(make_worker, c: Case, want: list, upload, how: str = "hand", batch: int = 0, budget: int = 0, remote=None):
    """Every step of a case on a fresh worker: [(step name,) + difference].  `how`: "hand" (plan),
    "image" (plan_index) or "pull" (pull_index over the resident `remote`)."""
    bad = []
    with make_worker(listing(c), c.reserve) as w:
        for ix, e in zip(c.steps, want):
            if ix is None:
                w.new_group()
                continue
            info = v.resolve_info(ix, e["honest"])
            if how == "pull":
                got = through_pull_index(w, c, e["image"], info, remote, budget)
            elif how == "image" or e["index_check"]:
                got = by_hand(w, c, ix, upload, batch, image=e["image"], info=info)
            else:
                got = by_hand(w, c, ix, upload, batch)
            bad += [(c.label, ix.name) + x for x in outcome_diff(got, e)]
    return bad


# ---- a real datastore ----------------------------------------------------------------------------

def build_remote(oracle, pbschunk, base):
    """A source datastore under `base` with one snapshot: a .didx archive of 30 chunks (kinds 0 and
    1, repeats; one chunk file damaged behind a recomputed CRC, one absent), a .fidx archive of
    four chunks that comes before it in the manifest, a .blob file and the manifest.  Returns
    (snapshot_dir, dict(files, didx digests, bad digest, absent digest))."""
    snap = os.path.join(base, "vm", "100", "2024-01-01T00:00:00Z")
    os.makedirs(snap)

    def put(dig, blob):
        h = dig.hex()
        os.makedirs(os.path.join(base, ".chunks", h[:4]), exist_ok=True)
        with open(os.path.join(base, ".chunks", h[:4], h), "wb") as f:
            f.write(blob)

    digs, sizes = [], []
    for k in range(30):
        c = v._good(oracle, k % 2, 4200 + 37 * k if k % 2 else 1 + 50 * k, 7000 + k)
        digs.append(c[0])
        sizes.append(c[2])
        if k == 6:
            put(c[0], d._with_crc(d._flip(c[1], d.HDR + 3, 4)))
        elif k != 11:
            put(c[0], c[1])
    digs += digs[:5]
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
        put(fdigs[-1], d.make_blob(oracle, i % 2, chunk, v.g.KEY1, v.g._iv(1)))
    fimg, fcsum = pbschunk.fidx_build(np.frombuffer(b"".join(fdigs), np.uint8).reshape(-1, 32), fsize, cs)
    with open(os.path.join(snap, "drive-scsi0.img.fidx"), "wb") as f:
        f.write(bytes(fimg))
    conf = oracle.blob_uncompressed(b"memory: 2048\n")
    with open(os.path.join(snap, "qemu-server.conf.blob"), "wb") as f:
        f.write(conf)
    files = [
        {"filename": "qemu-server.conf.blob", "size": len(conf), "csum": hashlib.sha256(conf).hexdigest(), "crypt-mode": "none"},
        {"filename": "drive-scsi0.img.fidx", "size": fsize, "csum": bytes(fcsum).hex(), "crypt-mode": "none"},
        {"filename": "root.pxar.didx", "size": int(ends[-1]), "csum": dcsum.hex(), "crypt-mode": "none"},
    ]
    manifest = {"backup-type": "vm", "backup-id": "100", "backup-time": 1704067200, "files": files, "unprotected": {}}
    with open(os.path.join(snap, "index.json.blob"), "wb") as f:
        f.write(oracle.blob_uncompressed(json.dumps(manifest).encode()))
    return snap, dict(files=files, didx=digs, sizes=sizes, fidx=fdigs, bad=digs[6], absent=digs[11])


def _store_files(base):
    out = {}
    root = os.path.join(base, ".chunks")
    for sub in sorted(os.listdir(root)) if os.path.isdir(root) else []:
        for name in sorted(os.listdir(os.path.join(root, sub))):
            with open(os.path.join(root, sub, name), "rb") as f:
                out[name] = f.read()
    return out


def check_pull_snapshot(p, oracle, tmp_path, device):
    """pull_snapshot between two directories against the model, on the mirror or on the device."""
    rbase, lbase = str(tmp_path / "remote"), str(tmp_path / "local")
    rsnap, what = build_remote(oracle, p, rbase)
    lsnap = os.path.join(lbase, "vm", "100", "2024-01-01T00:00:00Z")
    # the local store already has two of the source's chunks, one with an old atime
    have = [what["didx"][0], what["fidx"][1]]
    remote = {}
    for name, data in _store_files(rbase).items():
        remote[bytes.fromhex(name)] = data
    for dg in have:
        path = p.chunk_path(lbase, dg)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "wb") as f:
            f.write(remote[dg])
        os.utime(path, (1000, 1000))
    mdl = Model(oracle, sorted(have))
    fsizes = [4096, 4096, 4096, 100]
    want_f = mdl.pull_index(Index("f", what["fidx"], fsizes, 0, None), remote)
    want_d = mdl.pull_index(Index("d", what["didx"], what["sizes"], 0, None), remote)
    with p.SyncWorker(p.list_chunk_store(lbase), device=device) as w:
        verdict, files = p.pull_snapshot(rbase, rsnap, lbase, lsnap, w, batch_bytes=20000)
        # the .didx names a damaged and an absent chunk: the walk fails there, after the other two files
        assert verdict == "failed" and [f[0] for f in files] == [x["filename"] for x in what["files"]]
        assert files[0][1:] == (None, None) and files[1][1] is None and "fetch item" in files[2][1]
        for got, want in ((files[1][2], want_f["result"]), (files[2][2], want_d["result"])):
            assert [(k, got[k], want[k]) for k in RESULT_KEYS if got[k] != want[k]] == []
        assert files[2][2]["first_failed"] == 5 and files[2][2]["failed"] == 1 and files[2][2]["load_failed"] == 1
        # the local store holds exactly the model's inserted set beside what it had, byte for byte
        inserted = set(want_f["inserted"]) | set(want_d["inserted"])
        local = _store_files(lbase)
        assert set(local) == {dg.hex() for dg in inserted | set(have)}
        assert all(local[name] == remote[bytes.fromhex(name)] for name in local)
        assert what["bad"] not in inserted and what["absent"] not in inserted
        # cond_touch_chunk: the chunks it had got a new atime
        assert all(os.stat(p.chunk_path(lbase, dg)).st_atime > 1000 for dg in have)
        # the files that passed are in place and byte-equal; the failed index stays a .tmp; no manifest yet
        for name in ("qemu-server.conf.blob", "drive-scsi0.img.fidx"):
            with open(os.path.join(lsnap, name), "rb") as a, open(os.path.join(rsnap, name), "rb") as b:
                assert a.read() == b.read()
        assert sorted(os.listdir(lsnap)) == ["drive-scsi0.img.fidx", "index.json.tmp", "qemu-server.conf.blob", "root.pxar.tmp"]
        # the source is repaired; a new group pulls the snapshot again: the two files that passed are
        # skipped, and of the .didx only the two chunks that stayed absent are fetched, at their old positions
        good = v._good(oracle, 0, 1 + 50 * 6, 7006)
        for dg, blob in ((what["bad"], good[1]), (what["absent"], v._good(oracle, 1, 4200 + 37 * 11, 7011)[1])):
            path = p.chunk_path(rbase, dg)
            os.makedirs(os.path.dirname(path), exist_ok=True)
            with open(path, "wb") as f:
                f.write(blob)
        w.new_group()
        verdict, files = p.pull_snapshot(rbase, rsnap, lbase, lsnap, w)
        assert verdict == "ok" and [f[1] for f in files] == [None] * 3 and files[0][2] is None and files[1][2] is None
        res = files[2][2]
        assert (res["fetch"], res["inserted"], res["appended"], res["exists"], res["dup"]) == (2, 2, 0, 28, 5)
        assert sorted(os.listdir(lsnap)) == sorted(os.listdir(rsnap))
        for name in os.listdir(rsnap):
            with open(os.path.join(lsnap, name), "rb") as a, open(os.path.join(rsnap, name), "rb") as b:
                assert a.read() == b.read()
        assert set(_store_files(lbase)) == set(_store_files(rbase))
        assert p.pull_snapshot(rbase, rsnap, lbase, lsnap, w) == ("ok", [])  # "no data changes"
        # a manifest that lies about a blob: the walk stops there
        lies = [dict(f) for f in what["files"]]
        lies[0]["size"] += 1
        with open(os.path.join(rsnap, "index.json.blob"), "wb") as f:
            f.write(oracle.blob_uncompressed(json.dumps({"files": lies}).encode()))
        verdict, files = p.pull_snapshot(rbase, rsnap, lbase, lsnap, w)
        assert verdict == "failed" and len(files) == 1 and "wrong size" in files[0][1]
