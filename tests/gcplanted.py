"""Planted inputs for garbage collection (include/pbs_gc.h) and a Python model of the reference.

The model is a transliteration of `index_mark_used_chunks` (pbs-datastore/src/datastore.rs:952-986),
`get_chunk_iterator` (pbs-datastore/src/chunk_store.rs:247-343) and `sweep_unused_chunks`
(:350-440) over a simulated store: a dict of path -> [size, atime, is_file].  Phase 1 really sets
atimes to `now` and touches the ".N.bad" paths only of absent chunks; phase 2 really lists,
filters names and classifies.  The host mirror and the front end are checked against it.
"""
import os
import stat

import numpy as np

HASH_MUL = 0x9E3779B97F4A7C15
VANISHED = (1 << 64) - 1
BAD, FOREIGN = 1, 2
KEEP, PENDING, REMOVE = 0, 1, 2
STATUS_KEYS = ("index-file-count", "index-data-bytes", "disk-bytes", "disk-chunks", "removed-bytes",
               "removed-chunks", "pending-bytes", "pending-chunks", "removed-bad", "still-bad")
HEXDIGITS = set("0123456789abcdefABCDEF")


def table_log2(m: int) -> int:
    """The smallest L with 2^L >= max(2 m, 64) (pbs_gc_begin)."""
    L = 6
    while (1 << L) < 2 * m:
        L += 1
    return L


def home_slot(digest: bytes, L: int) -> int:
    """pbs_gc_home_slot as the header documents it."""
    return ((int.from_bytes(digest[:8], "big") * HASH_MUL) & ((1 << 64) - 1)) >> (64 - L)


# ---- the model ------------------------------------------------------------------------------------

def chunk_path(digest: bytes) -> str:
    """ChunkStore::chunk_path (chunk_store.rs:557-570): .chunks/<first four hex>/<hex>."""
    h = digest.hex()
    return f".chunks/{h[:4]}/{h}"


def model_list(files):
    """get_chunk_iterator: (path, bad) of every listed name, subdirectory by subdirectory."""
    out = []
    for path in sorted(files):
        parts = path.split("/")
        if len(parts) != 3 or parts[0] != ".chunks":
            continue
        sub, name = parts[1], parts[2]
        if len(sub) != 4 or any(c not in "0123456789abcdef" for c in sub):  # format!("{:04x}", at)
            continue
        b = name.encode()
        if len(b) != 64 and len(b) != 64 + len(".0.bad"):
            continue
        if not all(c in HEXDIGITS for c in name[:64]):
            continue
        out.append((path, name.endswith(".bad")))
    return out


def model_gc(files, indexes, phase1_start, oldest_writer, now):
    """garbage_collection over a copy of `files`.  `indexes`: [(name, [digest, ...], index_bytes)].
    Returns dict(status, warnings [(name, position)], touched {path}, removed {path}, pending
    {path}); `touched`: the paths whose atime phase 1 set."""
    files = {p: list(v) for p, v in files.items()}
    status = dict.fromkeys(STATUS_KEYS, 0)
    warnings, touched = [], set()

    def cond_touch_path(path):  # chunk_store.rs:220-245 with assert_exists == false
        if path not in files:
            return False
        files[path][1] = now
        touched.add(path)
        return True

    for name, digests, index_bytes in indexes:  # index_mark_used_chunks
        status["index-file-count"] += 1
        status["index-data-bytes"] += index_bytes
        for pos, d in enumerate(digests):
            if not cond_touch_path(chunk_path(d)):
                warnings.append((name, pos))
                for i in range(10):
                    cond_touch_path(chunk_path(d) + f".{i}.bad")

    min_atime = phase1_start - 3600 * 24  # sweep_unused_chunks
    if oldest_writer < min_atime:
        min_atime = oldest_writer
    min_atime -= 300
    removed, pending = set(), set()
    for path, bad in model_list(files):
        size, atime, is_file = files[path]
        if size is None or not is_file:  # (size None: the stat fails)
            continue
        if atime < min_atime:
            removed.add(path)
            status["removed-bad" if bad else "removed-chunks"] += 1
            status["removed-bytes"] += size
        elif atime < oldest_writer:
            pending.add(path)
            status["still-bad" if bad else "pending-chunks"] += 1
            status["pending-bytes"] += size
        else:
            if not bad:
                status["disk-chunks"] += 1
            status["disk-bytes"] += size
    return {"status": status, "warnings": warnings, "touched": touched, "removed": removed, "pending": pending}


def sim_listing(files):
    """What list_chunk_store returns for a real directory, for the simulated one: (paths, digests
    (m, 32), flags).  FOREIGN: any listed name that chunk_path never builds."""
    paths, digs, flags = [], [], []
    for path, bad in model_list(files):
        sub, name = path.split("/")[1:]
        f = BAD if bad else 0
        lower = all(c in "0123456789abcdef" for c in name[:64])
        own = lower and name[:4] == sub and (len(name) == 64 or (name[64] == "." and name[65].isdigit()
                                                                  and name[66:] == ".bad"))
        if not own:
            f |= FOREIGN
        paths.append(path)
        digs.append(bytes.fromhex(name[:64]))
        flags.append(f)
    d = np.frombuffer(b"".join(digs), dtype=np.uint8).reshape(-1, 32).copy()
    return paths, d, np.asarray(flags, dtype=np.uint8)


def sim_sizes_atimes(files, paths):
    sizes = np.full(len(paths), VANISHED, dtype=np.uint64)
    atimes = np.zeros(len(paths), dtype=np.int64)
    for j, p in enumerate(paths):
        size, atime, is_file = files[p]
        if size is not None and is_file:
            sizes[j], atimes[j] = size, atime
    return sizes, atimes


# ---- planted stores -------------------------------------------------------------------------------

def _wrap_digests(rng, L, want):
    """Digests whose home slot is one of the last four of a 2^L table: their cluster wraps to 0."""
    out = []
    while len(out) < want:
        pre = rng.integers(0, 1 << 63, size=1 << 18, dtype=np.uint64) * np.uint64(2) + rng.integers(
            0, 2, size=1 << 18, dtype=np.uint64)
        slot = (pre * np.uint64(HASH_MUL)) >> np.uint64(64 - L)
        for p in pre[slot >= np.uint64((1 << L) - 4)][: want - len(out)]:
            d = int(p).to_bytes(8, "big") + rng.bytes(24)
            assert home_slot(d, L) >= (1 << L) - 4
            out.append(d)
    return out


def planted(m: int, seed: int = 1):
    """A store of exactly m listed files and the digests an index over it names.
    Returns (files, index): files path -> [size, atime, is_file] (sizes and atimes still zero),
    index a list of 32-byte digests.  As many of the planted groups as fit into m:
      triple    one digest as chunk + .0.bad + .9.bad, referenced: its .bad files stay untouched
      tenbad    one digest with ten .bad files and no chunk, referenced: all ten are touched
      lonebad   an unreferenced .bad file
      foreign   an upper-case name and a "<hex>x0.bad" name, both referenced, never touched, never
                the chunk; a referenced .bad next to the upper-case name IS touched
      wrap      eight digests with home slots among the table's last four
      cluster   300 digests with the same first 8 bytes, every second one referenced
    The index also names absent digests: random ones, and ones equal to a present digest except in
    byte 8 or in byte 31."""
    rng = np.random.default_rng(seed)
    L = table_log2(m)
    files, index = {}, []

    def rnd():
        return b"\xab" + rng.bytes(31)  # (a letter in the name: its upper case is another name)

    def add(d, suffix="", name=None):
        h = d.hex()
        files[f".chunks/{h[:4]}/{(name or h) + suffix}"] = [0, 0, True]

    groups = []
    t, tb, lb, f1, f2 = rnd(), rnd(), rnd(), rnd(), rnd()
    groups.append((3, lambda: ([add(t), add(t, ".0.bad"), add(t, ".9.bad")], index.append(t))))
    groups.append((10, lambda: ([add(tb, f".{i}.bad") for i in range(10)], index.append(tb))))
    groups.append((1, lambda: add(lb, ".3.bad")))
    groups.append((3, lambda: ([add(f1, name=f1.hex().upper()), add(f1, ".1.bad"), add(f2, "x0.bad")],
                               index.extend([f1, f2]))))

    def wrap():
        for d in _wrap_digests(rng, L, 8):
            add(d)
            index.append(d)
    groups.append((8, wrap))

    def cluster():
        pre = b"\xab" + rng.bytes(7)
        for k in range(300):
            d = pre + rng.bytes(24)
            add(d)
            if k % 2 == 0:
                index.append(d)
    groups.append((300, cluster))
    for need, make in groups:
        if len(files) + need <= m:
            make()
    present = []
    while len(files) < m:
        d = rnd()
        if rng.integers(0, 50) == 0:
            add(d, f".{int(rng.integers(0, 10))}.bad")
        else:
            add(d)
            present.append(d)
    assert len(files) == m
    for k, d in enumerate(present):
        if k % 2 == 0:
            index.append(d)
        if k % 64 == 1:  # absent, equal to a present digest except in one byte
            index.append(d[:8] + bytes([d[8] ^ 1]) + d[9:])
        if k % 64 == 2:
            index.append(d[:31] + bytes([d[31] ^ 0x80]))
        if k % 16 == 3:
            index.append(rnd())
    index += [rnd(), rnd()]
    if files:  # (the smallest stores too have a named file)
        index.append(bytes.fromhex(sorted(files)[0].split("/")[2][:64]))
    order = rng.permutation(len(index))
    return files, [index[k] for k in order]


def plant_times(files, index, phase1_start, oldest_writer, seed: int = 2):
    """Sizes and atimes for every file of `files`, in place.  A file whose digest the index names
    gets an ancient atime (a touched one must stay all the same); the others cycle, bad and
    non-bad files separately, through atimes exactly at min_atime - 1, min_atime, oldest_writer - 1
    and oldest_writer, sizes 0 and 2^40, a failing stat and a non-regular file."""
    named = {d.hex() for d in index}
    min_atime = min(phase1_start - 86400, oldest_writer) - 300
    cyc = [min_atime - 1, min_atime, oldest_writer - 1, oldest_writer]
    count = {False: 0, True: 0}
    for path in sorted(files):
        name = path.split("/")[2]
        bad = name.endswith(".bad")
        if name[:64].lower() in named:
            files[path] = [1 << 40, 1000, True]
            continue
        k = count[bad]
        count[bad] += 1
        if k % 11 == 9:
            files[path] = [None, 0, True]  # the stat fails
        elif k % 11 == 10:
            files[path] = [4096, cyc[0], False]  # a directory of that name
        else:
            files[path] = [0 if k % 3 == 0 else 1 << 40, cyc[k % 4], True]
    return files


def digest_rows(digests):
    return np.frombuffer(b"".join(digests), dtype=np.uint8).reshape(-1, 32).copy()


def index_images(p, index):
    """The planted index as a .didx (first half) and a .fidx (second half) image."""
    half = len(index) // 2
    a, b = index[:half], index[half:]
    didx, _ = p.didx_build(np.arange(1, len(a) + 1, dtype=np.uint64) * 1000, a)
    fidx, _ = p.fidx_build(b, 4096 * len(b) - 5, 4096)
    return (didx, a, 1000 * len(a)), (fidx, b, 4096 * len(b) - 5)


# ---- a real chunk store ---------------------------------------------------------------------------

MTIME = 1_500_000_000


def real_store(base, files):
    """Writes the simulated files under `base`: a failing stat becomes a dangling symlink (lstat
    sees no regular file), a non-regular file a directory; sizes are cut to a few KiB and written
    back into `files`."""
    for path, (size, atime, is_file) in sorted(files.items()):
        full = os.path.join(base, path)
        os.makedirs(os.path.dirname(full), exist_ok=True)
        if size is None:
            os.symlink("nowhere", full)
        elif not is_file:
            os.mkdir(full)
        else:
            size = min(size, 3000 + len(path) % 7)
            with open(full, "wb") as f:
                f.write(b"x" * size)
            os.utime(full, (atime, MTIME))
            files[path][0] = size


def run_real_store(p, tmp_path, device):
    files, index = planted(40, seed=21)
    # names the iterator must skip, and a file in a subdirectory it never opens
    files[".chunks/abcd/" + "ab" * 32 + ".tmp"] = [10, 5, True]
    files[".chunks/abcd/" + "zz" * 32] = [10, 5, True]
    files[".chunks/ABCD/" + "ab" * 32] = [10, 5, True]
    phase1_start, oldest_writer = 1_700_000_000, 1_700_000_000 - 200_000
    plant_times(files, index, phase1_start, oldest_writer)
    base = str(tmp_path)
    real_store(base, files)
    (didx, a, abytes), (fidx, b, bbytes) = index_images(p, index)
    for name, img in (("a.didx", didx), ("b.fidx", fidx), ("c.blob", b"junk")):
        with open(os.path.join(base, name), "wb") as f:
            f.write(img)
    ipaths = [os.path.join(base, n) for n in ("a.didx", "gone.didx", "b.fidx", "c.blob")]
    model = model_gc(files, [("a.didx", a, abytes), ("b.fidx", b, bbytes)], phase1_start, oldest_writer, now=phase1_start)
    assert model["removed"] and model["pending"] and model["touched"]

    def snapshot():
        out = {}
        for path in files:
            try:
                st = os.lstat(os.path.join(base, path))
            except FileNotFoundError:
                continue
            out[path] = (st.st_atime_ns // 10**9, st.st_mtime_ns // 10**9, stat.S_ISREG(st.st_mode))
        return out

    before = snapshot()
    # a dry run: the same status, nothing changes
    status, warnings = p.garbage_collection(base, ipaths, phase1_start, oldest_writer, device=device, apply=False)
    assert status == model["status"]
    assert snapshot() == before
    t0 = os.stat(base).st_mtime_ns // 10**9  # (any "now" of this run is later than the planted times)
    status, warnings = p.garbage_collection(base, ipaths, phase1_start, oldest_writer, device=device, apply=True)
    assert status == model["status"]
    want = [(os.path.join(base, n), (a if n == "a.didx" else b)[pos].hex()) for n, pos in model["warnings"]]
    assert warnings == want
    after = snapshot()
    assert set(after) == set(files) - model["removed"]
    for path, (atime, mtime, reg) in after.items():
        if path in model["touched"]:
            assert atime >= t0 - 1 > before[path][0], path
        else:
            assert atime == before[path][0], path
        if reg:
            assert mtime == before[path][1], path
