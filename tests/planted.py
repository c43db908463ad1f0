"""Inputs whose cut candidates sit at chosen positions (helpers of test_planted_cpu.py and
test_gpu_planted.py; not a conftest).

A position p is a candidate iff the hash H of bytes [p-63, p] passes (H & mask) >= mask-2,
so a 64-byte window that passes can be copied to any p.  A background whose period divides
32 (zeros, one constant byte, 32 bytes repeated) has H == 0 everywhere -- every table entry
is XOR-ed in twice at the same rotation -- and so holds no candidate of its own; a random
background is defused by flipping one byte inside every natural candidate's window.  The
planted positions are then the complete candidate set, which check() proves with the CPU
oracle before an input reaches a GPU.

The geometry helpers restate where the kernels' lanes, tiles, passes and tail items begin
(scan_fused.h tile_off / tile_nit, scan_main.h, scan_server.h), from the library's own plan
hooks, so candidates can be put on those boundaries.
"""
import numpy as np

KiB, MiB, GiB = 1024, 1024 * 1024, 1024 * 1024 * 1024
WINDOW = 64
BLOCK = 128          # kBlockBytes: exact-evaluation granule
TAIL_BLOCKS = 64     # kTailBlocks: blocks per tail item of the fused pass
SRV_LANE = 32        # scan server: bytes per lane
SRV_PASS = 8192      # scan server: bytes per pass (256 lanes)
EDGE_OFFSETS = (-1, 0, 1, 31, 62, 63, 64)

_windows = {}


def params(avg: int):
    """(mask, min_eff, max_eff) of an average (chunker.rs:75-106; first test at size 65)."""
    return 2 * avg - 1, max(avg // 4, 65), max(avg * 4, 65)


def _isolated(oracle, avg: int, w: np.ndarray) -> bool:
    """The window alone in a zero and in a constant background is exactly one candidate:
    none of the 63 windows on either side that overlap it passes."""
    for fill in (0, 0xA5):
        buf = np.full(4 * WINDOW, fill, np.uint8)
        buf[WINDOW:2 * WINDOW] = w
        if oracle.candidates(avg, buf).tolist() != [2 * WINDOW - 1]:
            return False
    return True


def passing_windows(oracle, avg: int) -> dict:
    """{r: uint8[64]} for r in 0, 1, 2 with (H & mask) == mask - 2 + r, taken from the
    candidates of seeded gen_random buffers (each window isolated, see _isolated)."""
    if avg in _windows:
        return _windows[avg]
    mask = 2 * avg - 1
    size = min(64 * MiB, max(avg * 512, 1 * MiB))
    found = {}
    for seed in range(1, 41):
        buf = oracle.gen_random(size, 0x9A55 + seed)
        for p in oracle.candidates(avg, buf)[:4096].tolist():
            r = (oracle.window_hash(buf, p) & mask) - (mask - 2)
            assert 0 <= r <= 2, (avg, p, r)
            if r not in found:
                w = buf[p - 63:p + 1].copy()
                if _isolated(oracle, avg, w):
                    found[r] = w
        if len(found) == 3:
            _windows[avg] = found
            return found
    raise AssertionError(f"no passing windows for all three residues at average {avg}: {sorted(found)}")


def background(kind: str, n: int, seed: int = 1, oracle=None, avg: int = 0) -> np.ndarray:
    """n background bytes without a candidate: "zeros", "const" (0xA5), "p32" (32 seeded
    bytes repeated), "random_defused" (seeded random bytes, one byte flipped inside every
    natural candidate's window until the oracle finds none at `avg`)."""
    if kind == "zeros":
        return np.zeros(n, np.uint8)
    if kind == "const":
        return np.full(n, 0xA5, np.uint8)
    if kind == "p32":
        pat = np.random.default_rng(seed).integers(0, 256, 32, dtype=np.uint8)
        return np.tile(pat, n // 32 + 1)[:n].copy()
    if kind == "random_defused":
        bg = oracle.gen_random(n, seed)
        for rnd in range(20):
            cand = oracle.candidates(avg, bg)
            if cand.size == 0:
                return bg
            bg[cand.astype(np.int64) - 31 + (rnd % 7)] ^= 0x5A
        raise AssertionError(f"random background still holds {cand.size} candidates after 20 rounds")
    raise ValueError(kind)


def plant(bg: np.ndarray, positions, windows: dict, first: int = 0) -> np.ndarray:
    """Window windows[i % 3] copied to bytes [p-63, p] for the i-th position (in place;
    `first`: the index of positions[0] when an input is planted in several steps)."""
    n, prev = bg.size, None
    for i, p in enumerate(positions, first):
        p = int(p)
        assert 63 <= p < n, (p, n)
        assert prev is None or p - prev >= WINDOW, (prev, p)
        bg[p - 63:p + 1] = windows[i % 3]
        prev = p
    return bg


def check(oracle, avg: int, data: np.ndarray, positions) -> np.ndarray:
    """The oracle's candidates of `data` are exactly `positions`, its resolve of them is its
    streaming chunker's cut list; returns that list with the EOF tail appended."""
    pos = np.asarray(sorted(int(p) for p in positions), dtype=np.uint64)
    cand = oracle.candidates(avg, data)
    assert np.array_equal(cand, pos), (cand.size, pos.size, np.setxor1d(cand, pos)[:8])
    ref = oracle.chunk_feed(avg, data)
    assert np.array_equal(oracle.resolve(avg, cand, data.size), ref)
    if ref.size == 0 or int(ref[-1]) != data.size:
        ref = np.append(ref, np.uint64(data.size))
    return ref


def make_input(oracle, avg: int, kind: str, n: int, positions, seed: int = 1) -> np.ndarray:
    """background + plant, then the windows that straddle a planted window's edge made
    harmless: where one of them passes (at small averages some always do), a background byte
    of it that lies in no planted window is redrawn, until the oracle finds exactly
    `positions` (a periodic background is then no longer periodic next to that window)."""
    win = passing_windows(oracle, avg)
    pos = np.asarray(sorted(int(p) for p in positions), dtype=np.int64)
    want = pos.astype(np.uint64)
    data = plant(background(kind, n, seed, oracle, avg), pos, win)
    rng = np.random.default_rng(seed)
    for _ in range(40):
        extra = np.setdiff1d(oracle.candidates(avg, data), want).astype(np.int64)
        if extra.size == 0:
            return data
        for q in extra.tolist():
            for x in range(q, q - 64, -1):  # a byte of q's window in no planted one
                j = int(np.searchsorted(pos, x))
                if x >= 0 and (j == pos.size or pos[j] - 63 > x):
                    data[x] = (int(data[x]) + int(rng.integers(1, 256))) & 0xFF
                    break
            else:
                raise AssertionError(f"candidate {q} lies wholly inside planted windows")
    raise AssertionError(f"{kind}: {extra.size} stray candidates remain beside the planted windows")


# ---- geometry ----------------------------------------------------------------------

def fused_segments(gpu, n: int, nw: int) -> dict:
    """Static tile order of the fused pass / scan pass over nw scanner waves for a batch of
    n bytes (scan_fused.h tile_nit / tile_off): byte offsets of every lane segment ("lanes"),
    tile ("tiles"), the first normal tile after the long ones ("t_long"), the first tile of
    the short round or pool ("t_small"), the short round's tiles ("short"), the covered end,
    the tail items of 64 blocks ("tail") and the last partial block."""
    pl = gpu.plan_fused_static(n, nw)
    nt, q, tl, ts, qs, tsl = (pl[k] for k in ("ntiles", "seg_q", "t_long", "t_small", "seg_qs", "t_small_long"))

    def nit(t):
        return q + (1 if t < tl else 0) if t < ts else qs + (1 if t - ts < tsl else 0)

    def off(t):
        if t < ts:
            return (t * q + min(t, tl)) * 64 * BLOCK
        u = t - ts
        return (ts * q + tl + u * qs + min(u, tsl)) * 64 * BLOCK

    tiles = [off(t) for t in range(nt)]
    lanes = [off(t) + l * nit(t) * BLOCK for t in range(nt) for l in range(64)]
    covered = off(nt - 1) + 64 * nit(nt - 1) * BLOCK if nt else 0
    assert covered == pl["covered"], (covered, pl)
    for t in range(1, nt):
        assert tiles[t] == tiles[t - 1] + 64 * nit(t - 1) * BLOCK
    nblk = (n + BLOCK - 1) // BLOCK
    tail = list(range(covered, nblk * BLOCK, TAIL_BLOCKS * BLOCK))
    return {"plan": pl, "tiles": tiles, "lanes": lanes, "covered": covered, "tail": tail,
            "t_long": [off(tl)] if 0 < tl < ts else [],
            "t_small": [off(ts)] if ts < nt else [],
            "short": [off(t) for t in range(ts, nt)],
            "tail_blocks": list(range(covered + BLOCK, (n - 1) // BLOCK * BLOCK, BLOCK)),
            "last_block": [(n - 1) // BLOCK * BLOCK], "n": n}


def scan_main_segments(gpu, n: int, cu: int) -> dict:
    """scan_main's tiles for a batch of n bytes on cu compute units: tiles [0, t_big) of 64
    segments of seg bytes, then tiles of seg / 4; the blocks past `covered` are evaluated
    exactly, one by one."""
    pl = gpu.plan_scan_main(n, cu)
    seg, nt, tb = pl["seg"], pl["ntiles"], min(pl["t_big"], pl["ntiles"])
    tiles, lanes = [], []
    for t in range(nt):
        s = seg if t < tb else seg // 4
        o = t * 64 * seg if t < tb else tb * 64 * seg + (t - tb) * 64 * s
        tiles.append(o)
        lanes += [o + l * s for l in range(64)]
    covered = tb * 64 * seg + (nt - tb) * 16 * seg
    assert covered == pl["covered"] and covered <= n, (covered, pl, n)
    return {"plan": pl, "tiles": tiles, "lanes": lanes, "covered": covered,
            "t_big": [tb * 64 * seg] if tb < nt else [],
            "tail": list(range(covered, n, BLOCK))[:1],
            "tail_blocks": list(range(covered + BLOCK, (n - 1) // BLOCK * BLOCK, BLOCK)),
            "last_block": [(n - 1) // BLOCK * BLOCK], "n": n}


def server_segments(length: int, n_wg: int, minpass: int = 1) -> dict:
    """One scan-server request of `length` bytes (scan_server.h): 32-byte lanes, 8 KiB
    passes, workgroup g of gu takes passes [g npass / gu, (g + 1) npass / gu)."""
    npass = (length + SRV_PASS - 1) // SRV_PASS
    gu = max(1, min(npass // max(minpass, 1), n_wg))
    return {"lanes": list(range(0, length, SRV_LANE)), "passes": list(range(0, length, SRV_PASS)),
            "wgs": [g * npass // gu * SRV_PASS for g in range(gu)], "gu": gu, "npass": npass}


def place_edges(groups, min_gap: int, n: int, rot: int = 0, lo: int = 0, taken=()) -> list:
    """edge_positions over several boundary groups in priority order (the rare boundaries
    first, the lane segments last): group g's boundary i gets the offset number
    (i + g + rot) % 7 -- or one of the group's own offsets when it is a (boundaries, offsets)
    pair -- and is taken when its candidate lies in [max(lo, 63, min_gap - 1), n) and at
    least min_gap (and two windows) from every candidate taken before (`taken` included).
    Returns the new candidates, sorted."""
    import bisect
    gap = max(min_gap, 2 * WINDOW)
    have = sorted(int(p) for p in taken)
    new = []
    for g, grp in enumerate(groups):
        bounds, offs = grp if isinstance(grp, tuple) else (grp, EDGE_OFFSETS)
        for i, b in enumerate(sorted(set(int(b) for b in bounds))):
            p = b + offs[(i + g + rot) % len(offs)]
            if p < max(lo, 63, min_gap - 1) or p >= n:
                continue
            j = bisect.bisect_left(have, p)
            if (j > 0 and p - have[j - 1] < gap) or (j < len(have) and have[j] - p < gap):
                continue
            have.insert(j, p)
            new.append(p)
    return sorted(new)


def edge_positions(boundaries, min_gap: int, n: int, prev: int = -1) -> list:
    """Boundary i (sorted, unique) gets the candidate b + (-1, 0, 1, 31, 62, 63, 64)[i % 7];
    boundaries whose candidate is not at least min_gap (and two windows) after the previous
    one, or lies outside [63, n), are skipped: place_edges over one group."""
    return place_edges([list(boundaries)], min_gap, n, lo=prev + min_gap, taken=[prev] if prev >= 0 else ())


# ---- the min/max rule ----------------------------------------------------------------

def minmax_positions(oracle, avg: int, n: int, adjacent: bool = False) -> list:
    """Candidates at the edges of the min/max rule, chunk after chunk (s = the open chunk's
    start): s+min-2 (ignored) and a later cut; s+min-1 (the first position that cuts);
    s+max-1 (a cut that coincides with the forced one); s+max (the forced cut comes first,
    the candidate is then byte 0 of the new chunk); a chain min-1 apart (each acceptance
    depends on the previous one).  adjacent: also s+min-2 and s+min-1 together (lists for
    the resolver alone; planted windows must be 64 apart)."""
    _, mn, mx = params(avg)
    pos, s, skipped, k = [], 0, 0, 0
    while skipped < 6:
        step, k = k % 6, k + 1
        if step == 0:
            new = [s + mn - 2, s + 2 * mn]
        elif step == 1:
            new = [s + mn - 1]
        elif step == 2:
            new = [s + mx - 1]
        elif step == 3:
            new = [s + mx]
        elif step == 4:
            new = [s + mn - 1 + i * (mn - 1) for i in range(7)]
            new = [p for p in new if p < n - WINDOW] or new[:1]
        else:
            new = [s + mn - 2, s + mn - 1] if adjacent else []
        if not new or new[-1] >= n - WINDOW or new[0] < 63 or (pos and new[0] - pos[-1] < (1 if adjacent else WINDOW)):
            skipped += 1
            continue
        skipped = 0
        pos += new
        cuts = oracle.resolve(avg, np.asarray(pos, np.uint64), pos[-1] + 1)
        s = int(cuts[-1]) if cuts.size else 0
    return pos


def first_test_input(oracle, n: int, kind: str = "zeros"):
    """Average 256 (min_eff = 65, the first test of a chunk): for chunk start s a candidate
    at s+64 (cut, size 65), or at s+63 (size 64: ignored) and a cut 128 later.  The planted
    windows nearly touch, so every step is kept only if the oracle still finds exactly the
    planted candidates (else the other step, else a spacer cut at s+200).  (data, positions)"""
    avg = 256
    win = passing_windows(oracle, avg)
    bg = background(kind, n)
    data, pos, s, used = bg.copy(), [], 0, [0, 0]
    while s + 600 < n:
        opts = [(0, [s + 64]), (1, [s + 63, s + 63 + 128])]
        if used[1] < used[0]:
            opts.reverse()
        for which, new in opts + [(2, [s + 200])]:
            hi = new[-1] + 2 * WINDOW
            plant(data, new, win, len(pos))
            if oracle.candidates(avg, data[:hi]).tolist() == pos + new:
                break
            data[s:hi] = bg[s:hi]
        else:
            raise AssertionError(f"no clean step at chunk start {s}")
        pos += new
        if which < 2:
            used[which] += 1
        s = new[-1] + 1
    assert min(used) >= 8, used
    return data, pos


# ---- dense candidates (limits) -------------------------------------------------------

def passing_pattern(oracle, period: int, avg: int) -> np.ndarray:
    """`period` seeded random bytes whose periodic continuation passes the cut test at some
    phase: every period-th byte of a run of them is a candidate."""
    mask = 2 * avg - 1
    for seed in range(1, 1 << 20):
        pat = oracle.gen_random(period, seed)
        buf = np.tile(pat, 64 // period + 3)
        if any((oracle.window_hash(buf, 63 + k) & mask) >= mask - 2 for k in range(period)):
            return pat
    raise AssertionError("no passing pattern")


def dense_run(oracle, avg: int, data: np.ndarray, at: int, count: int, pat: np.ndarray) -> int:
    """A run of the passing pattern written at data[at:] (zeros around it), as long as it takes
    to hold exactly `count` candidates; returns its length."""
    probe = np.zeros(7000 + 256, np.uint8)
    probe[128:7128] = np.tile(pat, 7000 // pat.size + 1)[:7000]
    rate = oracle.candidates(avg, probe).size / 7000.0
    guess = int(count / rate)
    for L in range(max(64, guess - 400), guess + 400):
        buf = np.zeros(L + 256, np.uint8)
        buf[128:128 + L] = np.tile(pat, L // pat.size + 1)[:L]
        if oracle.candidates(avg, buf).size == count:
            assert not data[at - 128:at + L + 128].any()
            data[at:at + L] = buf[128:128 + L]
            return L
    raise AssertionError(f"no run length holds exactly {count} candidates")


# ---- a hash equal to the threshold ---------------------------------------------------

def _rotl(x: int, r: int) -> int:
    r &= 31
    return ((x << r) | (x >> (32 - r))) & 0xFFFFFFFF if r else x


def threshold_window(oracle, avg: int) -> np.ndarray:
    """64 bytes whose window hash is exactly mask - 2 as a 32-bit value: the lowest passing
    residue with every bit above the mask zero.  The kernels test rotl(h, rot) >= thr with
    thr = (mask - 2) << rot, and this window sits on that threshold, where >= and > part.
    Random data reaches it once in 2^32 positions; here it is solved for: the hash is the XOR
    of the rotated table words of the 64 bytes, so choosing each byte from two candidates is
    a linear system over GF(2) with 64 unknowns and 32 equations."""
    zeros = np.zeros(WINDOW, np.uint8)
    assert oracle.window_hash(zeros, 63) == 0
    word = []  # T[b] ^ T[0], read through the oracle: a window of zeros but its last byte
    for b in range(256):
        w = zeros.copy()
        w[63] = b
        word.append(oracle.window_hash(w, 63))
    target = 2 * avg - 1 - 2
    for seed in range(1, 200):
        rng = np.random.default_rng(seed)
        a, b = rng.integers(0, 256, WINDOW), rng.integers(0, 256, WINDOW)
        want, cols = target, []
        for i in range(WINDOW):
            ra, rb = _rotl(word[a[i]], 63 - i), _rotl(word[b[i]], 63 - i)
            want ^= ra
            cols.append(ra ^ rb)
        basis = {}  # leading bit -> (vector, the columns XOR-ed into it)
        for i, c in enumerate(cols):
            m = 1 << i
            while c:
                p = c.bit_length() - 1
                if p not in basis:
                    basis[p] = (c, m)
                    break
                c, m = c ^ basis[p][0], m ^ basis[p][1]
        sel = 0
        while want and want.bit_length() - 1 in basis:
            v, m = basis[want.bit_length() - 1]
            want, sel = want ^ v, sel ^ m
        if want:
            continue
        w = np.array([b[i] if (sel >> i) & 1 else a[i] for i in range(WINDOW)], np.uint8)
        if oracle.window_hash(w, 63) == target and _isolated(oracle, avg, w):
            return w
    raise AssertionError(f"no window with hash {target:#x}")
