"""Cut candidates planted at the kernels' own boundaries (tests/planted.py): every lane
segment, tile, round switch, tail item, call boundary, min/max edge and record limit gets a
candidate on purpose instead of by chance.  Each input is proved on the CPU first
(test_planted_cpu.py runs check() over the same case table); here the HIP paths must give
the oracle's cut list, take the intended path and report the planted number of candidates.

Run on an MI355X:  python -m pytest tests/test_gpu_planted.py -m gpu -q
"""
import contextlib
import functools
import os

import numpy as np
import pytest

import planted
from planted import KiB, MiB, GiB

pytestmark = pytest.mark.gpu

BGS = ("zeros", "const", "p32", "random_defused")
PTR_OFFS = (0, 1, 3, 15)
WAVES_PER_WG, RESOLVER_WAVES = 8, 5  # kFusedWavesPerWG, kFusedResolverWaves

# how a path is forced, and what last_timing() then says
PATH_ENV = {
    "fused": {"PBS_FUSED": "1", "PBS_STATIC_QMAX": "32"},
    "pool": {"PBS_FUSED": "1", "PBS_STATIC_QMAX": "32", "PBS_POOL_DIV": "2"},
    # the fused pass at a 4 KiB average: min_eff = 1 KiB, so the few KiB past the tiles hold
    # several candidates (covered, inner tail blocks, the last partial block)
    "fusedtail": {"PBS_FUSED": "1", "PBS_STATIC_QMAX": "32", "PBS_FUSED_MIN_AVG": "4096"},
    "fuseddyn": {"PBS_FUSED": "1", "PBS_SCAN_DYN": "1"},  # dynamic tile order, small tiles at the end
    "scanpass": {"PBS_STATIC_QMAX": "32"},
    "multi": {"PBS_FUSED": "0"},
    "multidyn": {"PBS_FUSED": "0", "PBS_SCAN_DYN": "1"},
    "small": {},
}
TIMING_PATH = {"pool": "fused", "fusedtail": "fused", "fuseddyn": "fused", "multidyn": "multi"}
TAIL = 5 * KiB + 77  # past the tiles: one tail item of 41 blocks, the last one partial


def _case(path, avg, cu, n, kb, ko, **more):
    bg, off = BGS[kb], PTR_OFFS[ko]
    return {"id": f"{path}-{avg // KiB or avg}{'K' if avg >= KiB else ''}-cu{cu}-{bg}-off{off}",
            "path": path, "avg": avg, "cu": cu, "n": n, "bg": bg, "off": off, "rot": 5 * kb + ko, **more}


# A. one buffer per (path, background, pointer offset); a path's variants (average, compute
# units, size) are spread over its sixteen buffers
CROSS = [(kb, ko) for kb in range(4) for ko in range(4)]
FUSED_VARIANTS = [(128 * KiB, 2, 32 * MiB + TAIL), (128 * KiB, 4, 24 * MiB + 77),
                  (4 * MiB, 2, 32 * MiB + 77), (4 * MiB, 4, 24 * MiB + TAIL)]
MULTI_VARIANTS = [(128 * KiB, 4, 24 * MiB + 200 * KiB + 77), (4 * KiB, 4, 8 * MiB + TAIL)]
SMALL_VARIANTS = [(4 * KiB, 4, 1 * MiB), (256, 4, 300 * KiB + 5)]
EDGE_CASES = (
    [_case("fused", *FUSED_VARIANTS[(kb + ko) % 4], kb, ko) for kb, ko in CROSS]
    + [_case("pool", 128 * KiB, 2, 32 * MiB + 77, kb, ko) for kb, ko in CROSS]
    + [_case("fusedtail", 4 * KiB, 4, 8 * MiB + TAIL, kb, ko, lane_gap=4 * KiB) for kb, ko in CROSS]
    + [_case("scanpass", 64 * KiB, 4, 24 * MiB + (TAIL if ko % 2 else 77), kb, ko) for kb, ko in CROSS]
    + [_case("multi", *MULTI_VARIANTS[(kb + ko) % 2], kb, ko) for kb, ko in CROSS]
    + [_case("small", *SMALL_VARIANTS[(kb + ko) % 2], kb, ko) for kb, ko in CROSS]
    + [_case("fuseddyn", 128 * KiB, 2, 32 * MiB + 77, k, (k + 1) % 4) for k in range(4)]
    + [_case("multidyn", (128 * KiB, 64 * KiB)[k % 2], 2, 32 * MiB + 77, k, (k + 2) % 4) for k in range(4)]
)
EDGE_BY_ID = {c["id"]: c for c in EDGE_CASES}
assert len(EDGE_BY_ID) == len(EDGE_CASES)


def edge_id(path, avg, cu, bg):
    return next(c["id"] for c in EDGE_CASES if (c["path"], c["avg"], c["cu"], c["bg"]) == (path, avg, cu, bg))


@contextlib.contextmanager
def env(values):
    """The library reads its knobs with getenv when a handle is made or a plan is laid."""
    old = {k: os.environ.get(k) for k in values}
    os.environ.update(values)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def tail_picks(g, min_eff):
    """Up to three inner block starts of the bytes past the tiles, far enough from `covered`,
    from each other and from the last block for candidates a minimum chunk apart."""
    step = max(9, min_eff // planted.BLOCK + 1)
    return [b for b in g["tail_blocks"][step::step][:3] if b + 64 + max(min_eff, 128) < g["last_block"][0]]


def edge_groups(gpu, case):
    """(the boundaries of a case's path, the rare ones first and the lane segments last; the
    geometry they come from)."""
    n, cu, path, off = case["n"], case["cu"], case["path"], case["off"]
    _, min_eff, _ = planted.params(case["avg"])
    with env(PATH_ENV[path]):
        if path in ("fused", "pool", "fusedtail", "scanpass"):
            nw = cu * WAVES_PER_WG - (0 if path == "scanpass" else RESOLVER_WAVES)
            g = planted.fused_segments(gpu, n, nw)
            if path == "pool":
                assert g["plan"]["pool"] == 1, g["plan"]
            rare = [g["t_long"], g["t_small"], [g["covered"]], tail_picks(g, min_eff), g["last_block"], g["short"],
                    g["tiles"]]
        elif path in ("multi", "multidyn", "fuseddyn"):  # scan_main's plan (the fused pass's dynamic order too)
            g = planted.scan_main_segments(gpu, n, cu)
            assert (path == "multi") == (g["plan"]["t_big"] == g["plan"]["ntiles"]), g["plan"]
            rare = [g["t_big"], [g["covered"]], tail_picks(g, min_eff), g["last_block"], g["tiles"]]
        else:  # scan_blocks_kernel: 128-byte blocks on 16-byte-aligned addresses
            mis = off & 15
            g = {"lanes": [b - mis for b in range(0, n + mis, planted.BLOCK)]}
            rare = [[g["lanes"][-1]], [g["lanes"][1]]]
    rot = case["rot"] % len(rare)
    rare = rare[rot:] + rare[:rot]
    return [([n - 1], (0,))] * (case["rot"] % 2) + rare + [([n - 1], (0,))], g


@functools.lru_cache(maxsize=8)
def build_edge(case_id):
    """(data, positions, positions that no rule lets cut, reference cut list)."""
    import oracle
    import pbschunk
    case = EDGE_BY_ID[case_id]
    avg, n = case["avg"], case["n"]
    _, min_eff, _ = planted.params(avg)
    start = [63 + case["rot"] % 2]  # p = 63 / 64: the first positions with a full window
    rare, g = edge_groups(pbschunk, case)
    pos = planted.place_edges(rare, min_eff, n, case["rot"], taken=start)
    # (lane_gap: a tile's record takes 64 flagged blocks, so small averages space the lanes' share)
    pos += planted.place_edges([g["lanes"]], case.get("lane_gap", min_eff), n, case["rot"], taken=start + pos)
    pos = sorted(start + pos)
    data = planted.make_input(oracle, avg, case["bg"], n, pos, seed=len(case_id))
    ref = planted.check(oracle, avg, data, pos)
    return data, pos, [p for p in start if p < min_eff - 1], ref


def to_device(data, off):
    """The bytes at a device address that is `off` past an aligned allocation."""
    import torch
    dev = torch.empty(data.size + 64, dtype=torch.uint8, device="cuda")
    assert dev.data_ptr() % 256 == 0
    dev[off:off + data.size] = torch.from_numpy(data)
    torch.cuda.synchronize()
    return dev, dev.data_ptr() + off


def assert_path(t, path, n):
    path = TIMING_PATH.get(path, path)
    if path == "fused":
        assert t["fused"] == n and t["scan_pass"] == 0, t
    elif path == "scanpass":
        assert t["fused"] == n and t["scan_pass"] == n, t
    else:
        assert t["fused"] == 0 and t["scan_pass"] == 0, t


def cuts_device(gpu, case, data, final=True):
    dev, ptr = to_device(data, case["off"])
    with gpu.Chunker(case["avg"]) as c:
        c.set_cu_count(case["cu"])
        got = c.find_cuts_device(ptr, data.size, is_final=final)
        t = c.last_timing()
    del dev
    return got, t


# ---------------------------------------------------------------- A. geometry edges

@pytest.mark.parametrize("case_id", list(EDGE_BY_ID))
def test_edges(gpu, monkeypatch, case_id):
    case = EDGE_BY_ID[case_id]
    data, pos, _, ref = build_edge(case_id)
    for k, v in PATH_ENV[case["path"]].items():
        monkeypatch.setenv(k, v)
    got, t = cuts_device(gpu, case, data)
    assert np.array_equal(got, ref), (got.size, ref.size, np.setxor1d(got, ref)[:8])
    assert_path(t, case["path"], data.size)
    assert t["candidates"] == len(pos), t


KNOB_CASE = edge_id("fused", 128 * KiB, 2, "zeros")
KNOBS = {
    "dyn": {"PBS_SCAN_DYN": "1"},
    "dyn-nosmall": {"PBS_SCAN_DYN": "1", "PBS_SCAN_SMALL": "0"},
    "dyn-maxseg8k": {"PBS_SCAN_DYN": "1", "PBS_MAX_SEG": "8192"},
    "balance0": {"PBS_BALANCE": "0"},
    "balance2": {"PBS_BALANCE": "2"},
    "direct-out0": {"PBS_DIRECT_OUT": "0"},
    "sync-mode0": {"PBS_SYNC_MODE": "0"},
}


@pytest.mark.parametrize("knob", list(KNOBS))
def test_fused_knobs(gpu, monkeypatch, knob):
    """The same fused buffer under the knobs no other test sets (defaults in pbs_chunker_new:
    balance 1, direct out on, sync mode 1, static order): the same cuts, still one fused pass."""
    case = EDGE_BY_ID[KNOB_CASE]
    data, pos, _, ref = build_edge(KNOB_CASE)
    for k, v in {**PATH_ENV["fused"], **KNOBS[knob]}.items():
        monkeypatch.setenv(k, v)
    got, t = cuts_device(gpu, case, data)
    assert np.array_equal(got, ref), (got.size, ref.size, np.setxor1d(got, ref)[:8])
    assert_path(t, "fused", data.size)
    assert t["candidates"] == len(pos), t


@pytest.mark.parametrize("knob", ["direct-out0", "sync-mode0"])
def test_scan_pass_pinned_out_knobs(gpu, monkeypatch, knob):
    """PBS_DIRECT_OUT / PBS_SYNC_MODE act on the resolve into a pinned cut array (the scan
    pass and the multi-kernel resolve): the scan-pass buffer into pinned memory, both ways."""
    import torch
    case_id = edge_id("scanpass", 64 * KiB, 4, "zeros")
    case = EDGE_BY_ID[case_id]
    data, pos, _, ref = build_edge(case_id)
    for k, v in {**PATH_ENV["scanpass"], **KNOBS[knob]}.items():
        monkeypatch.setenv(k, v)
    dev, ptr = to_device(data, case["off"])
    with gpu.Chunker(case["avg"]) as c:
        c.set_cu_count(case["cu"])
        out = torch.empty(c.cuts_bound(data.size), dtype=torch.int64, pin_memory=True).numpy().view(np.uint64)
        got = c.find_cuts_device(ptr, data.size, is_final=True, out=out).copy()
        t = c.last_timing()
    assert np.array_equal(got, ref)
    assert_path(t, "scanpass", data.size)
    assert t["candidates"] == len(pos), t


CAND_DEV = {"avg": 128 * KiB, "cu": 4, "n": 24 * MiB + 40 * KiB + 77, "s0": 4099}


@functools.lru_cache(maxsize=4)
def build_cand_dev(bg):
    """A stream whose bytes from s0 on are one candidates_device call: candidates at the edges
    of that call's scan_main tiles, from its first byte on (windows that begin in `pre`)."""
    import oracle
    import pbschunk
    avg, cu, n, s0 = (CAND_DEV[k] for k in ("avg", "cu", "n", "s0"))
    with env(PATH_ENV["multi"]):
        g = planted.scan_main_segments(pbschunk, n - s0, cu)
    groups = [[s0 + b for b in grp] for grp in (g["tiles"], [g["covered"]], tail_picks(g, 1024), g["last_block"],
                                                g["lanes"])]
    pos = planted.place_edges([([s0], (0,)), ([n - 1], (0,))] + groups, 1024, n, rot=len(bg), lo=1024)
    pos = sorted(pos + [s0 - 200])  # one before the call's range: not reported
    data = planted.make_input(oracle, avg, bg, n, pos, seed=5)
    planted.check(oracle, avg, data, pos)
    return data, pos


CAND_BASES = {"natural": None, "base0": 0, "2^32-100": 2**32 - 100, "2^40+5": 2**40 + 5}


@pytest.mark.parametrize("bg,off,base", [(BGS[kb], PTR_OFFS[ko], list(CAND_BASES)[(kb + ko) % 4]) for kb, ko in CROSS])
def test_candidates_device_edges(gpu, monkeypatch, bg, off, base):
    """candidates_device over [s0, n) with the 63 bytes before as `pre`, at the stream offset
    the bytes really have, and at bases around 2^32 and 2^40 (E): the planted positions,
    shifted; base 0 without history drops the positions below 63.  One buffer per
    (background, pointer offset), the bases spread over them."""
    import torch
    data, pos = build_cand_dev(bg)
    avg, cu, n, s0 = (CAND_DEV[k] for k in ("avg", "cu", "n", "s0"))
    monkeypatch.setenv("PBS_FUSED", "0")
    b = s0 if CAND_BASES[base] is None else CAND_BASES[base]
    pre = data[s0 - 63:s0].tobytes() if b else b""
    want = np.array([p - s0 + b for p in pos if p >= s0 + (0 if b else 63)], dtype=np.uint64)
    assert want.size and (b == 0 or want[0] == b)  # a candidate on the call's first byte
    dev, ptr = to_device(data[s0:], off)
    out = torch.zeros(want.size + 16, dtype=torch.int64, device="cuda")
    with gpu.Chunker(avg) as c:
        c.set_cu_count(cu)
        k = c.candidates_device(ptr, n - s0, pre, b, out.data_ptr(), out.numel())
    got = out.cpu().numpy().view(np.uint64)[:k]
    assert np.array_equal(got, want), (k, want.size, np.setxor1d(got, want)[:8])


def scan_reads(c, data, sizes):
    """scan() driven like a reader loop over reads of the given sizes: the cut list."""
    got, pos = [], 0
    for s in sizes:
        p = data[pos:pos + s]
        off = 0
        while off < p.size:
            k = c.scan(p[off:])
            if k == 0:
                break
            off += k
            got.append(pos + off)
        pos += p.size
    return np.array(got, dtype=np.uint64)


def server_plan(avg, n, read, wgs, minpass=1):
    """Candidates at the lane, pass and workgroup boundaries of every scan-server request of
    a stream read `read` bytes at a time.  A request covers what scan() has not seen of a
    read, minus the bytes no cut can fall in (up to chunk_start + min_eff - 1 - 63), so the
    requests follow from the cuts: the reads are planned one after the other."""
    _, min_eff, _ = planted.params(avg)
    pos, chunk_start, scanned, requests = [], 0, 0, 0
    for i, a in enumerate(range(0, n, read)):
        b = min(a + read, n)
        lo = chunk_start + min_eff - 1
        start = max(scanned, min(b, max(lo - 63, 0)))
        scanned = b
        if start >= b:
            continue
        requests += 1
        g = planted.server_segments(b - start, wgs, minpass)
        groups = [[start + x for x in grp] for grp in (g["wgs"], g["passes"], g["lanes"])]
        new = planted.place_edges(groups, min_eff, b, rot=i, lo=max(lo, start), taken=pos)
        pos += new
        if new:
            chunk_start = new[-1] + 1
    return pos, requests


SERVER_CASES = [(8 * KiB, "3"), (24 * KiB, "32"), (256 * KiB + 3, "3"), (256 * KiB + 3, "32"), (1 * MiB, "32")]


@functools.lru_cache(maxsize=2)
def build_server(read, wgs, bg):
    import oracle
    avg = 4 * KiB
    n = min(6 * MiB + 77, 40 * read + 77)
    pos, requests = server_plan(avg, n, read, int(wgs))
    data = planted.make_input(oracle, avg, bg, n, pos, seed=9)
    planted.check(oracle, avg, data, pos)
    return avg, data, pos, requests


def assert_served(c, requests=None, refused=0):
    """The scan server took the reads: every request sent was served, but `refused` of them."""
    st = c.stats_for_test()
    assert st["broken"] == 0 and st["requests"] > 0 and st["served"] == st["requests"] - refused, st
    assert requests is None or st["requests"] == requests, (st, requests)


# (PBS_SERVER_POLL=4: lane 0 of every wave polls; the flag is read by the server alone)
@pytest.mark.parametrize("bg", BGS)
@pytest.mark.parametrize("read,wgs,poll", [(r, w, None) for r, w in SERVER_CASES] + [(256 * KiB + 3, "32", "4")],
                         ids=[f"{r}-wgs{w}" for r, w in SERVER_CASES] + ["262147-wgs32-poll4"])
def test_scan_server_edges(gpu, oracle, monkeypatch, read, wgs, poll, bg):
    monkeypatch.setenv("PBS_SERVER_WGS", wgs)
    monkeypatch.setenv("PBS_SERVER_MINPASS", "1")
    if poll:
        monkeypatch.setenv("PBS_SERVER_POLL", poll)
    avg, data, pos, requests = build_server(read, wgs, bg)
    with gpu.Chunker(avg) as c:
        got = scan_reads(c, data, [read] * (data.size // read + 1))
        t = c.last_timing()
        assert_served(c, requests)
    ref = oracle.chunk_feed(avg, data)
    assert np.array_equal(got, ref), (got.size, ref.size, np.setxor1d(got, ref)[:8])
    assert t["fused"] == 0 and t["scan_pass"] == 0, t


# ---------------------------------------------------------------- B. call boundaries

def feed(gpu, api, avg, data, splits, cu=None):
    """The stream in pieces [splits[i], splits[i+1]) through find_cuts, find_cuts_device or
    scan(): the cut list (scan(): without the EOF tail)."""
    bounds = [0] + [int(s) for s in splits] + [data.size]
    with gpu.Chunker(avg) as c:
        if cu:
            c.set_cu_count(cu)
        if api == "scan":
            return scan_reads(c, data, np.diff(bounds)), c.last_timing(), c.stats_for_test()
        if api == "device":
            dev, ptr = to_device(data, 0)
        got = []
        for a, b in zip(bounds[:-1], bounds[1:]):
            if api == "device":
                got.append(c.find_cuts_device(ptr + a, b - a, is_final=b == data.size))
            else:
                got.append(c.find_cuts(data[a:b], is_final=b == data.size))
        return np.concatenate(got), c.last_timing(), c.stats_for_test()


def boundary_input(oracle, avg, gap, js, bg, middles=()):
    """One window per split: window i ends j bytes after split i (j from -1, the window wholly
    in the earlier call, to 63, wholly in the later one); then, for every m of `middles`, a
    window across a piece of m bytes between two more splits, so the history of the call after
    it is assembled from two calls.  (data, positions, splits, reference)"""
    _, min_eff, _ = planted.params(avg)
    pos, splits, at = [], [], max(gap, min_eff)
    for j in js:
        splits.append(at)
        pos.append(at + j)
        at += gap + 37
    for m in middles:
        splits += [at, at + m]
        pos.append(at + m + 20)  # bytes before, inside (all m of them) and after the middle piece
        at += gap + 37
    n = at + 5
    data = planted.make_input(oracle, avg, bg, n, pos, seed=11)
    return data, pos, splits, planted.check(oracle, avg, data, pos)


ALL_J = list(range(-1, 64))
MIDDLES = (1, 7, 62, 63, 64)
# pieces past the small path's and the server's 1 MiB, also after scan() has skipped the up to
# min_eff bytes behind a cut in which none can fall; all 65 offsets take two buffers
BIG = 1 * MiB + 40 * KiB
B_CASES = {
    # pieces <= 1 MiB: the one-launch small path (and the scan server for scan())
    "small-4K": (4 * KiB, 3 * KiB, ALL_J, MIDDLES, "random_defused", {}, None),
    # pieces > 1 MiB: the fused pass, the scan pass, the multi-launch path; scan() then scans
    # each piece with scan_main + exact + sort and carries the 63 bytes itself
    "fused-128K-a": (128 * KiB, BIG, ALL_J[0::2], MIDDLES, "zeros", PATH_ENV["fused"], 2),
    "fused-128K-b": (128 * KiB, BIG, ALL_J[1::2], (), "random_defused", PATH_ENV["fused"], 2),
    "scanpass-64K-a": (64 * KiB, BIG, ALL_J[0::2], MIDDLES, "p32", PATH_ENV["scanpass"], 4),
    "scanpass-64K-b": (64 * KiB, BIG, ALL_J[1::2], (), "zeros", PATH_ENV["scanpass"], 4),
    "multi-128K-a": (128 * KiB, BIG, ALL_J[0::2], MIDDLES, "const", PATH_ENV["multi"], 4),
    "multi-128K-b": (128 * KiB, BIG, ALL_J[1::2], (), "p32", PATH_ENV["multi"], 4),
}


@functools.lru_cache(maxsize=2)
def build_boundary(name):
    import oracle
    avg, gap, js, middles, bg, _, _ = B_CASES[name]
    return boundary_input(oracle, avg, gap, js, bg, middles)


@pytest.mark.parametrize("api", ["host", "device", "scan"])
@pytest.mark.parametrize("name", list(B_CASES))
def test_call_boundaries(gpu, oracle, monkeypatch, name, api):
    avg, gap, _, middles, _, envs, cu = B_CASES[name]
    data, pos, splits, ref = build_boundary(name)
    assert data.size <= 48 * MiB
    for k, v in envs.items():
        monkeypatch.setenv(k, v)
    got, t, st = feed(gpu, api, avg, data, splits, cu)
    if api == "scan":
        ref = oracle.chunk_feed(avg, data)
    assert np.array_equal(got, ref), (got.size, ref.size, np.setxor1d(got, ref)[:8])
    if api != "scan":
        assert_path(t, name.split("-")[0], data.size - splits[-1])
    elif gap > 1 * MiB:  # scan() knows no fused pass; without a piece of at most 1 MiB the server
        assert t["fused"] == 0 and t["bytes"] > 1 * MiB, t  # never ran: the batch path scanned them all
        assert middles or st["requests"] == 0, st
    else:
        assert st["served"] == st["requests"] > 0 and st["broken"] == 0, st


# ---------------------------------------------------------------- C. the min/max rule

C_CASES = {
    "fused-128K": ("fused", 128 * KiB, 8 * MiB + 5, 2, "zeros"),
    "fused-4M": ("fused", 4 * MiB, 40 * MiB + 5, 2, "random_defused"),
    "scanpass-64K": ("scanpass", 64 * KiB, 6 * MiB + 5, 4, "const"),
    "small-4K": ("small", 4 * KiB, 1 * MiB, 4, "p32"),
    "multi-128K": ("multi", 128 * KiB, 8 * MiB + 5, 4, "random_defused"),
}


@functools.lru_cache(maxsize=2)
def build_minmax(name):
    import oracle
    _, avg, n, _, bg = C_CASES[name]
    pos = planted.minmax_positions(oracle, avg, n)
    data = planted.make_input(oracle, avg, bg, n, pos, seed=13)
    return data, pos, planted.check(oracle, avg, data, pos)


@pytest.mark.parametrize("name", list(C_CASES))
def test_minmax_edges(gpu, monkeypatch, name):
    """Candidates at s+min-2, s+min-1, s+max-1, s+max and a chain min-1 apart (planted.
    minmax_positions) through every resolver that sits behind a scan."""
    path, avg, n, cu, _ = C_CASES[name]
    data, pos, ref = build_minmax(name)
    for k, v in PATH_ENV[path].items():
        monkeypatch.setenv(k, v)
    got, t = cuts_device(gpu, {"avg": avg, "cu": cu, "off": 0}, data)
    assert np.array_equal(got, ref), (got.size, ref.size, np.setxor1d(got, ref)[:8])
    assert_path(t, path, n)
    assert t["candidates"] == len(pos), t


@functools.lru_cache(maxsize=1)
def build_first_test():
    import oracle
    data, pos = planted.first_test_input(oracle, 48 * KiB)
    return data, pos, planted.check(oracle, 256, data, pos)


@pytest.mark.parametrize("api", ["host", "scan"])
def test_first_test_rule(gpu, oracle, api):
    """Average 256: min_eff is 65 because the first test of a chunk comes at size 65 -- a
    candidate at s+63 (size 64) is ignored, one at s+64 cuts."""
    data, pos, ref = build_first_test()
    got, t, _ = feed(gpu, api, 256, data, [] if api == "host" else [8 * KiB, 8 * KiB + 63, 20 * KiB])
    if api == "scan":
        ref = oracle.chunk_feed(256, data)
    assert np.array_equal(got, ref), (got.size, ref.size, np.setxor1d(got, ref)[:8])


def synthetic_lists(oracle):
    """name -> (avg, sorted candidate list, stream end) for resolve_device alone."""
    rng = np.random.default_rng(0x5EED)
    out = {}
    for avg in (4 * KiB, 128 * KiB):
        p = planted.minmax_positions(oracle, avg, 600 * avg, adjacent=True)
        out[f"edges-{avg // KiB}K"] = (avg, p, p[-1] + 100)
    # either side of kSmallResolveMax (16384 nodes = the list + 2): gaps around min_eff
    _, mn, mx = planted.params(4 * KiB)
    gaps = rng.choice([1, 64, mn - 2, mn - 1, mn, mn + 1, 2 * mn, mx - 1, mx, mx + 1], 16383)
    p = (np.cumsum(gaps) + 63).tolist()
    out["16382"] = (4 * KiB, p[:16382], p[16381] + mx + 7)
    out["16383"] = (4 * KiB, p, p[-1] + mx + 7)
    # forced-cut runs longer than 256 between candidates, and after the last one
    _, mn, mx = planted.params(256)
    p = np.cumsum(rng.choice([mn - 1, mn, 300 * mx + 5, 257 * mx, 700 * mx - 1], 40)).tolist()
    out["forced-runs"] = (256, p, p[-1] + 1000 * mx + 3)
    # positions beyond 2^32
    _, mn, mx = planted.params(4 * MiB)
    near = 2**32
    p = [near - mx - 1, near - mn, near - 1, near + mn - 2, near + mn - 1, near + 2 * mn, near + 2 * mn + mx]
    out["beyond-2^32"] = (4 * MiB, p, near + 5 * mx + 9)
    return out


@pytest.mark.parametrize("name", ["edges-4K", "edges-128K", "16382", "16383", "forced-runs", "beyond-2^32"])
def test_resolve_device_synthetic(gpu, oracle, name):
    """resolve_device fed lists that no scan produced, against the oracle's resolve."""
    import torch
    avg, cand, end = synthetic_lists(oracle)[name]
    cand = np.asarray(cand, dtype=np.uint64)
    assert np.all(np.diff(cand.astype(np.int64)) > 0) and int(cand[-1]) < end
    ref = oracle.resolve(avg, cand, end)
    if ref.size == 0 or int(ref[-1]) != end:
        ref = np.append(ref, np.uint64(end))
    dev = torch.from_numpy(cand.view(np.int64)).to("cuda")
    torch.cuda.synchronize()
    with gpu.Chunker(avg) as c:
        got = c.resolve_device(dev.data_ptr(), cand.size, end, is_final=True)
    assert np.array_equal(got, ref), (got.size, ref.size, np.setxor1d(got, ref)[:8])


# ---------------------------------------------------------------- D. limits, both sides

def one_tile_input(oracle, gpu, path, avg, cu, n, count, stride):
    """`count` candidates in `count` different blocks of one tile (not tile 0, whose first
    block is always evaluated), each window inside its own block."""
    with env(PATH_ENV[path]):
        g = planted.fused_segments(gpu, n, cu * WAVES_PER_WG - (0 if path == "scanpass" else RESOLVER_WAVES))
    t0, t1 = g["tiles"][2], g["tiles"][3]
    pos = [t0 + stride * planted.BLOCK * i + 100 for i in range(count)]
    assert pos[-1] < t1
    data = planted.make_input(oracle, avg, "zeros", n, pos, seed=17)
    return data, pos, planted.check(oracle, avg, data, pos)


@pytest.mark.parametrize("path,avg,cu,n,limit", [("fused", 128 * KiB, 2, 32 * MiB + 77, 64),
                                                 ("scanpass", 64 * KiB, 4, 24 * MiB + 77, 256)],
                         ids=["fused-64", "scanpass-4x64"])
@pytest.mark.parametrize("over", [0, 1], ids=["at", "over"])
def test_flagged_blocks_per_tile(gpu, oracle, monkeypatch, path, avg, cu, n, limit, over):
    """A tile's record(s) take 64 (fused pass) or 4 x 64 (scan pass) flagged blocks: at the
    limit the pass serves the batch, one block more and it stands down; the cuts are the
    oracle's either way."""
    data, pos, ref = one_tile_input(oracle, gpu, path, avg, cu, n, limit + over, 2 if path == "fused" else 3)
    for k, v in PATH_ENV[path].items():
        monkeypatch.setenv(k, v)
    got, t = cuts_device(gpu, {"avg": avg, "cu": cu, "off": 0}, data)
    assert np.array_equal(got, ref), (got.size, ref.size, np.setxor1d(got, ref)[:8])
    if over and path == "fused":  # stood down; at 128 KiB the scan pass (4 records a tile) serves it
        assert t["fused"] == n and t["scan_pass"] == n, t
    elif over:
        assert t["fused"] == 0 and t["scan_pass"] == 0, t
    else:
        assert_path(t, path, n)
        assert t["suspects"] == limit + 1, t  # + the stream's first block
    assert t["candidates"] == len(pos), t


@functools.lru_cache(maxsize=2)
def build_keep(count):
    """A cut, then `count` candidates inside the new chunk's minimum, and the stream ends
    before a forced cut: the open chunk keeps exactly `count` candidates."""
    import oracle
    avg, n = 128 * KiB, 6 * MiB + 400 * KiB + 77
    data = np.zeros(n, np.uint8)
    p0 = 6 * MiB + 100 * KiB
    planted.plant(data, [p0], planted.passing_windows(oracle, avg))
    planted.dense_run(oracle, avg, data, p0 + 1 + 4 * KiB, count, planted.passing_pattern(oracle, 7, avg))
    cand = oracle.candidates(avg, data)
    ref = oracle.chunk_feed(avg, data)
    assert cand.size == count + 1 and int(cand[0]) == p0 and int(ref[-1]) == p0 + 1
    assert int(cand[-1]) < p0 + 32 * KiB - 1 and p0 + 1 + 512 * KiB > n
    return data, cand, np.append(ref, np.uint64(n))


@pytest.mark.parametrize("count", [512, 513])
def test_open_chunk_candidates_limit(gpu, monkeypatch, count):
    """kFusedKeep: the fused pass's resolver keeps 512 candidates of the open chunk; with 513
    it stands down (at 128 KiB the scan pass then serves the batch).  The oracle's cuts either
    way."""
    data, cand, ref = build_keep(count)
    n = data.size
    for k, v in PATH_ENV["fused"].items():
        monkeypatch.setenv(k, v)
    got, t = cuts_device(gpu, {"avg": 128 * KiB, "cu": 2, "off": 0}, data)
    assert np.array_equal(got, ref), (got.size, ref.size, np.setxor1d(got, ref)[:8])
    assert t["fused"] == n and t["scan_pass"] == (0 if count == 512 else n), t
    assert t["candidates"] == cand.size, t


@functools.lru_cache(maxsize=2)
def build_capacity(over):
    """Exactly as many candidates as the fused pass's list holds (expected * 2 + 8192 with
    expected = bytes / avg * 3 / 2 + 1), or one more: dense runs of at most 48 blocks in as
    many tiles as it takes (a tile's record takes 64 flagged blocks), then one clean cut so
    that the open chunk keeps nothing."""
    import oracle
    import pbschunk
    avg, cu, n = 128 * KiB, 2, 32 * MiB + 77
    cap = (n // avg * 3 // 2 + 1) * 2 + 8192
    with env(PATH_ENV["fused"]):
        g = planted.fused_segments(pbschunk, n, cu * WAVES_PER_WG - RESOLVER_WAVES)
    pat = planted.passing_pattern(oracle, 7, avg)
    data = np.zeros(n, np.uint8)
    total, t = 0, 2
    while cap + over - total > 700:
        total, t = total + 600, t + 1
        assert planted.dense_run(oracle, avg, data, g["tiles"][t] + 1024, 600, pat) <= 48 * planted.BLOCK
    assert planted.dense_run(oracle, avg, data, g["tiles"][t + 1] + 1024, cap + over - total - 1, pat) <= 48 * planted.BLOCK
    planted.plant(data, [g["tiles"][t + 2] + 100], planted.passing_windows(oracle, avg))
    cand = oracle.candidates(avg, data)
    assert cand.size == cap + over, (cand.size, cap)
    ref = oracle.chunk_feed(avg, data)
    return data, cand, ref if int(ref[-1]) == n else np.append(ref, np.uint64(n))


@pytest.mark.parametrize("over", [0, 1], ids=["at", "over"])
def test_candidate_list_capacity(gpu, monkeypatch, over):
    """The candidate list of fused_pass: full to the last entry the pass serves the batch,
    one candidate more and it stands down (the scan pass's list is as long: the multi-launch
    path, which grows its list, takes the batch)."""
    data, cand, ref = build_capacity(over)
    n = data.size
    for k, v in PATH_ENV["fused"].items():
        monkeypatch.setenv(k, v)
    got, t = cuts_device(gpu, {"avg": 128 * KiB, "cu": 2, "off": 0}, data)
    assert np.array_equal(got, ref), (got.size, ref.size, np.setxor1d(got, ref)[:8])
    if over:
        assert t["fused"] == 0 and t["scan_pass"] == 0, t
    else:
        assert_path(t, "fused", n)
    assert t["candidates"] == cand.size, t


def test_scan_server_one_region_overflows(gpu, oracle, monkeypatch):
    """A 1 MiB read split over 32 workgroups (512 candidates each): one 8 KiB pass of a
    passing period-7 pattern (~1170 candidates) overflows one workgroup's region while the
    others hold nothing; scan() takes the batch path for that read -- the oracle's cuts."""
    avg = 4 * KiB
    monkeypatch.setenv("PBS_SERVER_WGS", "32")
    monkeypatch.setenv("PBS_SERVER_MINPASS", "1")
    pat = planted.passing_pattern(oracle, 7, avg)
    data = np.zeros(3 * MiB + 5, np.uint8)
    at = 1 * MiB + 41 * 8 * KiB  # pass 41 of the second read: workgroup 10's range
    data[at:at + 8 * KiB] = np.tile(pat, 8 * KiB // 7 + 1)[:8 * KiB]
    cand = oracle.candidates(avg, data)
    assert cand.size > 16384 // 32 and cand[0] >= at and cand[-1] < at + 8 * KiB + 64
    ref = oracle.chunk_feed(avg, data)
    with gpu.Chunker(avg) as c:
        got = scan_reads(c, data, [1 * MiB] * 4)
        assert_served(c, refused=1)  # the second read came back "too many": the batch path took it
    assert np.array_equal(got, ref), (got.size, ref.size, np.setxor1d(got, ref)[:8])


# ---------------------------------------------------------------- E. absolute offsets

def test_offsets_beyond_4gib(gpu, oracle, monkeypatch):
    """One handle: 4 GiB of zeros (cuts at the multiples of max_eff), then a planted buffer
    whose cuts are the oracle's on that buffer alone, shifted by 4 GiB -- the reference
    restarts at a cut, and 4 GiB is one."""
    import torch
    case = EDGE_BY_ID[edge_id("fused", 4 * MiB, 2, "p32")]
    avg = case["avg"]
    _, _, max_eff = planted.params(avg)
    data, pos, _, ref = build_edge(case["id"])
    for k, v in PATH_ENV["fused"].items():
        monkeypatch.setenv(k, v)
    zeros = torch.zeros(4 * GiB, dtype=torch.uint8, device="cuda")
    dev, ptr = to_device(data, case["off"])
    with gpu.Chunker(avg) as c:
        first = c.find_cuts_device(zeros.data_ptr(), 4 * GiB, is_final=False)
        assert np.array_equal(first, np.arange(1, 4 * GiB // max_eff + 1, dtype=np.uint64) * np.uint64(max_eff))
        assert c.chunk_start == 4 * GiB
        c.set_cu_count(case["cu"])
        got = c.find_cuts_device(ptr, data.size, is_final=True)
        t = c.last_timing()
    del zeros
    assert np.array_equal(got, ref + np.uint64(4 * GiB)), (got.size, ref.size)
    assert_path(t, "fused", data.size)
    assert t["candidates"] == len(pos), t


# ---------------------------------------------------------------- F. epoch wrap

def test_fused_epoch_wrap(gpu, monkeypatch):
    """The tile records carry a 16-bit epoch: from 0xFFFD five passes on one handle cross the
    wrap (0xFFFE, 0xFFFF, then the records are zeroed and the count restarts at 1); each pass
    over a different planted buffer gives that buffer's cuts.  The first, largest buffer sizes
    the records, so no later pass re-allocates them (which would restart the epoch as well):
    the epoch read back after every pass shows the wrap was crossed."""
    for k, v in PATH_ENV["fused"].items():
        monkeypatch.setenv(k, v)
    ids = [edge_id("fused", 128 * KiB, cu, bg) for cu in (2, 4) for bg in BGS[:3]]
    with gpu.Chunker(128 * KiB) as c:
        c.set_cu_count(4)
        for i, cid in enumerate(ids):
            if i == 1:  # (the first pass allocates the records, which zeroes them and the epoch)
                c.set_fused_epoch_for_test(0xFFFD)
            data, pos, _, ref = build_edge(cid)
            dev, ptr = to_device(data, EDGE_BY_ID[cid]["off"])
            got = c.find_cuts_device(ptr, data.size, is_final=True)
            t = c.last_timing()
            assert np.array_equal(got, ref), (cid, got.size, ref.size)
            assert_path(t, "fused", data.size)
            assert t["candidates"] == len(pos), (cid, t)
            assert c.stats_for_test()["epoch"] == (1, 0xFFFE, 0xFFFF, 1, 2, 3)[i], (i, c.stats_for_test())


# ---------------------------------------------------------------- the threshold itself

T_CASES = {
    "fused-128K": ("fused", 128 * KiB, 2, 8 * MiB + 77),
    "fused-4M": ("fused", 4 * MiB, 2, 24 * MiB + 77),
    "scanpass-64K": ("scanpass", 64 * KiB, 4, 8 * MiB + 77),
    "multi-128K": ("multi", 128 * KiB, 4, 8 * MiB + 77),
    "multi-4K": ("multi", 4 * KiB, 4, 2 * MiB + 77),
    "small-4K": ("small", 4 * KiB, 4, 1 * MiB),
    "small-256": ("small", 256, 4, 64 * KiB + 5),
}


@functools.lru_cache(maxsize=2)
def build_threshold(name):
    """Windows whose hash equals the threshold exactly (planted.threshold_window), one per
    minimum chunk at shifting offsets within the 128-byte blocks."""
    import oracle
    _, avg, _, n = T_CASES[name]
    _, min_eff, _ = planted.params(avg)
    w = planted.threshold_window(oracle, avg)
    step = max(min_eff, 256) + 37
    pos = list(range(step + 63, n - 64, step))[:200]
    data = planted.plant(np.zeros(n, np.uint8), pos, {0: w, 1: w, 2: w})
    return data, pos, planted.check(oracle, avg, data, pos)


@pytest.mark.parametrize("name", list(T_CASES))
def test_hash_on_the_threshold(gpu, monkeypatch, name):
    """(H & mask) == mask - 2 with every higher bit zero: rotl(H, rot) == thr, the value at
    which the kernels' >= and a wrong > differ (scan screen, exact test)."""
    path, avg, cu, n = T_CASES[name]
    data, pos, ref = build_threshold(name)
    for k, v in PATH_ENV[path].items():
        monkeypatch.setenv(k, v)
    got, t = cuts_device(gpu, {"avg": avg, "cu": cu, "off": 0}, data)
    assert np.array_equal(got, ref), (got.size, ref.size, np.setxor1d(got, ref)[:8])
    assert_path(t, path, n)
    assert t["candidates"] == len(pos), t


@pytest.mark.parametrize("read", [8 * KiB, 256 * KiB + 3])
def test_hash_on_the_threshold_scan_server(gpu, oracle, read):
    data, pos, _ = build_threshold("multi-4K")
    with gpu.Chunker(4 * KiB) as c:
        got = scan_reads(c, data, [read] * (data.size // read + 1))
        assert_served(c)
    ref = oracle.chunk_feed(4 * KiB, data)
    assert np.array_equal(got, ref), (got.size, ref.size, np.setxor1d(got, ref)[:8])
    assert set(p + 1 for p in pos) <= set(ref.tolist())
