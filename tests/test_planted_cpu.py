"""The planted inputs of test_gpu_planted.py, proved on the CPU: every input holds exactly
the candidates its name claims (planted.check with the oracle), the candidates that were
placed a minimum chunk apart all cut, and the tile plans the placement relies on cover the
batch.  No GPU: the plan hooks of the library are host code."""
import numpy as np
import pytest

import planted
import test_gpu_planted as tg
from planted import KiB, MiB


def test_helpers(oracle):
    """passing_windows gives one window per residue; a periodic background has no candidate;
    edge_positions walks the offsets and keeps the gap."""
    for avg in (256, 4 * KiB, 64 * KiB, 128 * KiB, 512 * KiB, 4 * MiB):
        mask = 2 * avg - 1
        win = planted.passing_windows(oracle, avg)
        for r in (0, 1, 2):
            assert (oracle.window_hash(win[r], 63) & mask) == mask - 2 + r
    for kind in ("zeros", "const", "p32", "random_defused"):
        bg = planted.background(kind, 1 * MiB + 77, 3, oracle, 4 * KiB)
        assert oracle.candidates(4 * KiB, bg).size == 0
        if kind != "random_defused":
            assert all(oracle.window_hash(bg, p) == 0 for p in (63, 64, 95, 4099, bg.size - 1))
    pos = planted.edge_positions(range(0, 1 << 20, 4096), 1000, 1 << 20)
    assert pos[:7] == [4096, 8193, 12319, 16446, 20543, 24640, 28671]
    assert planted.edge_positions(range(0, 1 << 20, 4096), 10000, 1 << 20)[:3] == [12319, 24640, 36865]
    with pytest.raises(AssertionError):
        planted.plant(np.zeros(500, np.uint8), [100, 163], planted.passing_windows(oracle, 256))


@pytest.mark.parametrize("case_id", list(tg.EDGE_BY_ID))
def test_edge_inputs(oracle, pbschunk, case_id):
    """check() ran in build_edge; with min_gap = min_eff every planted p + 1 is a cut (but a
    stream-start candidate below the minimum); the boundary group placed first got its
    candidates; where the minimum chunk allows it (4 KiB averages, or a long multi-launch tail)
    the bytes past the tiles hold distinct candidates at `covered`, at inner tail blocks and in
    the last partial block or on the last byte."""
    case = tg.EDGE_BY_ID[case_id]
    data, pos, not_cut, ref = tg.build_edge(case_id)
    assert data.size == case["n"] <= 48 * MiB
    cuts = set(ref.tolist())
    assert [p for p in pos if p + 1 not in cuts] == not_cut
    _, min_eff, _ = planted.params(case["avg"])
    groups, g = tg.edge_groups(pbschunk, case)
    first = groups[0][0] if isinstance(groups[0], tuple) else groups[0]
    near = np.asarray(pos)
    for b in first:
        if min_eff <= b < case["n"] - 64:
            assert np.min(np.abs(near - b)) <= max(min_eff, 128), (case_id, b)
    assert len(pos) >= min(case["n"] // (2 * max(min_eff, 4096)), 16)
    if "covered" in g and case["n"] - g["covered"] > 4 * min_eff:
        cov, last = g["covered"], g["last_block"][0]
        assert any(cov - 1 <= p <= cov + 64 for p in pos), case_id
        assert sum(1 for p in pos if cov + 128 <= p < last - 64) >= 2, case_id
        assert any(p >= last - 1 for p in pos), case_id


def test_edge_cases_cover_the_plan(pbschunk):
    """The case table reaches every kind of tile: long and normal tiles (t_long), a short
    round (t_small), the pool, a tail item of many blocks, the dynamic order's small tiles
    (t_big < ntiles) for the fused pass and for scan_main; and every path but the two
    dynamic-order ones has one buffer per (background, pointer offset)."""
    seen, pairs = set(), {}
    for case in tg.EDGE_CASES:
        pairs.setdefault(case["path"], set()).add((case["bg"], case["off"]))
        _, g = tg.edge_groups(pbschunk, case)
        pl = g.get("plan", {})
        if case["path"] in ("fused", "pool", "fusedtail", "scanpass"):
            seen |= {k for k in ("t_long", "pool") if pl[k]}
            if pl["t_small"] < pl["ntiles"]:
                seen.add("short")
            if case["n"] - pl["covered"] > 32 * planted.BLOCK:
                seen.add("tail-" + case["path"])
        elif case["path"] != "small":
            if pl["t_big"] < pl["ntiles"]:
                seen.add("t_big-" + case["path"])
            if case["n"] - pl["covered"] > 32 * planted.BLOCK:
                seen.add("tail-" + case["path"])
    assert seen == {"t_long", "pool", "short", "tail-fused", "tail-fusedtail", "tail-scanpass", "tail-multi",
                    "t_big-fuseddyn", "t_big-multidyn"}, seen
    for path in ("fused", "pool", "fusedtail", "scanpass", "multi", "small"):
        assert len(pairs[path]) == 16, path


def test_cand_dev_and_server_inputs(oracle):
    s0 = tg.CAND_DEV["s0"]
    for bg in tg.BGS:
        data, pos = tg.build_cand_dev(bg)
        assert s0 in pos and s0 - 200 in pos and data.size - 1 in pos  # the call's first and last byte
    for read, wgs in tg.SERVER_CASES:
        for bg in tg.BGS:
            avg, data, pos, requests = tg.build_server(read, wgs, bg)
            ref = set(oracle.chunk_feed(avg, data).tolist())
            assert all(p + 1 in ref for p in pos), (read, wgs)
            assert len(pos) >= data.size // read and requests >= data.size // read // 2


@pytest.mark.parametrize("name", list(tg.B_CASES))
def test_boundary_inputs(oracle, name):
    data, pos, splits, ref = tg.build_boundary(name)
    assert data.size <= 48 * MiB and sorted(splits) == splits
    js = sorted(p - s for p, s in zip(pos, splits))  # (the first len(js) splits: one window each)
    assert set(tg.B_CASES[name][2]) <= set(js)


def test_boundary_cases_cover_every_offset():
    """Every path sees every j in -1..63 (the large-piece paths over two buffers) and the
    middle pieces of 1, 7, 62, 63 and 64 bytes."""
    for path in ("small", "fused", "scanpass", "multi"):
        cases = [v for k, v in tg.B_CASES.items() if k.startswith(path)]
        assert sorted(j for v in cases for j in v[2]) == list(range(-1, 64)), path
        assert any(tuple(v[3]) == (1, 7, 62, 63, 64) for v in cases), path


@pytest.mark.parametrize("name", list(tg.C_CASES))
def test_minmax_inputs(oracle, name):
    """The four edges behave as named: s+min-2 does not cut, s+min-1 does, s+max-1 and the
    forced cut coincide, s+max falls into the next chunk's minimum."""
    _, avg, n, _, _ = tg.C_CASES[name]
    _, mn, mx = planted.params(avg)
    data, pos, ref = tg.build_minmax(name)
    cuts = [0] + ref.tolist()
    ends = set(cuts)
    kinds = set()
    for p in pos:
        s = max(c for c in cuts if c <= p)  # start of the chunk p lies in
        if p + 1 in ends:
            kinds.add("min-1" if p - s == mn - 1 else "max-1" if p - s == mx - 1 else "cut")
        else:
            kinds.add("min-2" if p - s == mn - 2 else "max" if p == s and s - mx in ends else "ignored")
    need = {"min-2", "min-1", "cut"} | ({"max-1", "max"} if n > 3 * mx else set())
    assert need <= kinds, kinds


def test_first_test_input(oracle):
    data, pos, ref = tg.build_first_test()
    cuts = [0] + ref.tolist()
    d = [p - max(c for c in cuts if c <= p) for p in pos]
    assert d.count(63) >= 8 and d.count(64) >= 8
    assert all((p + 1 in set(cuts)) == (x >= 64) for p, x in zip(pos, d))


def test_limit_inputs(oracle, pbschunk):
    """The inputs at a limit hold what they claim: 64 / 65 and 256 / 257 candidates in as many
    blocks of one tile, 512 / 513 candidates in the open chunk, a full candidate list and one
    more (the builders assert the counts with the oracle)."""
    for path, avg, cu, n, limit in (("fused", 128 * KiB, 2, 32 * MiB + 77, 64), ("scanpass", 64 * KiB, 4, 24 * MiB + 77, 256)):
        for over in (0, 1):
            data, pos, ref = tg.one_tile_input(oracle, pbschunk, path, avg, cu, n, limit + over, 2 if path == "fused" else 3)
            assert len(set(p // planted.BLOCK for p in pos)) == limit + over
            assert all(p % planted.BLOCK >= 63 for p in pos)  # each window inside its block
    for count in (512, 513):
        data, cand, ref = tg.build_keep(count)
        assert np.count_nonzero(cand >= ref[-2]) == count
    for over in (0, 1):
        data, cand, ref = tg.build_capacity(over)
        assert cand.size == (data.size // (128 * KiB) * 3 // 2 + 1) * 2 + 8192 + over
        assert np.count_nonzero(cand >= ref[-2]) == 0  # nothing kept at the end


def test_synthetic_lists(oracle):
    lists = tg.synthetic_lists(oracle)
    assert len(lists["16382"][1]) + 2 == 16384 and len(lists["16383"][1]) + 2 == 16385
    _, mn, mx = planted.params(256)
    avg, cand, end = lists["forced-runs"]
    cuts = oracle.resolve(avg, np.asarray(cand, np.uint64), end)
    runs = np.diff(np.flatnonzero(np.diff(cuts.astype(np.int64)) != mx))
    assert runs.max() > 256
    assert lists["beyond-2^32"][1][-1] > 2**32


@pytest.mark.parametrize("cu", [1, 2, 4, 64, 256])
@pytest.mark.parametrize("knobs", [{}, {"PBS_SCAN_DYN": "1"}, {"PBS_SCAN_DYN": "1", "PBS_SCAN_SMALL": "0"},
                                   {"PBS_MAX_SEG": "8192"}, {"PBS_SCAN_DYN": "1", "PBS_MAX_SEG": "8192"}],
                         ids=["default", "dyn", "dyn-nosmall", "maxseg8k", "dyn-maxseg8k"])
def test_scan_main_plan_covers_the_batch(pbschunk, cu, knobs):
    """scan_main's plan (pbs_test_scan_main_plan): power-of-two segments, the tiles cover the
    batch up to the tail (less than one big tile), t_big <= ntiles, small tiles are a quarter."""
    rng = np.random.default_rng(11)
    sizes = [0, 1, 262143, 262144, 1 << 20, (1 << 20) + 77, 24 * MiB + 77, 32 * MiB + 77, 1 << 30,
             (8 << 30) + 12345, 64 << 30] + [int(x) for x in rng.integers(1, 70 << 30, 30)]
    with tg.env(knobs):
        for n in sizes:
            pl = pbschunk.plan_scan_main(n, cu)
            seg, nt, tb, dyn, cov = (pl[k] for k in ("seg", "ntiles", "t_big", "dyn", "covered"))
            assert seg in (4096, 8192, 16384, 32768) and seg <= int(knobs.get("PBS_MAX_SEG", 32768)) or seg == 4096
            assert tb <= nt and cov <= n and n - cov < 64 * seg, (n, pl)
            assert cov == tb * 64 * seg + (nt - tb) * 16 * seg
            if not dyn or knobs.get("PBS_SCAN_SMALL") == "0":
                assert tb == nt
            if nt:
                g = planted.scan_main_segments(pbschunk, n, cu) if n <= 64 * MiB else None
                assert g is None or (g["lanes"][0] == 0 and len(g["lanes"]) == 64 * nt)


@pytest.mark.parametrize("name", list(tg.T_CASES))
def test_threshold_inputs(oracle, name):
    """The solved window hashes to mask - 2 exactly (all 32 bits), and planted it is a
    candidate like any other (check() ran in the builder)."""
    avg = tg.T_CASES[name][1]
    w = planted.threshold_window(oracle, avg)
    assert oracle.window_hash(w, 63) == 2 * avg - 3
    data, pos, ref = tg.build_threshold(name)
    assert len(pos) >= 7 and all(oracle.window_hash(data, p) == 2 * avg - 3 for p in pos)
