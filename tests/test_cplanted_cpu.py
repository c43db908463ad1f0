"""CPU: the inputs of tests/test_gpu_cplanted.py put the copy kernel's items where cplanted.py
says.  Nothing of the library runs here: this is a condition on the planted stream and on the
pad pairs, so that a change of either cannot quietly thin out what the GPU test shows."""
import cplanted as c
import dplanted as d


def test_stream_is_the_planted_one(oracle):
    items = c.items(oracle)
    assert tuple(len(it.payload) for it in items) == c.PLENS and tuple(it.kind for it in items) == c.PKINDS
    assert sorted(n for i, n in enumerate(c.PLENS) if i != c.BAD_AT) == sorted(
        (0, 1, 15, 16, 17, 31, 32, 33, 65535, 65536, 65537, 65536 + 15, 65536 + 16, 2 * 65536 + 5))
    assert {0, 2} == set(c.PKINDS) and all(0 not in it.payload for i, it in enumerate(items) if i != c.BAD_AT)
    bad = items[c.BAD_AT]
    assert 0 < c.BAD_AT < len(items) - 1 and [it.status for it in items] == [
        d.BAD_TAG if i == c.BAD_AT else d.OK for i in range(len(items))]
    assert d.reference_outcome(oracle, bad, c.g.KEY1)[0] == d.BAD_TAG and not any(bad.payload)
    # the largest buffer of a call: the blob stream, and the roomier slots
    assert sum(len(it.blob) for it in items) + 64 < 1 << 20 and sum(c.slot_sizes("roomy")) + 512 < 1 << 20
    assert c.PKINDS[c.SHORT_AT] == 0 and c.slot_sizes("short")[c.SHORT_AT] == c.PLENS[c.SHORT_AT] - c.SHORT_BY


def test_items_follow_the_kernel_contract():
    for ip, op in c.PADS:
        for src, dst, n in c.segments(ip, op):
            its = c.copy_items(src, dst, n)
            assert sum(m for _, _, m in its) == n and all(0 < m <= c.PIECE + 15 for _, _, m in its)
            assert all(t % 16 == 0 for _, t, _ in its[1:]), "a later piece starts off a boundary"
            assert all(a[0] + a[2] == b[0] and a[1] + a[2] == b[1] for a, b in zip(its, its[1:]))


def test_pad_pairs_show_every_alignment():
    """Over the pad pairs of the GPU test the kernel's items of 16 bytes and more show every
    (source - destination) difference mod 16 at every destination residue, each both with and
    without tail bytes after the last 16-byte store; the shorter items show every length 1..15."""
    t = c.triples()
    assert len(c.PADS) == 128 and set(c.triples(c.PADS[:1])) < t
    shown = {((s - dst) % 16, dst, c.tail_of(m, dst) != 0) for m, s, dst in t if m >= 16}
    assert shown == {(diff, dst, tail) for diff in range(16) for dst in range(16) for tail in (False, True)}
    assert {m for m, _, _ in t if m < 16} == set(range(1, 16))
    # head bytes: a destination off the boundary, and an item that ends before reaching it
    assert any(m < 16 and dst and m < 16 - dst for m, _, dst in t)
