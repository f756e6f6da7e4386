"""The digest constructor of tests/_dedup.py (no GPU): the collision tests rely on it to put digests on chosen slots
of the device set, so its geometry is checked here against the table's home formula at every capacity."""
import numpy as np

from _dedup import (LAST, adjacent_homes, capacity_after, capacity_for, digest, digests, home_of, near_misses,
                    same_home, tag01, tag_of, walk, wrap)

CAPACITIES = [1 << b for b in range(10, 32)]
TAGS = [0, 1, 2, 0x1F2E3D4C5B6A7988, (1 << 64) - 1, 1 << 63, 0x20000]


def _home(d, capacity):
    """(d[1] ^ (d[0] >> 17)) & (capacity - 1), restated from the little-endian bytes."""
    w0 = int.from_bytes(bytes(d[0:8]), "little")
    w1 = int.from_bytes(bytes(d[8:16]), "little")
    return (w1 ^ (w0 >> 17)) & (capacity - 1)


def test_digest_home_at_every_capacity():
    for t in TAGS:
        for h in (0, 1, 2, 511, 1000, 1023, LAST):
            d = digest(t, h, 12345)
            assert d.dtype == np.uint8 and d.shape == (32,)
            assert int.from_bytes(bytes(d[0:8]), "little") == t
            for c in CAPACITIES:
                assert _home(d, c) == home_of(d, c) == (c - 1 if h == LAST else h), (t, h, c)


def test_digest_tags_salts_and_families():
    assert tag_of(digest(0, 5, 1)) == tag_of(digest(1, 5, 2)) == 1
    assert digest(7, 3, 9).tobytes() == digest(7, 3, 9).tobytes()
    f = same_home(7, 3, 50, 0)
    assert len({r.tobytes() for r in f}) == 50 and {tag_of(r) for r in f} == {7}
    assert {home_of(r, 1 << 20) for r in f} == {3}
    g = adjacent_homes(7, 100, 4, 12, 0)
    assert sorted({home_of(r, 1024) for r in g}) == [100, 101, 102, 103] and len({r.tobytes() for r in g}) == 12
    t = tag01(40, 6, 0)
    assert [int.from_bytes(bytes(r[:8]), "little") for r in t] == [0, 1] * 3
    assert {tag_of(r) for r in t} == {1} and {home_of(r, 1 << 31) for r in t} == {40}
    w = wrap(9, 3, 0, spill=2)
    assert [home_of(r, 4096) for r in w] == [4095, 4095, 4095, 0, 1]
    assert np.array_equal(digests([5, 6], [1, 2], [3, 4])[1], digest(6, 2, 4))


def test_near_misses_keep_tag_and_home_and_differ():
    d = np.concatenate([same_home(0x1F2E3D4C5B6A7988, 17, 4, 0), wrap(3, 2, 0)])
    nm = near_misses(d)
    assert len(nm) == 3 * len(d)
    for i, r in enumerate(nm):
        src = d[i // 3]
        assert tag_of(r) == tag_of(src) and r.tobytes() != src.tobytes()
        assert all(home_of(r, c) == home_of(src, c) for c in CAPACITIES)
        assert int(np.count_nonzero(r != src)) == 1


def test_walk_and_capacity_rule():
    a, b = digest(1, 1, 1), digest(1, 1, 2)
    store = set()
    assert walk(store, np.stack([a, b, a, b])).tolist() == [True, True, False, False]
    assert walk(store, np.stack([b, digest(1, 1, 3)])).tolist() == [False, True]
    assert capacity_for(0) == 1024 and capacity_for(512) == 1024 and capacity_for(513) == 2048
    assert capacity_for(1 << 40) == 1 << 31
    assert capacity_after(1024, 0, 512) == 1024 and capacity_after(1024, 500, 13) == 4096
