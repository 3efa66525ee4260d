"""CPU: the live memtable's two restatements (tests/live_memtable_ref.py) agree
on seeded logs, and the hand cases pin what the reference's Add / ShouldFlush /
Find do where a plausible reading would differ."""
import numpy as np
import pytest

from nakevaleng_amd import record
from tests import live_memtable_ref as ref

CAP, THR, BOTH = ref.FLUSH_CAPACITY, ref.FLUSH_THRESHOLD, ref.FLUSH_CAPACITY | ref.FLUSH_THRESHOLD


def rec(key, value, status=0, ts=1):
    r = record.New(key, value, ts)
    r.Status = status
    return r


def seeded_log(seed, n, distinct):
    rng = np.random.default_rng(seed)
    keys = [rng.integers(0, 256, int(rng.integers(0, 12)), dtype=np.uint8).tobytes() for _ in range(distinct)]
    return [rec(keys[int(rng.integers(0, distinct))], bytes(int(rng.integers(0, 60))), int(rng.integers(0, 2)), i)
            for i in range(n)]


@pytest.mark.parametrize("seed,n,distinct", [(1, 1, 1), (2, 40, 5), (3, 300, 300), (4, 300, 17), (5, 257, 1)])
@pytest.mark.parametrize("strategy", [0, CAP, THR, BOTH])
def test_literal_equals_closed(seed, n, distinct, strategy):
    log = seeded_log(seed, n, distinct)
    for capacity, threshold in ((10, 2000), (3, 100), (1000, 10**9)):
        assert ref.add_literal(log, strategy, capacity, threshold) == ref.add_closed(log, strategy, capacity, threshold)
    keys = sorted({r.Key for r in log}) + [b"\xff" * 13, b"absent"]
    found = ref.find_literal(log, keys)
    hit, status = ref.find_closed(log, keys)
    for k, f, h, s in zip(keys, found, hit, status):
        if f is None:
            assert (h, s) == (ref.NONE, ref.ABSENT)
        else:
            assert f is log[h] and f.Key == k and s == (ref.TOMBSTONE if f.IsDeleted() else ref.LIVE)


def test_overwrite_leaves_memusage_where_it_was():
    first = rec(b"k", b"v" * 10)
    for other in (rec(b"k", b"v" * 500), rec(b"k", b"")):  # a longer record, a shorter one
        t = ref.add_literal([first, other], 0, 10, 2000)
        assert t.is_new == [True, False]
        assert t.count == [1, 1]
        assert t.memusage == [first.TotalSize()] * 2
        assert t == ref.add_closed([first, other], 0, 10, 2000)


def test_capacity_fires_at_equality_only():
    log = [rec(bytes([i]), b"") for i in range(5)]
    t = ref.add_literal(log, CAP, 3, 0)
    assert t.should_flush == [False, False, True, False, False]  # above the capacity: never again
    assert t.flush_at() == 2 and t.flush_at(3) == ref.NONE
    # an overwrite at the capacity still finds Count == capacity
    t = ref.add_literal(log[:3] + [rec(bytes([0]), b"x")], CAP, 3, 0)
    assert t.should_flush == [False, False, True, True] and t.flush_at(3) == 3


def test_threshold_only_both_and_neither():
    log = [rec(bytes([i]), b"v" * 70) for i in range(6)]  # 101 bytes each
    t = ref.add_literal(log, THR, 2, 250)
    assert t.should_flush == [False, False, True, True, True, True] and t.flush_at() == 2
    t = ref.add_literal(log, BOTH, 2, 450)
    assert t.should_flush == [False, True, False, False, True, True] and t.flush_at() == 1 and t.flush_at(2) == 4
    t = ref.add_literal(log, 0, 2, 250)
    assert not any(t.should_flush) and t.flush_at() == ref.NONE
    for strategy in (0, CAP, THR, BOTH):
        assert ref.add_literal(log, strategy, 2, 250) == ref.add_closed(log, strategy, 2, 250)


def test_find_returns_the_latest_write_tombstones_included():
    log = [rec(b"a", b"1", ts=9), rec(b"b", b"2"), rec(b"a", b"", status=1, ts=3), rec(b"b", b"3", ts=0),
           rec(b"c", b"x", status=1), rec(b"c", b"y")]
    a, b, c, d = ref.find_literal(log, [b"a", b"b", b"c", b"d"])
    assert a is log[2] and a.IsDeleted()  # a tombstone as the latest write, older Timestamp and all
    assert b is log[3] and c is log[5] and not c.IsDeleted() and d is None
    assert ref.find_closed(log, [b"a", b"b", b"c", b"d"], 31) == (
        [(31 << 32) | 2, (31 << 32) | 3, (31 << 32) | 5, ref.NONE], [ref.TOMBSTONE, ref.LIVE, ref.LIVE, ref.ABSENT])
    assert ref.get_model(log, [], b"a") == (ref.TOMBSTONE, None)
    assert ref.get_model(log, [], b"b") == (ref.LIVE, b"3")
    assert ref.get_model(log, [], b"d") == (ref.ABSENT, None)
