"""CPU: the two restatements of compaction's merge (tests/merge_ref.py) against
hand-derived expectations, then against each other on a seeded fuzz; and the
argument checks of lsmtree.merge that need no device."""
import numpy as np
import pytest

from nakevaleng_amd import record
from tests.merge_ref import merge_closed, merge_literal


def rec(key: bytes, ts: int = 0, val: bytes = b"v", tomb: bool = False) -> record.Record:
    r = record.New(key, val, timestamp=ts)
    if tomb:
        r.Status = record.RECORD_TOMBSTONE_REMOVED
    return r


# name -> (runs, expected (run, index) of every output record), derived by hand
HAND_CASES = {
    # a < b < c < d < e, alternating between the runs
    "interleaved": ([[rec(b"a"), rec(b"c"), rec(b"e")], [rec(b"b"), rec(b"d")]],
                    [(0, 0), (1, 0), (0, 1), (1, 1), (0, 2)]),
    # b is in both runs; run 0 holds the later one; run 1's c still comes out
    "newer_in_run0": ([[rec(b"a", 1), rec(b"b", 5), rec(b"d", 1)], [rec(b"b", 3), rec(b"c", 1)]],
                      [(0, 0), (0, 1), (1, 1), (0, 2)]),
    # the same with the runs swapped: the later b is in run 1
    "newer_in_run1": ([[rec(b"b", 3), rec(b"c", 1)], [rec(b"a", 1), rec(b"b", 5), rec(b"d", 1)]],
                      [(1, 0), (1, 1), (0, 1), (1, 2)]),
    # the newest record of k is a tombstone: it wins and stays
    "tombstone": ([[rec(b"k", 1, b"live")], [rec(b"k", 2, b"", tomb=True)]], [(1, 0)]),
    # tie on the first record of both runs: both entered the queue at the start, run 0 first
    "tie_first": ([[rec(b"a", 1, b"x")], [rec(b"a", 1, b"y")]], [(0, 0)]),
    # tie on k; run 1's k entered the queue when a was consumed, run 0's only when c was
    "tie_pred": ([[rec(b"c", 0), rec(b"k", 1, b"x")], [rec(b"a", 0), rec(b"k", 1, b"y")]],
                 [(1, 0), (0, 0), (1, 1)]),
    # three-way tie on k; run 1's k has no predecessor, so it was in the queue from the start
    "tie3_first": ([[rec(b"b", 0), rec(b"k", 1)], [rec(b"k", 1)], [rec(b"a", 0), rec(b"k", 1)]],
                   [(2, 0), (0, 0), (1, 0)]),
    # three-way tie on k, predecessors c, a, b: run 1's k entered first
    "tie3_pred": ([[rec(b"c", 0), rec(b"k", 1)], [rec(b"a", 0), rec(b"k", 1)], [rec(b"b", 0), rec(b"k", 1)]],
                  [(1, 0), (2, 0), (0, 0), (1, 1)]),
    # bytes.Compare: "" < "a" < "a\0" < "ab" < "\x80" (unsigned, a proper prefix first)
    "key_order": ([[rec(b""), rec(b"a\x00"), rec(b"\x80")], [rec(b"a"), rec(b"ab")]],
                  [(0, 0), (1, 0), (0, 1), (1, 1), (0, 2)]),
    # Timestamp is signed: -1 is older than 0
    "negative_ts": ([[rec(b"k", -1)], [rec(b"k", 0)]], [(1, 0)]),
    "empty_run": ([[rec(b"a")], [], [rec(b"b")]], [(0, 0), (2, 0)]),
    "all_empty": ([[], []], []),
    "k1_identity": ([[rec(b"a", 3), rec(b"b", -7, tomb=True), rec(b"c", 0, b"")]], [(0, 0), (0, 1), (0, 2)]),
}


@pytest.mark.parametrize("merge", [merge_literal, merge_closed], ids=["literal", "closed"])
@pytest.mark.parametrize("name", sorted(HAND_CASES))
def test_hand_cases(merge, name):
    runs, want = HAND_CASES[name]
    out, src = merge(runs)
    assert src == want
    assert [r.ToBytes() for r in out] == [runs[r][i].ToBytes() for r, i in want]


def test_tombstone_is_kept_as_written():
    out, _ = merge_closed(HAND_CASES["tombstone"][0])
    assert len(out) == 1 and out[0].IsDeleted() and out[0].Value == b""


def test_tie_is_not_lowest_run_and_not_input_order():
    """In tie_pred the lower run loses; with the predecessors swapped it wins."""
    runs = [[rec(b"a", 0), rec(b"k", 1)], [rec(b"c", 0), rec(b"k", 1)]]
    for merge in (merge_literal, merge_closed):
        assert merge(runs)[1] == [(0, 0), (1, 0), (0, 1)]


def fuzz_runs(rng, k, nkeys=6, nts=3):
    keys = [bytes([97 + j]) for j in range(nkeys)]
    runs = []
    for _ in range(k):
        mine = [key for key in keys if rng.random() < 0.6]
        runs.append([rec(key, int(rng.integers(0, nts)), b"") for key in mine])
    return runs


def test_literal_equals_closed_fuzz():
    rng = np.random.default_rng(0x6D65726765)
    for case in range(6000):
        k = 1 + case % 6
        runs = fuzz_runs(rng, k)
        a, b = merge_literal(runs), merge_closed(runs)
        assert a[1] == b[1], (case, [[(r.Key, r.Timestamp) for r in run] for run in runs])
        assert all(x is y for x, y in zip(a[0], b[0]))


def test_lsmtree_merge_refuses_bad_arguments_without_a_device():
    """k outside 1..16 is refused before any device work (NKV_ERR_INVALID)."""
    from nakevaleng_amd import lsmtree
    with pytest.raises(ValueError):
        lsmtree.merge([])
    with pytest.raises(ValueError):
        lsmtree.merge([record.data_table([rec(b"a")])] * 17)
