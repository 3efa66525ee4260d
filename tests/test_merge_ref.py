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
    # around the dense 8-byte prefix of the device's key comparison: "abcdefg" and "abcdefg\0" have
    # the same zero-padded prefix and differ in length only; "abcdefgh" follows both; the later
    # "abcdefgh" is in run 1
    "prefix_7_8": ([[rec(b"abcdefg", 0), rec(b"abcdefgh", 1)], [rec(b"abcdefg\x00", 0), rec(b"abcdefgh", 2)]],
                   [(0, 0), (1, 0), (1, 1)]),
    # an 8-byte key sorts before the same 8 bytes followed by \0 (a proper prefix first)
    "prefix_8_9": ([[rec(b"abcdefgh\x00", 5)], [rec(b"abcdefgh", 1)]], [(1, 0), (0, 0)]),
    # a 10-byte key in both runs, tied on Timestamp: run 1's entered the queue when "abcdefghia"
    # was consumed, run 0's only when "abcdefghib" was; the predecessors differ in byte 10 alone
    "tie_pred_long": ([[rec(b"abcdefghib", 0), rec(b"abcdefghik", 1, b"x")],
                       [rec(b"abcdefghia", 0), rec(b"abcdefghik", 1, b"y")]],
                      [(1, 0), (0, 0), (1, 1)]),
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


BOUNDARY_SEEDS = 12
BOUNDARY_K = [2, 3, 4, 6, 16, 1]


def boundary_pool(rng):
    """61 keys over {0x00, 'a', 0xFF} around byte 8, where the device's key
    comparison (cmp_key) switches from its dense zero-padded 8-byte prefix to
    the lengths or the remaining bytes: every prefix of a random 8-byte stem,
    the stem followed by every tail of 0..3 bytes, and a second stem that
    differs in byte 8 only, followed by every tail of 0..2 bytes."""
    alphabet = [0x00, 0x61, 0xFF]
    stem = bytes(rng.choice(alphabet, 8).tolist())
    other = stem[:7] + bytes([alphabet[(alphabet.index(stem[7]) + 1 + int(rng.integers(0, 2))) % 3]])

    def tails(upto):
        out = [b""]
        for _ in range(upto):
            out += [t + bytes([c]) for t in out if len(t) == len(out[-1]) for c in alphabet]
        return out

    pool = {stem[:j] for j in range(9)} | {stem + t for t in tails(3)} | {other + t for t in tails(2)}
    assert len(pool) == 61
    return sorted(pool)


def boundary_runs(seed):
    """(k, runs) of the prefix-boundary fuzz: each run a random subset of
    boundary_pool with Timestamps in {-1, 0, 1} and values of 0..39 bytes."""
    rng = np.random.default_rng(0xB0DA + seed)
    k = BOUNDARY_K[seed % len(BOUNDARY_K)]
    pool = boundary_pool(rng)
    runs = []
    for _ in range(k):
        pick = sorted(rng.choice(len(pool), int(rng.integers(1, len(pool) + 1)), replace=False).tolist())
        runs.append([rec(pool[j], int(rng.integers(-1, 2)), rng.bytes(int(rng.integers(0, 40)))) for j in pick])
    return k, runs


def boundary_coverage(runs):
    """What a case holds of the comparisons the fuzz is for: pairs of distinct
    keys with equal zero-padded 8-byte prefixes where one key has at most 8
    bytes / where both are longer; keys in more than one run; of those, keys
    whose greatest Timestamp occurs more than once."""
    keys = sorted({r.Key for run in runs for r in run})
    pad = lambda key: key[:8].ljust(8, b"\0")
    short = long_ = 0
    for i, a in enumerate(keys):
        for b in keys[i + 1:]:
            if pad(a) == pad(b):
                if min(len(a), len(b)) <= 8:
                    short += 1
                else:
                    long_ += 1
    ts = {}
    for run in runs:
        for r in run:
            ts.setdefault(r.Key, []).append(r.Timestamp)
    dup = [v for v in ts.values() if len(v) > 1]
    return short, long_, len(dup), sum(v.count(max(v)) > 1 for v in dup)


def boundary_case(seed):
    """The runs of one seed, after the CPU-side checks every seed must pass:
    the two restatements agree wherever the reference's result is pinned
    (k <= 6), and the comparisons the case is for are present."""
    k, runs = boundary_runs(seed)
    assert all(a.Key < b.Key for run in runs for a, b in zip(run, run[1:]))
    if k <= 6:
        assert merge_literal(runs)[1] == merge_closed(runs)[1]
    return k, runs


def test_prefix_boundary_fuzz_covers_its_cases():
    """A generator change cannot silently drop the cases: over the 12 seeds at
    least 100 key pairs with equal padded prefixes of each sort, and keys that
    tie across runs."""
    total = np.zeros(4, np.int64)
    for seed in range(BOUNDARY_SEEDS):
        k, runs = boundary_case(seed)
        assert len(runs) == k
        total += boundary_coverage(runs)
    short, long_, dup, tied = total.tolist()
    print(f"prefix-boundary fuzz: {short} short pairs, {long_} long pairs, {dup} keys in several runs, {tied} tied")
    assert short >= 100 and long_ >= 100
    assert dup >= 100 and tied >= 50


def test_lsmtree_merge_refuses_bad_arguments_without_a_device():
    """k outside 1..16 is refused before any device work (NKV_ERR_INVALID)."""
    from nakevaleng_amd import lsmtree
    with pytest.raises(ValueError):
        lsmtree.merge([])
    with pytest.raises(ValueError):
        lsmtree.merge([record.data_table([rec(b"a")])] * 17)
