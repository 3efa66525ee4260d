"""CPU: the two restatements of the memtable flush (tests/memtable_ref.py)
against hand-derived expectations, then against each other on a seeded fuzz."""
import numpy as np
import pytest

from nakevaleng_amd import record
from tests.memtable_ref import flush_closed, flush_literal


def rec(key: bytes, ts: int = 0, val: bytes = b"v", tomb: bool = False, status: int = None,
        typeinfo: int = 0) -> record.Record:
    r = record.New(key, val, timestamp=ts)
    if tomb:
        r.Status = record.RECORD_TOMBSTONE_REMOVED
    if status is not None:
        r.Status = status
    r.TypeInfo = typeinfo
    return r


K8 = b"abcdefgh"

# name -> (log in arrival order, expected arrival index of every output record), derived by hand
HAND_CASES = {
    "one": ([rec(b"k")], [0]),
    "two_sorted": ([rec(b"a"), rec(b"b")], [0, 1]),
    "two_reversed": ([rec(b"b"), rec(b"a")], [1, 0]),
    "overwrite": ([rec(b"k", 1, b"old"), rec(b"k", 2, b"new")], [1]),
    # the empty key is smallest
    "empty_key": ([rec(b"a"), rec(b""), rec(b"\x00")], [1, 2, 0]),
    "empty_key_twice": ([rec(b"", 1, b"x"), rec(b"a"), rec(b"", 2, b"y")], [2, 1]),
    # a proper prefix sorts first
    "a_aa_aaa": ([rec(b"aaa"), rec(b"a"), rec(b"aa")], [1, 2, 0]),
    # the zero-padded prefixes of "abc" and "abc\0" are equal: the lengths decide
    "abc_abc0": ([rec(b"abc\x00"), rec(b"abc")], [1, 0]),
    "abc_abc0_dup": ([rec(b"abc\x00", 1), rec(b"abc", 1), rec(b"abc\x00", 2), rec(b"abc", 0)], [3, 2]),
    # an 8-byte key against itself plus \0 and plus \x01
    "k8_k8_0": ([rec(K8 + b"\x00"), rec(K8)], [1, 0]),
    "k8_k8_1": ([rec(K8 + b"\x01"), rec(K8 + b"\x00"), rec(K8)], [2, 1, 0]),
    "k8_tails": ([rec(K8 + b"\x01\x00"), rec(K8 + b"\x01"), rec(K8 + b"\x00\xff"), rec(K8), rec(K8 + b"\x01")],
                 [3, 2, 4, 0]),
    # unsigned bytes: 0x7f < 0x80 < 0xff, in the dense prefix and behind it
    "high_bytes": ([rec(b"\x80"), rec(b"\x7f\xff"), rec(b"\xff"), rec(b"\x7f")], [3, 1, 0, 2]),
    "high_bytes_tail": ([rec(K8 + b"x\x80"), rec(K8 + b"x\x7f"), rec(K8 + b"x\xff"), rec(K8 + b"x")], [3, 1, 0, 2]),
    # the rule: the last arrival wins whatever its Timestamp
    "older_timestamp_wins": ([rec(b"k", 9, b"first"), rec(b"k", 3, b"second")], [1]),
    "negative_timestamp_wins": ([rec(b"k", 0, b"first"), rec(b"k", -5, b"second")], [1]),
    "tombstone_shadows_live": ([rec(b"k", 1, b"live"), rec(b"k", 2, b"", tomb=True)], [1]),
    "live_shadows_tombstone": ([rec(b"k", 1, b"", tomb=True), rec(b"j"), rec(b"k", 2, b"back")], [1, 2]),
    "status_and_typeinfo": ([rec(b"b", 1, b"x", status=0xFE, typeinfo=0x7B), rec(b"a", 1, b"y", status=0x81, typeinfo=0xFF),
                             rec(b"b", 1, b"z", status=0x55, typeinfo=0xAA)], [1, 2]),
    "all_same_key": ([rec(b"k", t, bytes([t])) for t in range(7)], [6]),
}


@pytest.mark.parametrize("flush", [flush_literal, flush_closed], ids=["literal", "closed"])
@pytest.mark.parametrize("name", sorted(HAND_CASES))
def test_hand_cases(flush, name):
    log, want = HAND_CASES[name]
    out, src = flush(log)
    assert src == want
    assert all(x is log[i] for x, i in zip(out, want))
    assert [r.Key for r in out] == sorted({r.Key for r in log})


def test_status_and_typeinfo_come_through():
    log, _ = HAND_CASES["status_and_typeinfo"]
    out, _ = flush_closed(log)
    assert [(r.Status, r.TypeInfo, r.Value) for r in out] == [(0x81, 0xFF, b"y"), (0x55, 0xAA, b"z")]
    assert out[1].ToBytes()[12:14] == b"\x55\xaa"


def fuzz_log(rng, nmax=200):
    """Up to nmax writes over a pool of at most n/3 keys of 0..11 bytes over a
    3-letter alphabet (plus 0x00 and 0xFF), so most keys repeat and many share
    padded prefixes; a tenth are tombstones; Timestamps in any order."""
    n = int(rng.integers(0, nmax + 1))
    alphabet = [0x00, 0x61, 0x62, 0x63, 0xFF]
    pool = [bytes(rng.choice(alphabet, int(rng.integers(0, 12))).tolist()) for _ in range(max(1, n // 3))]
    return [rec(pool[int(rng.integers(0, len(pool)))], int(rng.integers(-2, 3)), rng.bytes(int(rng.integers(0, 4))),
                tomb=bool(rng.random() < 0.1)) for _ in range(n)]


def test_literal_equals_closed_fuzz():
    rng = np.random.default_rng(0x6D656D74)
    repeats = 0
    for case in range(3000):
        log = fuzz_log(rng)
        a, b = flush_literal(log), flush_closed(log)
        assert a[1] == b[1], (case, [(r.Key, r.Timestamp) for r in log])
        assert all(x is y for x, y in zip(a[0], b[0]))
        repeats += len(log) - len(a[1])
    assert repeats > 100000  # most writes hit a key that is written again
