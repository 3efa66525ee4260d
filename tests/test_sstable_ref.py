"""CPU: the Index / Summary reference itself (tests/sstable_ref.py).  The
literal restatement of makeIndexAndSummary produces a hand-computed case byte
for byte, equals the closed forms the device code uses on seeded cases, and its
images resolve every key through the restated readers."""
import itertools

import numpy as np
import pytest

from tests import sstable_ref as ref
from tests.sstable_ref import KeyContext

HAND_KEYS = [b"a", b"bb", b"ccc", b"d"]
HAND_SIZES = [40, 50, 60, 35]
HAND_PAGE = 2
HAND_INDEX = bytes.fromhex(
    "0100000000000000" "0000000000000000" "61"
    "0200000000000000" "2800000000000000" "6262"
    "0300000000000000" "5a00000000000000" "636363"
    "0100000000000000" "9600000000000000" "64")
HAND_SUMMARY = bytes.fromhex(
    "0100000000000000" "0100000000000000" "3500000000000000" "61" "64"
    "0100000000000000" "0000000000000000" "61"
    "0300000000000000" "2300000000000000" "636363"
    "0100000000000000" "3600000000000000" "64")

NS = (1, 2, 3, 4, 5, 7, 64, 65, 100)
PAGES = (1, 2, 3, 4, 64, 65, 1000)
KEY_LENGTHS = (0, 1, 3, 8, 9, 16, 40)


def literal(keys, sizes, page):
    return ref.make_index_and_summary([KeyContext(k, s) for k, s in zip(keys, sizes)], page)


def test_hand_case():
    assert len(HAND_INDEX) == 71 and len(HAND_SUMMARY) == 79
    index, summary = literal(HAND_KEYS, HAND_SIZES, HAND_PAGE)
    assert index == HAND_INDEX
    assert summary == HAND_SUMMARY
    assert ref.closed_index_and_summary(HAND_KEYS, HAND_SIZES, HAND_PAGE) == (HAND_INDEX, HAND_SUMMARY)
    assert ref.selected(4, 2) == [0, 2, 3]


def test_empty_and_single():
    for page in (0, 1, 3):
        assert literal([], [], page) == (b"", bytes(24))
        assert ref.closed_index_and_summary([], [], page) == (b"", bytes(24))
        index, summary = literal([b"key"], [77], page)
        assert index == (3).to_bytes(8, "little") + bytes(8) + b"key"
        # MinKey = MaxKey = the one key; one entry at Index offset 0
        assert summary == ((3).to_bytes(8, "little") * 2 + (19).to_bytes(8, "little") + b"keykey"
                           + (3).to_bytes(8, "little") + bytes(8) + b"key")
        assert ref.closed_index_and_summary([b"key"], [77], page) == (index, summary)
    # the empty key alone: header of 24 bytes with Payload 16, one 16-byte entry
    assert literal([b""], [30], 3) == (bytes(16), bytes(16) + (16).to_bytes(8, "little") + bytes(16))


def test_page_zero_divides_by_zero_from_the_second_record():
    with pytest.raises(ZeroDivisionError):
        literal([b"a", b"b"], [31, 31], 0)


def seeded_case(seed):
    rng = np.random.default_rng(0x5354 + seed)
    n = int(rng.choice(NS))
    page = int(rng.choice(PAGES))
    keys = [bytes(rng.integers(0, 256, int(rng.choice(KEY_LENGTHS)), dtype=np.uint8)) for _ in range(n)]
    sizes = [30 + len(k) + int(rng.integers(0, 201)) for k in keys]
    return keys, sizes, page


def test_literal_equals_closed_form_on_seeded_cases():
    seen_n, seen_page = set(), set()
    for seed in range(2200):
        keys, sizes, page = seeded_case(seed)
        seen_n.add(len(keys))
        seen_page.add(page)
        index, summary = literal(keys, sizes, page)
        assert (index, summary) == ref.closed_index_and_summary(keys, sizes, page), seed
        assert len(index) == 16 * len(keys) + sum(map(len, keys))
        m = ref.summary_entries(len(keys), page)
        payload = int.from_bytes(summary[16:24], "little")
        assert len(summary) == 24 + len(keys[0]) + len(keys[-1]) + payload
        assert payload == sum(16 + len(keys[i]) for i in ref.selected(len(keys), page)) and len(ref.selected(len(keys), page)) == m
    assert seen_n == set(NS) and seen_page == set(PAGES)


def test_entry_count_on_the_whole_grid():
    for n, page in itertools.product(range(0, 140), list(range(1, 70)) + [1000]):
        want = sorted({i for i in range(n) if i == 0 or i % page == 0 or i == n - 1})
        assert ref.selected(n, page) == want
        assert ref.summary_entries(n, page) == len(want)


def sorted_table(rng, n):
    """n distinct sorted keys (the empty key sometimes among them) and RecSizes."""
    keys = set()
    if rng.random() < 0.3:
        keys.add(b"")
    while len(keys) < n:
        keys.add(bytes(rng.integers(97, 101, int(rng.integers(1, 6)), dtype=np.uint8)))
    keys = sorted(keys)
    return keys, [30 + len(k) + int(rng.integers(0, 201)) for k in keys]


@pytest.mark.parametrize("seed", range(40))
def test_readers_resolve_every_key(seed):
    rng = np.random.default_rng(0x7264 + seed)
    n = int(rng.choice((1, 2, 3, 4, 5, 7, 64, 65, 100)))
    page = int(rng.choice((1, 2, 3, 4, 64, 65, 1000)))
    keys, sizes = sorted_table(rng, n)
    index, summary = literal(keys, sizes, page)
    off = np.concatenate(([0], np.cumsum(sizes)[:-1])).tolist()
    for k, o in zip(keys, off):
        assert ref.lookup(index, summary, k) == o
    present = set(keys)
    absent = [bytes(rng.integers(97, 102, int(rng.integers(0, 7)), dtype=np.uint8)) for _ in range(60)]
    absent += [keys[0][:-1] if keys[0] else b"", keys[-1] + b"\x00", b"\xff" * 3]
    summary_says = index_says = 0
    for k in absent:
        if k in present:
            continue
        ste = ref.find_summary_table_entry(summary, k)
        if ste.Offset == -1:
            summary_says += 1
            assert k < keys[0] or k > keys[-1]
        else:
            assert ref.find_index_table_entry(index, k, ste.Offset).Offset == -1
            index_says += 1
        assert ref.lookup(index, summary, k) == -1
    assert summary_says >= 1  # keys[-1] + b"\0" lies past MaxKey


def test_good_ste_lags_one_entry_behind():
    """The returned entry is the one before the first entry whose key is >= the
    wanted key; for the first key itself that is the zero entry (Offset 0)."""
    keys = [b"b", b"d", b"f", b"h", b"j"]
    index, summary = literal(keys, [31] * 5, 2)  # entries for b, f, j at Index offsets 0, 34, 68
    got = [ref.find_summary_table_entry(summary, k) for k in (b"b", b"c", b"f", b"g", b"j")]
    assert [(e.Offset, e.Key) for e in got] == [(0, b""), (0, b"b"), (0, b"b"), (34, b"f"), (34, b"f")]
    assert ref.find_summary_table_entry(summary, b"a").Offset == -1
    assert ref.find_summary_table_entry(summary, b"k").Offset == -1
