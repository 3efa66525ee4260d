"""CPU: the literal restatement of the engine's disk read path
(tests/lookup_ref.get over sstable_ref's readers) equals the closed form the
device code computes (tests/lookup_ref.closed_get) on strictly increasing
tables, at the places where the reference's lagging goodSte could matter."""
import numpy as np
import pytest

from nakevaleng_amd import record
from tests import lookup_ref as ref

NS = (1, 2, 3, 5, 64, 65, 200)
PAGES = (1, 2, 3, 64)
# crafted keys: the empty key, proper prefixes of each other, keys longer than
# 8 bytes that share their first 8, bytes >= 0x80 (the compare is unsigned)
CRAFTED = [b"", b"a", b"ab", b"abc", b"abcdefgh", b"abcdefghA", b"abcdefghB", b"abcdefghBA", b"abcdefgh\x00",
           b"abcdefgh\xff", b"\x7f", b"\x80", b"\x80\x00", b"\xff", b"\xff\xff", b"\xfe\xff\x80", b"a\x00", b"a\x80",
           b"prefix-of-eight-and-more", b"prefix-of-eight-and-most", b"prefix-o"]


def keys_for(rng, n, with_empty):
    pool = set(CRAFTED if with_empty else CRAFTED[1:])
    while len(pool) < n + 8:
        ln = int(rng.integers(1, 41))
        head = bytes(rng.choice([0x00, 0x61, 0x7f, 0x80, 0xff], min(ln, int(rng.integers(0, 10)))).astype(np.uint8))
        pool.add(head + bytes(rng.integers(0, 256, ln - len(head), dtype=np.uint8)))
    keys = sorted(pool)
    pick = sorted(rng.choice(len(keys), n, replace=False).tolist())
    if with_empty:
        pick[0] = 0  # b"" sorts first
    return [keys[i] for i in sorted(set(pick))]


def below(key):
    """A key just below `key` (None for the empty key, which has none)."""
    if not key:
        return None
    return key[:-1] if key[-1] == 0 else key[:-1] + bytes([key[-1] - 1]) + b"\xff" * 3


def queries_for(keys):
    """Every stored key (so MinKey, MaxKey and every Summary entry's key), one
    past each (key + 0x00 is the next byte string), a proper prefix of each,
    just below each, the neighbours of Min and Max, and the empty key."""
    out = [b""]
    for k in keys:
        out += [k, k + b"\x00", k + b"\xff", k[:-1], k[:8]]
        if below(k) is not None:
            out.append(below(k))
    out += [keys[-1] + b"\x00", keys[-1] + b"\x01", b"\xff" * 41]
    return list(dict.fromkeys(out))


def table(rng, keys, page, filt=None, tombstones=()):
    recs = []
    for i, k in enumerate(keys):
        r = record.New(k, bytes(rng.integers(0, 256, int(rng.integers(0, 20)), dtype=np.uint8)), 7)
        if i in tombstones:
            r.Status |= record.RECORD_TOMBSTONE_REMOVED
        recs.append(r)
    stream, sizes = record.data_table(recs)
    return ref.table_of(stream, sizes, page, filt)


@pytest.mark.parametrize("page", PAGES)
@pytest.mark.parametrize("n", NS)
def test_restatement_equals_closed_form_on_one_table(n, page):
    for with_empty in (False, True):
        rng = np.random.default_rng(0x6C6B + 131 * n + page + (1 << 12) * with_empty)
        keys = keys_for(rng, n, with_empty)
        assert keys == sorted(set(keys)) and (keys[0] == b"") == with_empty
        tab = table(rng, keys, page)
        stages = set()
        qs = queries_for(keys)
        for q in qs:
            got, want = ref.get([tab], q), ref.closed_get([tab], q)
            assert got == want, (n, page, q)
            assert (got.status != ref.ABSENT) == (q in keys)
            stages.add(got.stages[0])
        assert ref.FOUND in stages and ref.SUMMARY in stages
        assert (ref.INDEX in stages) == any(keys[0] < q < keys[-1] and q not in keys for q in qs)
        assert ref.INDEX in stages or n < 3


def test_restatement_equals_closed_form_over_several_tables(oracle):
    """Three tables with overlapping keys, tombstones, and filters small enough
    that absent keys pass them: every stage occurs, the first table in order
    wins, and a tombstone hides a later live record."""
    rng = np.random.default_rng(0x6C6D)
    pool = keys_for(rng, 90, True)
    seen = set()
    for page in (1, 3):
        tabs = []
        for t in range(3):
            keys = [k for i, k in enumerate(pool) if (i + t) % 3 != 0 and 10 * t <= i < 70 + 10 * t]
            other = [k for k in pool if k not in keys]
            filt = [ref.filter_of(keys, 64, 2, 11), ref.filter_of(other[:20], 256, 3, 5), None][t]
            tabs.append(table(rng, keys, page, filt, tombstones=set(range(0, len(keys), 4))))
        qs = queries_for(pool)
        got = ref.get_many(tabs, qs)
        assert got == ref.closed_get_many(tabs, qs)
        for r in got:
            seen.update(r.stages)
            if r.status == ref.TOMBSTONE:
                assert r.value == b"" and set(r.stages[r.table + 1:]) <= {ref.NOT_SEARCHED}
        hidden = [r for q, r in zip(qs, got) if r.status == ref.TOMBSTONE and any(
            q in tab.keys and not ref.parse_record(tab.data, tab.offsets[tab.keys.index(q)])[0] & 1
            for tab in tabs[r.table + 1:])]
        assert hidden, "no tombstone hides a live record: the fixture is degenerate"
    assert seen == {ref.NOT_SEARCHED, ref.FILTER, ref.SUMMARY, ref.INDEX, ref.FOUND}


def test_hit_is_table_and_record_index():
    rng = np.random.default_rng(1)
    tabs = [table(rng, [b"b", b"d"], 3), table(rng, [b"a", b"c", b"d"], 3)]
    want = {b"a": (1 << 32) | 0, b"b": 0, b"c": (1 << 32) | 1, b"d": 1, b"e": ref.HIT_NONE}
    for q, h in want.items():
        assert ref.get(tabs, q).hit(tabs) == h == ref.closed_get(tabs, q).hit(tabs)
