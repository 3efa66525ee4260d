"""GPU: the batched point lookup over device-resident tables (nkv_lookup_dev,
nkv_lookup_values_dev, lsmtree.upload_table / get_many) against
tests/lookup_ref: every hit, status, stage byte, Value byte and offset.  Small
cases are held to the literal restatement of the engine's read path, the
large ones to the closed form that tests/test_lookup_ref.py holds to it.
Every device call writes into tests/guarded buffers at the minimum alignment
the header promises; the guards stay intact and every input is unchanged."""
import ctypes
import struct
from dataclasses import dataclass, field
from typing import Callable, List

import numpy as np
import pytest

from nakevaleng_amd import record
from tests import far, lookup_ref as ref
from tests.guarded import frozen, guarded

pytestmark = pytest.mark.gpu

INVALID = 2  # NKV_ERR_INVALID
FILL = 0xA5
NS = (1, 2, 3, 63, 64, 65, 1000)
KINDS = ("real", "tiny", None, "other", "k17")
HEADS = (b"", b"k", b"samehead", b"samehead\x80", b"\x80\xff", b"\xff" * 8)


def _torch():
    import torch
    return torch


def _dev(a):
    a = np.ascontiguousarray(a).view(np.uint8)
    t = _torch().from_numpy((a if a.size else np.zeros(1, np.uint8)).copy()).cuda()
    _torch().cuda.synchronize()
    return t


# ---------------------------------------------------------------------------
# tables and queries

def key_pool(rng, count):
    """Sorted distinct keys of 0..40 bytes, the empty key among them; many share
    their first 8 bytes (and more), many start with bytes >= 0x80."""
    pool = {b""}
    while len(pool) < count:
        head = HEADS[int(rng.integers(0, len(HEADS)))]
        ln = int(rng.integers(len(head), 41))
        pool.add(head + bytes(rng.integers(0, 256, ln - len(head), dtype=np.uint8)))
    return sorted(pool)


def make_filter(oracle, kind, keys, others, seed):
    if kind is None:
        return None
    if kind == "real":  # bloomfilter.New(n, 0.01)
        m, k = oracle.bloom_params(len(keys), 0.01)
        return ref.filter_of(keys, m, k, seed)
    if kind == "tiny":  # absent keys pass it
        return ref.filter_of(keys, 64, 2, seed)
    if kind == "other":  # built from other keys: it rejects keys the table holds
        return ref.filter_of(others[:40], 512, 4, seed)
    assert kind == "k17"  # two register passes of the hash states
    return ref.filter_of(keys, 4099, 17, seed)


def make_table(oracle, rng, keys, kind="real", others=(), page=3, tomb_every=5, values=None, vmax=60):
    recs = []
    for i, k in enumerate(keys):
        v = values[i] if values is not None else bytes(rng.integers(0, 256, int(rng.integers(0, vmax + 1)), np.uint8))
        r = record.New(k, v, 7)
        if tomb_every and i % tomb_every == 2:
            r.Status |= record.RECORD_TOMBSTONE_REMOVED
        recs.append(r)
    stream, sizes = record.data_table(recs)
    return ref.table_of(stream, sizes, page, make_filter(oracle, kind, keys, list(others), int(rng.integers(0, 2**32))))


def make_world(oracle, seed, ns, kinds=KINDS):
    """len(ns) tables over one key pool, so that tables share keys; table t
    holds ns[t] keys and a filter of kind kinds[t % len(kinds)]."""
    rng = np.random.default_rng(seed)
    pool = key_pool(rng, max(ns) * 3 // 2 + 40)
    tabs = []
    for t, n in enumerate(ns):
        keys = [pool[i] for i in sorted(rng.choice(len(pool), n, replace=False).tolist())]
        held = set(keys)
        tabs.append(make_table(oracle, rng, keys, kinds[t % len(kinds)], [k for k in pool if k not in held]))
    return tabs, pool, rng


def make_queries(rng, pool, q):
    """Pool keys (held by some tables, not by others), their successors and
    near misses (absent, mostly in range), keys outside every range, the empty
    key; duplicates included."""
    out = []
    for _ in range(q):
        k = pool[int(rng.integers(0, len(pool)))]
        what = int(rng.integers(0, 8))
        if what == 0:
            k = k + b"\x00" if len(k) < 40 else k[:-1]
        elif what == 1:
            k = k[:int(rng.integers(0, len(k) + 1))]
        elif what == 2:
            k = b"\xff" * int(rng.integers(9, 41))
        elif what == 3:
            k = b""
        out.append(k)
    return out


# ---------------------------------------------------------------------------
# device calls

@dataclass
class Up:  # tables on the device
    structs: object
    T: int
    keep: List[object] = field(default_factory=list)
    intact: List[Callable] = field(default_factory=list)


def upload(nkv, tabs, residues=(1, 3, 5, 7, 9, 11, 13, 15)) -> Up:
    """Every stream at an odd base offset, the filter words as they are."""
    _lib, _ = nkv
    up = Up((_lib.NkvLookupTable * len(tabs))(), len(tabs))
    for t, tab in enumerate(tabs):
        res = residues[t % len(residues)]
        host = np.zeros(res + len(tab.data) + 1, np.uint8)
        host[res:res + len(tab.data)] = np.frombuffer(tab.data, np.uint8)
        d_data, d_off = _dev(host), _dev(np.asarray(tab.offsets, np.uint64))
        d_bits = _dev(tab.filter.words()) if tab.filter is not None else None
        f = tab.filter
        up.structs[t] = _lib.NkvLookupTable(d_data.data_ptr() + res, len(tab.data), d_off.data_ptr(), len(tab.offsets),
                                            d_bits.data_ptr() if f else None, f.m if f else 0, f.k if f else 0,
                                            f.seed0 if f else 0)
        for d in (d_data, d_off, d_bits):
            if d is not None:
                up.keep.append(d)
                up.intact.append(frozen(d))
    return up


@dataclass
class Got:
    rc: int
    hit: np.ndarray
    status: np.ndarray
    stage: np.ndarray
    err: int
    p_hit: int
    p_status: int
    q: int
    keep: object


def pack_keys(queries, key_at):
    klen = np.asarray([len(k) for k in queries], np.uint64)
    koff = np.zeros(len(queries), np.uint64)
    if len(queries) > 1:
        koff[1:] = np.cumsum(klen[:-1])
    buf = b"".join(queries)
    host = np.zeros(key_at + len(buf) + 1, np.uint8)
    host[key_at:key_at + len(buf)] = np.frombuffer(buf, np.uint8)
    return host, koff, klen


def dev_lookup(nkv, up, queries, key_at=0, stage=True, err=True, keys_ptr=None) -> Got:
    """nkv_lookup_dev with the key buffer `key_at` bytes past a 256-byte
    boundary, d_hit at an 8-byte, d_err at a 4-byte and the byte arrays at odd
    addresses.  keys_ptr: the packed keys lie there already."""
    _lib, ctx = nkv
    q, T = len(queries), up.T
    host, koff, klen = pack_keys(queries, key_at)
    d_keys, d_koff, d_klen = _dev(host), _dev(koff), _dev(klen)
    same = up.intact + [frozen(d_keys), frozen(d_koff), frozen(d_klen)]
    p_hit, c_hit = guarded(8 * q, 8, fill=FILL)
    p_status, c_status = guarded(q, 1, fill=FILL)
    p_stage, c_stage = guarded(q * T, 3, fill=FILL)
    p_err, c_err = guarded(4, 4, fill=FILL)
    rc = _lib.lib().nkv_lookup_dev(ctx.h, up.structs, T, keys_ptr or d_keys.data_ptr() + key_at, d_koff.data_ptr(),
                                   d_klen.data_ptr(), q, p_hit, p_status, p_stage if stage else None,
                                   p_err if err else None)
    ctx.sync()
    for intact in same:
        intact()
    return Got(rc, c_hit().view(np.uint64), c_status(), c_stage().reshape(q, T),
               int(c_err().view(np.uint32)[0]), p_hit, p_status, q, (c_hit, c_status))


def dev_values(nkv, up, got, out_at=0, cap=None, room=None, query=True):
    """nkv_lookup_values_dev over a lookup's d_hit / d_status: the size query,
    then the gather into a guarded d_out `out_at` bytes past a 256-byte
    boundary.  Returns (rc, d_out's bytes, d_out_off as written, out_len)."""
    _lib, ctx = nkv
    L = _lib.lib()
    n = ctypes.c_uint64(7)
    args = (ctx.h, up.structs, up.T, got.p_hit, got.p_status, got.q)
    if query:
        rc = L.nkv_lookup_values_dev(*args, None, 0, None, ctypes.byref(n))
        if rc != 0:
            return rc, None, None, n.value
    room = n.value if room is None else room
    p_out, c_out = guarded(room, out_at, fill=FILL)
    p_off, c_off = guarded(8 * (got.q + 1), 8, fill=FILL)
    m = ctypes.c_uint64(7)
    rc = L.nkv_lookup_values_dev(*args, p_out, room if cap is None else cap, p_off, ctypes.byref(m))
    ctx.sync()
    for intact in up.intact:
        intact()
    assert np.array_equal(got.keep[0]().view(np.uint64), got.hit) and np.array_equal(got.keep[1](), got.status)
    if query and rc == 0:
        assert m.value == n.value
    return rc, c_out().tobytes(), c_off().view(np.uint64), m.value


def check(nkv, tabs, queries, closed=False, up=None, out_at=0, **kw):
    """One lookup and one gather against the reference.  Returns (the
    reference's results, the device's stage array)."""
    want = ref.closed_get_many(tabs, queries) if closed else ref.get_many(tabs, queries)
    up = up or upload(nkv, tabs)
    got = dev_lookup(nkv, up, queries, **kw)
    assert got.rc == 0 and got.err == 0
    assert got.hit.tolist() == [r.hit(tabs) for r in want]
    assert got.status.tolist() == [r.status for r in want]
    assert got.stage.tolist() == [list(r.stages) for r in want]
    rc, out, off, out_len = dev_values(nkv, up, got, out_at=out_at)
    packed = b"".join(r.value for r in want)
    assert rc == 0 and out_len == len(packed)
    assert off.tolist() == np.concatenate([[0], np.cumsum([len(r.value) for r in want])]).astype(np.uint64).tolist()
    assert out == packed
    return want, got.stage


# ---------------------------------------------------------------------------
# shapes

def _ns(T, start):
    return tuple(NS[(start + t) % len(NS)] for t in range(T))


@pytest.mark.parametrize("n", NS)
def test_one_table(nkv, oracle, n):
    for j, kind in enumerate(("real", None)):
        tabs, pool, rng = make_world(oracle, 0x6C00 + 7 * n + j, (n,), (kind,))
        queries = tabs[0].keys[:20] + tabs[0].keys[-3:] + make_queries(rng, pool, 40)
        check(nkv, tabs, queries[:63], key_at=n % 16, out_at=(3 * n) % 16)
        check(nkv, tabs, queries[:1], key_at=5)


@pytest.mark.parametrize("ns,q", [((1, 1000), 64), ((2, 65), 64), ((3, 64), 65), ((63, 1), 63), ((64, 64), 1)])
def test_two_tables(nkv, oracle, ns, q):
    tabs, pool, rng = make_world(oracle, 0x6C20 + ns[0], ns, ("tiny", "real"))
    check(nkv, tabs, make_queries(rng, pool, q), key_at=ns[0] % 16, out_at=7)


@pytest.mark.parametrize("start", [0, 3, 6])
def test_five_tables(nkv, oracle, start):
    tabs, pool, rng = make_world(oracle, 0x6C50 + start, _ns(5, start))
    check(nkv, tabs, make_queries(rng, pool, 65), key_at=start + 1, out_at=start)


def test_thirty_two_tables(nkv, oracle):
    tabs, pool, rng = make_world(oracle, 0x6C32, _ns(32, 0))
    want, _ = check(nkv, tabs, make_queries(rng, pool, 63), key_at=9, out_at=1)
    assert max(r.table for r in want) >= 8  # answers come from deep in the order too


def test_many_queries(nkv, oracle):
    """q = 4097: 17 workgroups, the last with one query.  The closed form for
    all of them, the literal restatement for the first 64."""
    tabs, pool, rng = make_world(oracle, 0x6C97, (1000, 65), ("real", "tiny"))
    queries = make_queries(rng, pool, 4097)
    up = upload(nkv, tabs)
    want, _ = check(nkv, tabs, queries, closed=True, up=up, key_at=3, out_at=13)
    assert want[:64] == ref.get_many(tabs, queries[:64])
    assert {r.status for r in want} == {ref.ABSENT, ref.LIVE, ref.TOMBSTONE}


def test_no_queries(nkv, oracle):
    tabs, pool, rng = make_world(oracle, 0x6C01, _ns(5, 2))
    up = upload(nkv, tabs)
    got = dev_lookup(nkv, up, [])
    assert got.rc == 0 and got.err == FILL * 0x01010101  # nothing written, d_err included
    rc, out, off, out_len = dev_values(nkv, up, got, out_at=3)
    assert rc == 0 and out_len == 0 and out == b"" and off.tolist() == [0]


@pytest.mark.parametrize("key_at", range(16))
def test_every_key_buffer_alignment(nkv, oracle, key_at):
    tabs, pool, rng = make_world(oracle, 0x6CA0, (65, 64), ("k17", "real"))
    check(nkv, tabs, make_queries(rng, pool, 65), key_at=key_at, out_at=15 - key_at)


def test_without_stage_array(nkv, oracle):
    tabs, pool, rng = make_world(oracle, 0x6CA1, (63, 3))
    queries = make_queries(rng, pool, 64)
    want = ref.get_many(tabs, queries)
    got = dev_lookup(nkv, upload(nkv, tabs), queries, stage=False)
    assert got.rc == 0 and got.hit.tolist() == [r.hit(tabs) for r in want]
    assert (got.stage == FILL).all()


# ---------------------------------------------------------------------------
# order, tombstones, filters

def test_first_table_wins_and_a_tombstone_hides_a_live_record(nkv, oracle):
    rng = np.random.default_rng(0x6CB0)
    dead = record.New(b"dead", b"", 7)
    dead.Status |= record.RECORD_TOMBSTONE_REMOVED
    recs = [record.New(b"both", b"new value", 7), dead, record.New(b"newer-only", b"n", 7)]
    newer = ref.table_of(*record.data_table(recs), 3)
    older = make_table(oracle, rng, [b"both", b"dead", b"older-only"], None, tomb_every=0,
                       values=[b"old value", b"still alive here", b"o"])
    tabs = [newer, older]
    queries = [b"both", b"dead", b"newer-only", b"older-only", b"nowhere", b"dead"]
    want, stage = check(nkv, tabs, queries)
    assert [r.value for r in want] == [b"new value", b"", b"n", b"o", b"", b""]
    assert want[1].status == ref.TOMBSTONE and want[1].table == 0
    assert stage[1].tolist() == [ref.FOUND, ref.NOT_SEARCHED] == stage[5].tolist()
    assert stage[0].tolist() == [ref.FOUND, ref.NOT_SEARCHED]
    assert stage[3].tolist() == [ref.SUMMARY, ref.FOUND]
    # the other order: the live record answers
    want, _ = check(nkv, tabs[::-1], queries)
    assert want[1].status == ref.LIVE and want[1].value == b"still alive here"


def test_filters_and_every_stage(nkv, oracle):
    """Tiny filters let absent keys through to SUMMARY and to INDEX, a filter
    built from other keys rejects held keys (FILTER, and the search goes on),
    one table has no filter, one takes k = 17."""
    kinds = ("tiny", "other", None, "k17", "tiny")
    tabs, pool, rng = make_world(oracle, 0x6CF1, (64, 65, 63, 64, 3), kinds)
    queries = pool + make_queries(rng, pool, 100)
    want, stage = check(nkv, tabs, queries, closed=True)
    assert want[:64] == ref.get_many(tabs, queries[:64])
    assert set(np.unique(stage).tolist()) == {ref.NOT_SEARCHED, ref.FILTER, ref.SUMMARY, ref.INDEX, ref.FOUND}
    per = {t: set() for t in range(5)}
    rejected_but_held = found_after_filter = 0
    for qk, r in zip(queries, want):
        for t, s in enumerate(r.stages):
            if qk not in tabs[t].keys:
                per[t].add(s)
            elif s == ref.FILTER:
                rejected_but_held += 1
                found_after_filter += r.table > t
    assert {ref.SUMMARY, ref.INDEX} <= per[0]  # absent keys passed the tiny filter
    assert {ref.SUMMARY, ref.INDEX} <= per[2]  # and the table without one
    assert ref.FILTER in per[3]  # k = 17 rejects absent keys
    assert rejected_but_held and found_after_filter


# ---------------------------------------------------------------------------
# the gather

VALUE_LENGTHS = (0, 1, 15, 16, 17, 4096, 70000)


@pytest.fixture(scope="module")
def value_world(oracle):
    rng = np.random.default_rng(0x6CE0)
    keys = set()
    while len(keys) < 14:
        keys.add(bytes(rng.integers(0, 256, int(rng.integers(1, 41)), np.uint8)))
    keys = sorted(keys)
    lens = [VALUE_LENGTHS[i % 7] for i in range(len(keys))]
    values = [bytes(rng.integers(0, 256, ln, np.uint8)) for ln in lens]
    tab = make_table(oracle, rng, keys, None, tomb_every=0, values=values)
    other = make_table(oracle, rng, keys[:3], "real", tomb_every=3, values=[b"x" * 33] * 3)
    tabs = [other, tab]
    queries = keys + [b"", keys[3] + b"\x00"] + keys[::-1] + [keys[6]] * 3
    return tabs, queries, ref.get_many(tabs, queries)


@pytest.mark.parametrize("out_at", range(16))
def test_value_lengths_at_every_output_alignment(nkv, value_world, out_at):
    tabs, queries, want = value_world
    up = upload(nkv, tabs, residues=(out_at | 1, (out_at + 7) | 1))
    got = dev_lookup(nkv, up, queries)
    assert got.rc == 0 and got.status.tolist() == [r.status for r in want]
    rc, out, off, out_len = dev_values(nkv, up, got, out_at=out_at)
    packed = b"".join(r.value for r in want)
    assert rc == 0 and out_len == len(packed) > 3 * 70000
    assert off.tolist() == np.concatenate([[0], np.cumsum([len(r.value) for r in want])]).tolist()
    assert out == packed
    assert {len(r.value) for r in want} >= set(VALUE_LENGTHS)


def test_more_queries_than_bytes_in_a_tile(nkv, oracle):
    """Values of 0..2 bytes: one 16-KiB tile of d_out holds the Values of all
    4097 queries, more than the copy keeps in LDS."""
    rng = np.random.default_rng(0x6CE1)
    pool = key_pool(rng, 1000)
    values = [bytes(rng.integers(0, 256, int(rng.integers(0, 3)), np.uint8)) for _ in pool]
    tabs = [make_table(oracle, rng, pool, None, tomb_every=7, values=values)]
    queries = [pool[int(i)] for i in rng.integers(0, len(pool), 4097)]
    want, _ = check(nkv, tabs, queries, closed=True, out_at=5)
    assert 2000 < sum(len(r.value) for r in want) < 16384


def test_size_query_and_a_capacity_one_byte_short(nkv, value_world):
    tabs, queries, want = value_world
    up = upload(nkv, tabs)
    got = dev_lookup(nkv, up, queries)
    total = sum(len(r.value) for r in want)
    rc, out, off, out_len = dev_values(nkv, up, got, out_at=3, room=total, cap=total - 1, query=False)
    assert rc == INVALID and out_len == total  # still reported: the caller can retry
    assert out == bytes([FILL]) * total and (off.view(np.uint8) == FILL).all()
    # more room than needed: only the reported extent is written
    rc, out, off, out_len = dev_values(nkv, up, got, out_at=9, room=total + 50, query=False)
    assert rc == 0 and out_len == total
    assert out == b"".join(r.value for r in want) + bytes([FILL]) * 50


def test_all_absent(nkv, oracle):
    tabs, pool, rng = make_world(oracle, 0x6CE2, (64, 2), ("real", None))
    queries = [b"\xff" * 30, b"\xff" * 31] * 40
    up = upload(nkv, tabs)
    got = dev_lookup(nkv, up, queries)
    assert got.rc == 0 and (got.hit == ref.HIT_NONE).all() and (got.status == ref.ABSENT).all()
    rc, out, off, out_len = dev_values(nkv, up, got, out_at=11, room=64, query=False)
    assert rc == 0 and out_len == 0 and out == bytes([FILL]) * 64 and off.tolist() == [0] * 81


# ---------------------------------------------------------------------------
# errors: argument and data checks, none of which may reach past a buffer

def _good(nkv, oracle):
    tabs, pool, rng = make_world(oracle, 0x6CD0, (3, 2), (None, "tiny"))
    check(nkv, tabs, make_queries(rng, pool, 10))


def test_refused_arguments(nkv, oracle):
    _lib, ctx = nkv
    L = _lib.lib()
    tabs, pool, rng = make_world(oracle, 0x6CD1, (3, 2), (None, "tiny"))
    up = upload(nkv, tabs)
    queries = make_queries(rng, pool, 5)
    host, koff, klen = pack_keys(queries, 0)
    d_keys, d_koff, d_klen = _dev(host), _dev(koff), _dev(klen)
    p_hit, c_hit = guarded(8 * 5, 8, fill=FILL)
    p_status, c_status = guarded(5, 1, fill=FILL)
    n = ctypes.c_uint64(0)
    many = (_lib.NkvLookupTable * 33)(*[up.structs[0]] * 33)
    empty = (_lib.NkvLookupTable * 2)(up.structs[0], up.structs[1])
    empty[1].n = 0
    nofilter = (_lib.NkvLookupTable * 1)(up.structs[1])
    nofilter[0].m = 0  # k = 2 hash functions over 0 bits

    def lookup(structs, T, q=5, ctx_h=ctx.h, keys=d_keys.data_ptr(), hit=p_hit):
        return L.nkv_lookup_dev(ctx_h, structs, T, keys, d_koff.data_ptr(), d_klen.data_ptr(), q, hit, p_status,
                                None, None)

    def values(structs, T, q=5, n_ptr=ctypes.byref(n)):
        return L.nkv_lookup_values_dev(ctx.h, structs, T, p_hit, p_status, q, None, 0, None, n_ptr)

    for structs, T in ((up.structs, 0), (many, 33), (up.structs, -1), (empty, 2), (nofilter, 1), (None, 1)):
        assert lookup(structs, T) == INVALID
        assert values(structs, T) == INVALID
    assert lookup(many, 32) == 0  # the most tables a call takes
    assert lookup(up.structs, 2, q=2**31) == INVALID
    assert values(up.structs, 2, q=2**31) == INVALID
    assert lookup(up.structs, 2, ctx_h=None) == INVALID
    assert lookup(up.structs, 2, keys=None) == INVALID
    assert lookup(up.structs, 2, hit=None) == INVALID
    assert values(up.structs, 2, n_ptr=None) == INVALID
    ctx.sync()
    _good(nkv, oracle)


def _three(oracle):
    rng = np.random.default_rng(0x6CD2)
    return make_table(oracle, rng, [b"b", b"d", b"f"], None, tomb_every=0, values=[b"bee", b"dee", b"eff"])


BAD_TABLES = {
    # record 1's KeySize reaches past the end of the stream
    "key_past_stream": lambda s, off: (s[:off[1] + 14] + struct.pack("<Q", len(s) - off[1] - 30 + 1) + s[off[1] + 22:], off),
    "key_size_wraps": lambda s, off: (s[:off[1] + 14] + struct.pack("<Q", 2**64 - 8) + s[off[1] + 22:], off),
    "rec_off_past_stream": lambda s, off: (s, [off[0], len(s) - 29, off[2]]),
    "rec_off_wild": lambda s, off: (s, [off[0], 2**64 - 8, off[2]]),
}


@pytest.mark.parametrize("name", sorted(BAD_TABLES))
def test_a_record_that_reaches_outside_its_stream(nkv, oracle, name):
    """Probing record 1 sets d_err (or gives NKV_ERR_INVALID without one) and
    counts as no match; keys found without probing it are still answered, and
    the context serves a good call right after."""
    tab = _three(oracle)
    tab.data, tab.offsets = BAD_TABLES[name](tab.data, list(tab.offsets))
    up = upload(nkv, [tab])
    queries = [b"b", b"c", b"f", b"d", b"a", b"g"]
    got = dev_lookup(nkv, up, queries)
    assert got.rc == 0 and got.err == 1
    assert got.hit.tolist() == [0, ref.HIT_NONE, 2, ref.HIT_NONE, ref.HIT_NONE, ref.HIT_NONE]
    assert got.stage[:, 0].tolist() == [ref.FOUND, ref.INDEX, ref.FOUND, ref.INDEX, ref.SUMMARY, ref.SUMMARY]
    assert dev_lookup(nkv, up, queries, err=False).rc == INVALID
    # queries that never probe the bad record leave the flag at 0
    got = dev_lookup(nkv, up, [b"b", b"f", b"a"])
    assert got.rc == 0 and got.err == 0 and dev_lookup(nkv, up, [b"b", b"f", b"a"], err=False).rc == 0
    _good(nkv, oracle)


def test_a_value_that_reaches_outside_its_stream(nkv, oracle):
    tab = _three(oracle)
    o = tab.offsets[2]
    tab.data = tab.data[:o + 22] + struct.pack("<Q", 4) + tab.data[o + 30:]  # ValueSize 4 of a 3-byte Value
    up = upload(nkv, [tab])
    got = dev_lookup(nkv, up, [b"b", b"f"])
    assert got.rc == 0 and got.err == 0 and got.status.tolist() == [ref.LIVE, ref.LIVE]
    rc, _, _, out_len = dev_values(nkv, up, got)
    assert rc == INVALID and out_len == 0
    rc, out, off, out_len = dev_values(nkv, up, got, room=64, query=False, out_at=1)
    assert rc == INVALID and out_len == 0 and out == bytes([FILL]) * 64 and (off.view(np.uint8) == FILL).all()
    # a hit that names no record is refused the same way
    d_hit = _dev(np.asarray([5, 1 << 32], np.uint64))  # record 5 of 3, table 1 of 1
    n = ctypes.c_uint64(7)
    _lib, ctx = nkv
    assert _lib.lib().nkv_lookup_values_dev(ctx.h, up.structs, 1, d_hit.data_ptr(), got.p_status, 2, None, 0, None,
                                            ctypes.byref(n)) == INVALID
    _good(nkv, oracle)


# ---------------------------------------------------------------------------
# tables and keys more than 4 GiB apart

def test_tables_and_keys_4_gib_apart(nkv, oracle):
    """Two table streams and the query buffer in islands at 0, about 2^32 and
    about 2 * 2^32 of one allocation (tests/far.py)."""
    torch = _torch()
    _lib, ctx = nkv
    tabs, pool, rng = make_world(oracle, 0x6CFA, (65, 1000), ("real", None))
    queries = make_queries(rng, pool, 64)
    host, _, _ = pack_keys(queries, 0)
    big = torch.empty(far.ALLOC, dtype=torch.uint8, device="cuda")
    try:
        at = [far.BASES[0] + 1, far.BASES[1] + 3, far.BASES[2] + 5]
        blobs = [np.frombuffer(tabs[0].data, np.uint8), np.frombuffer(tabs[1].data, np.uint8), host]
        for a, blob in zip(at, blobs):
            big[a:a + blob.size].copy_(torch.from_numpy(blob.copy()))
        torch.cuda.synchronize()
        assert at[1] - at[0] > far.G32 and at[2] - at[1] > far.G32
        up = upload(nkv, tabs)  # the offsets and the filter; the streams are the islands
        for t in range(2):
            up.structs[t].stream = big.data_ptr() + at[t]
        want, _ = check(nkv, tabs, queries, up=up, keys_ptr=big.data_ptr() + at[2], out_at=3)
        assert {r.table for r in want} >= {0, 1}
        for a, blob in zip(at, blobs):
            assert np.array_equal(big[a:a + blob.size].cpu().numpy(), blob)
    finally:
        del big
        torch.cuda.empty_cache()


# ---------------------------------------------------------------------------
# lsmtree.upload_table / get_many / compact(resident=True)

def _bloom_of(f):
    from nakevaleng_amd import bloomfilter
    return bloomfilter.BloomFilter(f.m, f.k, [(f.seed0 + j) & 0xFFFFFFFF for j in range(f.k)], f.contents)


def _sizes(tab):
    return np.diff(np.asarray(tab.offsets + [len(tab.data)], np.uint64)).astype(np.uint64)


def test_get_many_over_uploaded_tables(nkv, oracle):
    from nakevaleng_amd import lsmtree
    tabs, pool, rng = make_world(oracle, 0x6C71, (65, 63), ("real", None))
    handles = [lsmtree.upload_table((t.data, _sizes(t)), filter=_bloom_of(t.filter) if t.filter else None, device=0)
               for t in tabs]
    queries = make_queries(rng, pool, 100)
    want = ref.get_many(tabs, queries)
    expect = [r.value if r.status == ref.LIVE else None for r in want]
    assert lsmtree.get_many(handles, queries) == expect
    values, stages, hits = lsmtree.get_many(handles, queries, device=0, stages=True)
    assert values == expect
    assert stages.tolist() == [list(r.stages) for r in want]
    assert hits.tolist() == [r.hit(tabs) for r in want]
    assert {None, b""} & set(expect) and any(expect)
    assert lsmtree.get_many(handles, []) == []
    with pytest.raises(ValueError):
        lsmtree.get_many([], [b"k"])
    with pytest.raises(ValueError):
        lsmtree.upload_table((b"", np.zeros(0, np.uint64)), device=0)


def test_get_many_over_a_compaction_output(nkv, oracle):
    from nakevaleng_amd import lsmtree
    from tests.test_gpu_merge import fuzz_runs
    rng = np.random.default_rng(0x6C72)
    runs = [record.data_table(run) for run in fuzz_runs(rng, 3, nmax=150, vmax=400)]
    plain = lsmtree.compact(runs, device=0, seed=99)
    out, handle = lsmtree.compact(runs, device=0, seed=99, resident=True)
    assert sorted(out) == sorted(plain) and out["table"][0] == plain["table"][0] and out["root"] == plain["root"]
    stream, sizes = out["table"]
    bf = out["filter"]
    tab = ref.table_of(stream, sizes, 3, ref.Filter(bf.M, bf.K, bf.HashSeeds[0], bf.Contents))
    older = make_table(oracle, rng, tab.keys[::3] + [tab.keys[-1] + b"z"], "real", tomb_every=0)
    queries = tab.keys + [k + b"\x00" for k in tab.keys[:50]] + older.keys + [b"", b"\xff" * 20]
    tabs = [tab, older]
    want = ref.get_many(tabs, queries)
    handles = [handle, lsmtree.upload_table((older.data, _sizes(older)), filter=_bloom_of(older.filter), device=0)]
    values, stages, hits = lsmtree.get_many(handles, queries, stages=True)
    assert values == [r.value if r.status == ref.LIVE else None for r in want]
    assert stages.tolist() == [list(r.stages) for r in want]
    assert hits.tolist() == [r.hit(tabs) for r in want]
    assert all(r.status != ref.ABSENT for r in want[:len(tab.keys)])  # the filter the device built holds every key
