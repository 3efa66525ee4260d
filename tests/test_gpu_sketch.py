"""GPU: HyperLogLog and Count-Min Sketch (csrc/sketch.hip) through the C-ABI and
the Python mirrors, byte for byte against tests/sketch_ref.py (pinned on the
CPU by tests/test_sketch_ref.py).  Every update runs on every value of
NKV_OPT_SKETCH_PATH (auto, direct global atomics, workgroup-private LDS copies)
and must leave the same bytes.  Seeds are explicit (the reference draws them
from the clock)."""
from functools import lru_cache

import numpy as np
import pytest

from tests import sketch_ref as ref
from tests.guarded import frozen, guarded

pytestmark = pytest.mark.gpu

PATHS = (0, 1, 2)
NS = (0, 1, 63, 64, 65, 5000)
TABLES = [(1, 1), (28, 3), (2719, 5), (27183, 14), (5000, 20), (3, 33)]  # (M, K); the last two: > 16 rows = two
#                                                                          register passes; (27183, 14) exceeds LDS
INVALID = 2


def _torch():
    import torch
    return torch


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


@lru_cache(maxsize=None)
def _keys(n, tag=0):
    """n keys of 0..40 bytes with [1000, 4097, 3, 0] in front, 3 bytes apart, so
    every byte alignment 0-3 occurs (the layout of test_gpu_bloom)."""
    rng = np.random.default_rng(1000 * tag + n)
    ln = rng.integers(0, 41, max(n, 1)).astype(np.uint64)
    ln[:4] = [1000, 4097, 3, 0][:ln.size]
    ln = ln[:n]
    off = np.zeros(n, np.uint64)
    if n > 1:
        off[1:] = np.cumsum(ln[:-1] + np.uint64(3))
    data = rng.integers(0, 256, int(off[-1] + ln[-1]) + 1 if n else 1, dtype=np.uint8)
    if n >= 63:
        assert {int(o) % 4 for o in off} == {0, 1, 2, 3}
    for a in (data, off, ln):
        a.setflags(write=False)
    return data, off, ln


@lru_cache(maxsize=None)
def _keys_200k(tag=0):
    rng = np.random.default_rng(77 + tag)
    n = 200000
    ln = rng.integers(0, 41, n).astype(np.uint64)
    off = np.zeros(n, np.uint64)
    off[1:] = np.cumsum(ln[:-1] + rng.integers(0, 4, n - 1).astype(np.uint64))
    data = rng.integers(0, 256, int(off[-1] + ln[-1]) + 1, dtype=np.uint8)
    return data, off, ln


@lru_cache(maxsize=None)
def _hashes_200k(seed):
    data, off, ln = _keys_200k()
    return ref.murmur3_32_many(data, off, ln, seed)


@pytest.fixture(scope="module")
def sk(nkv):
    """(_lib, a context of its own whose NKV_OPT_SKETCH_PATH the tests switch, the library)."""
    _lib, _ = nkv
    ctx = _lib.Context(0)
    yield _lib, ctx, _lib.lib()
    ctx.close()


class _Path:
    def __init__(self, sk, path):
        self.sk, self.path = sk, path

    def __enter__(self):
        self.sk[1].set_option(self.sk[0].NKV_OPT_SKETCH_PATH, self.path)

    def __exit__(self, *exc):
        self.sk[1].set_option(self.sk[0].NKV_OPT_SKETCH_PATH, 0)


def _hll_dev(sk, path, dkeys, n, p, pre, at=0):
    """nkv_hll_add_dev over uploaded keys into a guarded register file that starts as `pre`."""
    _lib, ctx, L = sk
    p_reg, c_reg = guarded(1 << p, at, init=pre)
    with _Path(sk, path):
        _lib.check(L.nkv_hll_add_dev(ctx.h, dkeys[0].data_ptr(), dkeys[1].data_ptr(), dkeys[2].data_ptr(), n, p,
                                     p_reg))
        ctx.sync()
    return c_reg()


def _cms_dev(sk, path, dkeys, n, m, k, seed0, pre, at=0):
    _lib, ctx, L = sk
    p_tab, c_tab = guarded(4 * m * k, at, init=pre)
    with _Path(sk, path):
        _lib.check(L.nkv_cms_insert_dev(ctx.h, dkeys[0].data_ptr(), dkeys[1].data_ptr(), dkeys[2].data_ptr(), n, m,
                                        k, seed0, p_tab))
        ctx.sync()
    return c_tab().view(np.uint32).reshape(k, m)


def _cms_query_dev(sk, dkeys, n, m, k, seed0, table, at=4):
    _lib, ctx, L = sk
    d_tab = _dev(table)
    _torch().cuda.synchronize()
    p_out, c_out = guarded(4 * n, at)
    _lib.check(L.nkv_cms_query_dev(ctx.h, dkeys[0].data_ptr(), dkeys[1].data_ptr(), dkeys[2].data_ptr(), n, m, k,
                                   seed0, d_tab.data_ptr(), p_out))
    ctx.sync()
    return c_out().view(np.uint32)


def _upload(keys):
    d = [_dev(a) for a in keys]
    _torch().cuda.synchronize()
    return d


# ---------------------------------------------------------------------------
# HLL

@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("p", [4, 5, 11, 14, 16])
def test_hll_add_matches_ref_on_every_path(sk, p, n):
    keys = _keys(n)
    dkeys = _upload(keys)
    intact = [frozen(t) for t in dkeys]
    rng = np.random.default_rng(p * 100 + n)
    zero = np.zeros(1 << p, np.uint8)
    pre = (rng.integers(0, 34, 1 << p) * (rng.random(1 << p) < 0.5)).astype(np.uint8)
    for start in (zero, pre):
        want = ref.hll_add_many(start, *keys, p)
        if n == 0:
            assert np.array_equal(want, start)
        for path in PATHS:
            got = _hll_dev(sk, path, dkeys, n, p, start, at=4)
            assert np.array_equal(got, want), (path, int(np.flatnonzero(got != want)[0]))
    if n >= 4:
        assert ref.hll_add_many(zero, *keys, p)[0] == 33  # the empty key (key 3) hashes to 0
    for check in intact:
        check()


@pytest.mark.parametrize("p", [14, 16])
def test_hll_200k_keys_and_two_calls_equal_one(sk, p):
    """Several workgroups per path; and the keys split over two calls (of
    different paths) leave what one call leaves."""
    _lib, ctx, L = sk
    keys = _keys_200k()
    n = keys[1].size
    zero = np.zeros(1 << p, np.uint8)
    want = ref.hll_add_many(zero, *keys, p)
    dkeys = _upload(keys)
    for path in PATHS:
        assert np.array_equal(_hll_dev(sk, path, dkeys, n, p, zero), want), path
    cut = 123457
    d_off2, d_len2 = _dev(keys[1][cut:]), _dev(keys[2][cut:])
    _torch().cuda.synchronize()
    for first, second in ((1, 2), (2, 1), (0, 0)):
        p_reg, c_reg = guarded(1 << p, 4, init=zero)
        with _Path(sk, first):
            _lib.check(L.nkv_hll_add_dev(ctx.h, dkeys[0].data_ptr(), dkeys[1].data_ptr(), dkeys[2].data_ptr(), cut,
                                         p, p_reg))
        with _Path(sk, second):
            _lib.check(L.nkv_hll_add_dev(ctx.h, dkeys[0].data_ptr(), d_off2.data_ptr(), d_len2.data_ptr(), n - cut,
                                         p, p_reg))
        ctx.sync()
        assert np.array_equal(c_reg(), want), (first, second)


def test_hll_200k_identical_keys_hit_one_register(sk):
    p, n = 14, 200000
    key = b"the one key that every lane adds"
    data = np.frombuffer(b"\0" + key, np.uint8)
    off, ln = np.full(n, 1, np.uint64), np.full(n, len(key), np.uint64)
    h = ref.HLLRef(p)
    h.Add(key)
    want = np.array(h.Reg, np.uint8)
    assert np.count_nonzero(want) == 1
    dkeys = _upload((data, off, ln))
    for path in PATHS:
        assert np.array_equal(_hll_dev(sk, path, dkeys, n, p, np.zeros(1 << p, np.uint8)), want), path


def test_hll_registers_that_start_non_zero_and_a_33_survive(sk):
    p = 11
    keys = _keys(5000)
    zero = np.zeros(1 << p, np.uint8)
    fresh = ref.hll_add_many(zero, *keys, p)
    pre = np.zeros(1 << p, np.uint8)
    hit = np.flatnonzero(fresh)
    hit = hit[hit > 0]          # register 0 already holds the empty key's 33
    pre[hit[0]] = 33            # above anything a non-zero hash can give (at most 32): must survive
    pre[hit[1]] = fresh[hit[1]]  # equal: unchanged
    pre[hit[2]] = fresh[hit[2]] - 1  # below: raised to the new value
    empty = np.flatnonzero(fresh == 0)
    pre[empty[0]] = 7           # a register no key touches keeps its value
    want = np.maximum(pre, fresh)
    assert want[hit[0]] == 33 and want[empty[0]] == 7
    dkeys = _upload(keys)
    for path in PATHS:
        assert np.array_equal(_hll_dev(sk, path, dkeys, 5000, p, pre, at=4), want), path


# ---------------------------------------------------------------------------
# CMS

@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("m,k", TABLES)
def test_cms_insert_and_query_match_ref_on_every_path(sk, m, k, n):
    keys = _keys(n)
    dkeys = _upload(keys)
    intact = [frozen(t) for t in dkeys]
    rng = np.random.default_rng(m + k + n)
    seed0 = int(rng.integers(0, 2**32))
    pre = rng.integers(0, 2**32, (k, m), dtype=np.uint32) * (rng.random((k, m)) < 0.3).astype(np.uint32)
    idx = ref.cms_indices(*keys, m, k, seed0)  # hashed once for both starts and the query
    for start in (np.zeros((k, m), np.uint32), pre):
        want = ref.cms_insert_many(start, *keys, seed0, idx=idx)
        for path in PATHS:
            got = _cms_dev(sk, path, dkeys, n, m, k, seed0, start, at=4)
            assert np.array_equal(got, want), path
    table = ref.cms_insert_many(np.zeros((k, m), np.uint32), *keys, seed0, idx=idx)
    if n:
        got = _cms_query_dev(sk, dkeys, n, m, k, seed0, table)
        assert np.array_equal(got, ref.cms_query_many(table, *keys, seed0, idx=idx))
        assert (got >= 1).all()
    for check in intact:
        check()


@pytest.mark.parametrize("m,k", [(28, 3), (27183, 14)])
def test_cms_200k_identical_keys_count_exactly(sk, m, k):
    n, seed0 = 200000, 41
    key = b"\x01\x02"
    data = np.frombuffer(b"\0\0\0" + key, np.uint8)
    off, ln = np.full(n, 3, np.uint64), np.full(n, 2, np.uint64)
    c = ref.CMSRef(m, k, seed0)
    c.Insert(key)
    want = np.array(c.Contents, np.uint32) * np.uint32(n)
    assert (want.sum(axis=1) == n).all()
    dkeys = _upload((data, off, ln))
    for path in PATHS:
        got = _cms_dev(sk, path, dkeys, n, m, k, seed0, np.zeros((k, m), np.uint32))
        assert np.array_equal(got, want), path


@pytest.mark.parametrize("m,k", [(28, 3), (2719, 5), (27183, 14)])
def test_cms_200k_ragged_keys(sk, m, k):
    """Several workgroups per path on distinct keys, and two calls equal one."""
    _lib, ctx, L = sk
    keys = _keys_200k()
    n, seed0 = keys[1].size, 2**32 - 2  # the seeds wrap at row 2
    want = np.stack([np.bincount((_hashes_200k((seed0 + i) & 0xFFFFFFFF) % np.uint32(m)).astype(np.int64),
                                 minlength=m).astype(np.uint32) for i in range(k)])
    dkeys = _upload(keys)
    for path in PATHS:
        assert np.array_equal(_cms_dev(sk, path, dkeys, n, m, k, seed0, np.zeros((k, m), np.uint32)), want), path
    cut = 99999
    d_off2, d_len2 = _dev(keys[1][cut:]), _dev(keys[2][cut:])
    _torch().cuda.synchronize()
    p_tab, c_tab = guarded(4 * m * k, 4, init=np.zeros((k, m), np.uint32))
    with _Path(sk, 2):
        _lib.check(L.nkv_cms_insert_dev(ctx.h, dkeys[0].data_ptr(), dkeys[1].data_ptr(), dkeys[2].data_ptr(), cut, m,
                                        k, seed0, p_tab))
    with _Path(sk, 1):
        _lib.check(L.nkv_cms_insert_dev(ctx.h, dkeys[0].data_ptr(), d_off2.data_ptr(), d_len2.data_ptr(), n - cut, m,
                                        k, seed0, p_tab))
    ctx.sync()
    assert np.array_equal(c_tab().view(np.uint32).reshape(k, m), want)


def test_cms_counter_wraps_at_2_32(sk):
    m, k, seed0 = 28, 3, 9
    key = b"wrap"
    c = ref.CMSRef(m, k, seed0)
    c.Insert(key)
    rows = [int(np.flatnonzero(np.array(r))[0]) for r in c.Contents]
    pre = np.zeros((k, m), np.uint32)
    pre[1, rows[1]] = 0xFFFFFFF0
    data = np.frombuffer(key, np.uint8)
    off, ln = np.zeros(32, np.uint64), np.full(32, len(key), np.uint64)
    dkeys = _upload((data, off, ln))
    for path in PATHS:
        got = _cms_dev(sk, path, dkeys, 32, m, k, seed0, pre, at=4)
        assert got[1, rows[1]] == 0x00000010 and got[0, rows[0]] == 32 and got[2, rows[2]] == 32, path
        assert got.sum(dtype=np.uint64) == 32 + 32 + 0x10


# ---------------------------------------------------------------------------
# records forms

@lru_cache(maxsize=None)
def _records():
    from nakevaleng_amd import record
    rng = np.random.default_rng(4)
    recs = [record.New(rng.bytes(int(kk)), rng.bytes(int(v)), timestamp=1)
            for kk, v in zip(rng.integers(1, 33, 2000), rng.integers(0, 301, 2000))]
    stream, sizes = record.data_table(recs)
    keys = [r.Key for r in recs]
    kl = np.array([len(x) for x in keys], np.uint64)
    ko = np.zeros_like(kl)
    ko[1:] = np.cumsum(kl[:-1])
    return bytes(stream), np.asarray(sizes, np.uint64), (np.frombuffer(b"".join(keys), np.uint8), ko, kl)


def test_records_forms_equal_the_span_forms(sk):
    _lib, ctx, L = sk
    stream, sizes, keys = _records()
    n = sizes.size
    rec_off = np.zeros(n, np.uint64)
    rec_off[1:] = np.cumsum(sizes[:-1])
    d_stream, d_off = _dev(np.frombuffer(stream, np.uint8)), _dev(rec_off)
    _torch().cuda.synchronize()
    intact = [frozen(d_stream), frozen(d_off)]
    p, m, k, seed0 = 11, 2719, 5, 1234
    want_reg = ref.hll_add_many(np.zeros(1 << p, np.uint8), *keys, p)
    want_tab = ref.cms_insert_many(np.zeros((k, m), np.uint32), *keys, seed0)
    buf = np.frombuffer(stream, np.uint8)
    for path in PATHS:
        p_reg, c_reg = guarded(1 << p, 4, init=np.zeros(1 << p, np.uint8))
        p_tab, c_tab = guarded(4 * m * k, 4, init=np.zeros(4 * m * k, np.uint8))
        with _Path(sk, path):
            _lib.check(L.nkv_hll_add_records_dev(ctx.h, d_stream.data_ptr(), len(stream), d_off.data_ptr(), n, p,
                                                 p_reg))
            _lib.check(L.nkv_cms_insert_records_dev(ctx.h, d_stream.data_ptr(), len(stream), d_off.data_ptr(), n, m,
                                                    k, seed0, p_tab))
            ctx.sync()
            # the host-pointer forms: staged, synchronous, read-update-write of the caller's arrays
            reg = np.zeros(1 << p, np.uint8)
            tab = np.zeros((k, m), np.uint32)
            _lib.check(L.nkv_hll_add_records(ctx.h, buf.ctypes.data, buf.size, sizes.ctypes.data, n, p,
                                             reg.ctypes.data))
            _lib.check(L.nkv_cms_insert_records(ctx.h, buf.ctypes.data, buf.size, sizes.ctypes.data, n, m, k, seed0,
                                                tab.ctypes.data))
            reg2 = np.zeros(1 << p, np.uint8)
            tab2 = np.zeros((k, m), np.uint32)
            _lib.check(L.nkv_hll_add(ctx.h, keys[0].ctypes.data, keys[1].ctypes.data, keys[2].ctypes.data, n, p,
                                     reg2.ctypes.data))
            _lib.check(L.nkv_cms_insert(ctx.h, keys[0].ctypes.data, keys[1].ctypes.data, keys[2].ctypes.data, n, m,
                                        k, seed0, tab2.ctypes.data))
        assert np.array_equal(c_reg(), want_reg), path
        assert np.array_equal(c_tab().view(np.uint32).reshape(k, m), want_tab), path
        assert np.array_equal(reg, want_reg) and np.array_equal(reg2, want_reg), path
        assert np.array_equal(tab, want_tab) and np.array_equal(tab2, want_tab), path
    out = np.zeros(n, np.uint32)
    _lib.check(L.nkv_cms_query(ctx.h, keys[0].ctypes.data, keys[1].ctypes.data, keys[2].ctypes.data, n, m, k, seed0,
                               want_tab.ctypes.data, out.ctypes.data))
    assert np.array_equal(out, ref.cms_query_many(want_tab, *keys, seed0))
    for check in intact:
        check()


def test_records_header_outside_the_stream(sk):
    """The last record's KeySize reaches outside the stream: NKV_ERR_INVALID
    from every records form.  The host forms leave the caller's registers and
    table as they were.  The device forms have no copy to discard: the bad
    record contributes nothing (the filter's rule), the others are in."""
    _lib, ctx, L = sk
    stream, sizes, keys = _records()
    n = sizes.size
    buf = np.frombuffer(stream, np.uint8).copy()
    last = int(sizes[:-1].sum())
    buf[last + 14:last + 22] = np.frombuffer(np.uint64(1 << 40).tobytes(), np.uint8)
    rec_off = np.zeros(n, np.uint64)
    rec_off[1:] = np.cumsum(sizes[:-1])
    p, m, k, seed0 = 11, 28, 3, 5
    rng = np.random.default_rng(8)
    reg0 = rng.integers(0, 5, 1 << p).astype(np.uint8)
    tab0 = rng.integers(0, 100, (k, m)).astype(np.uint32)
    d_stream, d_off = _dev(buf), _dev(rec_off)
    _torch().cuda.synchronize()
    head = tuple(a[:n - 1] for a in keys[1:])
    want_reg = ref.hll_add_many(reg0, keys[0], *head, p)
    want_tab = ref.cms_insert_many(tab0, keys[0], *head, seed0)
    for path in PATHS:
        with _Path(sk, path):
            reg, tab = reg0.copy(), tab0.copy()
            assert L.nkv_hll_add_records(ctx.h, buf.ctypes.data, buf.size, sizes.ctypes.data, n, p,
                                         reg.ctypes.data) == INVALID
            assert L.nkv_cms_insert_records(ctx.h, buf.ctypes.data, buf.size, sizes.ctypes.data, n, m, k, seed0,
                                            tab.ctypes.data) == INVALID
            assert np.array_equal(reg, reg0) and np.array_equal(tab, tab0), path
            p_reg, c_reg = guarded(1 << p, 4, init=reg0)
            p_tab, c_tab = guarded(4 * m * k, 4, init=tab0)
            assert L.nkv_hll_add_records_dev(ctx.h, d_stream.data_ptr(), buf.size, d_off.data_ptr(), n, p,
                                             p_reg) == INVALID
            assert L.nkv_cms_insert_records_dev(ctx.h, d_stream.data_ptr(), buf.size, d_off.data_ptr(), n, m, k,
                                                seed0, p_tab) == INVALID
            ctx.sync()
        assert np.array_equal(c_reg(), want_reg), path
        assert np.array_equal(c_tab().view(np.uint32).reshape(k, m), want_tab), path
    # a record offset past the stream, and a stream too short for one header
    d_bad = _dev(np.array([0, buf.size - 10], np.uint64))
    _torch().cuda.synchronize()
    p_reg, c_reg = guarded(16, 4, init=np.zeros(16, np.uint8))
    assert L.nkv_hll_add_records_dev(ctx.h, d_stream.data_ptr(), 20, d_bad.data_ptr(), 2, 4, p_reg) == INVALID
    ctx.sync()
    assert not c_reg().any()
    # the context stays usable
    reg = np.zeros(1 << p, np.uint8)
    good = np.frombuffer(stream, np.uint8)
    _lib.check(L.nkv_hll_add_records(ctx.h, good.ctypes.data, good.size, sizes.ctypes.data, n, p, reg.ctypes.data))
    assert np.array_equal(reg, ref.hll_add_many(np.zeros(1 << p, np.uint8), *keys, p))


# ---------------------------------------------------------------------------
# buffer contract and argument rules

def test_outputs_at_minimum_alignment_between_guards(sk):
    """d_reg at P = 4 (16 bytes), d_table at (28, 3) and the query's d_out, each
    4 bytes past a 256-byte boundary between guard bytes; inputs unchanged."""
    keys = _keys(5000)
    dkeys = _upload(keys)
    intact = [frozen(t) for t in dkeys]
    for path in PATHS:
        got = _hll_dev(sk, path, dkeys, 5000, 4, np.zeros(16, np.uint8), at=4)
        assert np.array_equal(got, ref.hll_add_many(np.zeros(16, np.uint8), *keys, 4))
        tab = _cms_dev(sk, path, dkeys, 5000, 28, 3, 17, np.zeros((3, 28), np.uint32), at=4)
        assert np.array_equal(tab, ref.cms_insert_many(np.zeros((3, 28), np.uint32), *keys, 17))
    got = _cms_query_dev(sk, dkeys, 5000, 28, 3, 17, tab, at=4)
    assert np.array_equal(got, ref.cms_query_many(tab, *keys, 17))
    for check in intact:
        check()


def test_argument_rules(sk):
    _lib, ctx, L = sk
    keys = _keys(64)
    d = _upload(keys)
    k0, k1, k2 = (t.data_ptr() for t in d)
    p_reg, c_reg = guarded(16, 4, init=np.zeros(16, np.uint8))
    p_tab, c_tab = guarded(4 * 84, 4, init=np.zeros(4 * 84, np.uint8))
    p_out, c_out = guarded(4 * 64, 4)
    big_n = 2**31
    for p in (3, 17, -1, 0):
        assert L.nkv_hll_add_dev(ctx.h, k0, k1, k2, 64, p, p_reg) == INVALID
        assert L.nkv_hll_add_records_dev(ctx.h, k0, 100, k1, 1, p, p_reg) == INVALID
    assert L.nkv_hll_add_dev(ctx.h, k0, k1, k2, 64, 4, None) == INVALID
    assert L.nkv_hll_add_dev(ctx.h, k0, k1, k2, big_n, 4, p_reg) == INVALID
    assert L.nkv_hll_add_dev(ctx.h, None, k1, k2, 64, 4, p_reg) == INVALID
    assert L.nkv_hll_add_dev(ctx.h, None, None, None, 0, 4, p_reg) == 0  # n = 0 after the checks: nothing touched
    assert L.nkv_hll_add_records_dev(ctx.h, None, 0, None, 0, 4, p_reg) == 0
    for m, k in ((0, 3), (28, 0), (2**31 - 1, 2), (65536, 32768)):
        assert L.nkv_cms_insert_dev(ctx.h, k0, k1, k2, 64, m, k, 0, p_tab) == INVALID
        assert L.nkv_cms_insert_records_dev(ctx.h, k0, 100, k1, 1, m, k, 0, p_tab) == INVALID
        assert L.nkv_cms_query_dev(ctx.h, k0, k1, k2, 64, m, k, 0, p_tab, p_out) == INVALID
    assert L.nkv_cms_insert_dev(ctx.h, k0, k1, k2, 64, 28, 3, 0, None) == INVALID
    assert L.nkv_cms_insert_dev(ctx.h, k0, k1, k2, big_n, 28, 3, 0, p_tab) == INVALID
    assert L.nkv_cms_query_dev(ctx.h, k0, k1, k2, 64, 28, 3, 0, p_tab, None) == INVALID
    assert L.nkv_cms_query_dev(ctx.h, k0, k1, k2, 64, 28, 3, 0, None, p_out) == INVALID
    assert L.nkv_cms_query_dev(ctx.h, k0, k1, k2, big_n, 28, 3, 0, p_tab, p_out) == INVALID
    assert L.nkv_cms_insert_dev(ctx.h, None, None, None, 0, 28, 3, 0, p_tab) == 0
    assert L.nkv_cms_query_dev(ctx.h, None, None, None, 0, 28, 3, 0, p_tab, None) == 0
    reg, tab = np.zeros(16, np.uint8), np.zeros(84, np.uint32)
    assert L.nkv_hll_add(ctx.h, None, None, None, 0, 4, reg.ctypes.data) == 0
    assert L.nkv_hll_add(ctx.h, None, None, None, 0, 4, None) == INVALID
    assert L.nkv_cms_insert(ctx.h, None, None, None, 0, 28, 3, 0, tab.ctypes.data) == 0
    assert L.nkv_cms_insert(ctx.h, None, None, None, 0, 0, 3, 0, tab.ctypes.data) == INVALID
    ctx.sync()
    assert not c_reg().any() and not c_tab().any() and (c_out() == 0xA5).all()
    for bad in (-1, 3):
        with pytest.raises(_lib.NkvError):
            ctx.set_option(_lib.NKV_OPT_SKETCH_PATH, bad)


# ---------------------------------------------------------------------------
# mirrors

def test_mirrors_reproduce_the_reference_demos(nkv):
    """cmsketch.go main(): insert {1,2} twice and {3,4} once, query {1,2},
    {3,4}, {2,5}; wrappereng.go's HLL at P = 4."""
    from nakevaleng_amd import sketch
    _lib, ctx = nkv
    seed = 1640995200
    cms = sketch.NewCMS(0.1, 0.1, seed=seed, ctx=ctx)
    assert (cms.K, cms.M) == (3, 28) and cms.HashSeeds == [seed, seed + 1, seed + 2]
    c = ref.CMSRef(28, 3, seed)
    for e in (bytes([1, 2]), bytes([1, 2]), bytes([3, 4])):
        cms.Insert(e)
        c.Insert(e)
    assert cms.Contents.tolist() == c.Contents
    for e in (bytes([1, 2]), bytes([3, 4]), bytes([2, 5])):
        assert cms.Query(e) == c.Query(e)
    assert cms.Query(bytes([1, 2])) >= 2 and cms.Query(bytes([3, 4])) >= 1
    assert cms.EncodeToDict() == {"M": 28, "K": 3, "HashSeeds": [seed, seed + 1, seed + 2], "Contents": c.Contents}
    again = sketch.CountMinSketch(cms.M, cms.K, cms.HashSeeds, cms.Contents, ctx=ctx)  # DecodeFromBytes' shape
    many = [bytes([1, 2]), bytes([3, 4]), bytes([2, 5]), b"", b"absent"]
    assert again.QueryMany(many).tolist() == [c.Query(e) for e in many]
    assert again.QueryMany([]).size == 0

    hll = sketch.New(4, ctx=ctx)
    h = ref.HLLRef(4)
    assert (hll.M, hll.P, hll.Reg) == (16, 4, bytes(16))
    words = [b"key%d" % i for i in range(10)] + [b"", b"key3"]
    for w in words[:5]:
        hll.Add(w)
    hll.AddMany(words[5:])
    for w in words:
        h.Add(w)
    assert hll.Reg == bytes(h.Reg)
    assert hll.Estimate() == h.Estimate() and hll.EstimateStandard() == h.EstimateStandard()
    assert hll.EncodeToDict() == {"M": 16, "P": 4, "Reg": bytes(h.Reg)}
    hll.Add(b"one more")  # a second batch max-es into the same registers
    h.Add(b"one more")
    assert hll.Reg == bytes(h.Reg)


def test_key_sketches_resident_equals_table(nkv):
    from nakevaleng_amd import lsmtree, sstable
    _lib, ctx = nkv
    stream, sizes, keys = _records()
    table = (stream, sizes)
    want_reg = ref.hll_add_many(np.zeros(1 << 12, np.uint8), *keys, 12)
    want_tab = ref.cms_insert_many(np.zeros((5, 2719), np.uint32), *keys, 321)
    resident = lsmtree.upload_table(table)
    results = [lsmtree.key_sketches(table, precision=12, cms=(0.001, 0.01), seed=321),
               lsmtree.key_sketches(resident, precision=12, cms=(0.001, 0.01), seed=321),
               sstable.key_sketches_from_records(stream, sizes, precision=12, cms=(0.001, 0.01), seed=321, ctx=ctx)]
    for hll, cms in results:
        assert (hll.P, hll.M) == (12, 4096) and hll.Reg == want_reg.tobytes()
        assert (cms.M, cms.K) == (2719, 5) and cms.HashSeeds == [321 + i for i in range(5)]
        assert np.array_equal(cms.Contents, want_tab)
    hll, cms = lsmtree.key_sketches(resident, precision=12)
    assert cms is None and hll.Reg == want_reg.tobytes()
    assert abs(hll.EstimateStandard() - len(set(map(bytes, (keys[0][int(o):int(o + l)].tobytes()
                                                            for o, l in zip(keys[1], keys[2])))))) < 0.1 * 2000
    hll, cms = lsmtree.key_sketches(resident, cms=(0.1, 0.1), seed=9)
    assert hll is None and np.array_equal(cms.Contents, ref.cms_insert_many(np.zeros((3, 28), np.uint32), *keys, 9))
