"""CPU: tests/sketch_ref.py, the restatement of ds/hll and ds/cmsketch, pinned by
hand-derived cases; its batch forms held to its per-key classes; and the two
pure host functions of the library (nkv_hll_estimate, nkv_cms_params) held to
the restatement.  No device is needed."""
import ctypes
import math

import numpy as np
import pytest

from tests import sketch_ref as ref


@pytest.fixture(scope="module")
def L():
    from nakevaleng_amd import build as b
    b.build(quiet=True)
    from nakevaleng_amd import _lib
    return _lib.lib()


def _spans(keys):
    ln = np.array([len(k) for k in keys], np.uint64)
    off = np.zeros(len(keys), np.uint64)
    off[1:] = np.cumsum(ln[:-1])
    return np.frombuffer(b"".join(keys) + b"\0", np.uint8), off, ln


def test_empty_key_sets_register_0_to_33(oracle):
    assert oracle.murmur3_32(b"", 0) == 0
    assert ref.trailing_zeros32(0) == 32 and ref.trailing_zeros32(1) == 0 and ref.trailing_zeros32(0x80000000) == 31
    for p in (4, 10, 16):
        h = ref.HLLRef(p)
        h.Add(b"")
        assert h.Reg[0] == 33 and h.emptyCount() == h.M - 1
        h.Add(b"")
        assert h.Reg[0] == 33


def test_add_follows_the_hash(oracle):
    h = ref.HLLRef(11)
    for key in (b"a", b"nakevaleng", bytes(range(40))):
        v = oracle.murmur3_32(key, 0)
        before = h.Reg[v >> 21]
        h.Add(key)
        assert h.Reg[v >> 21] == max(before, 1 + ref.trailing_zeros32(v))


def test_estimate_one_register_at_p4():
    """One register at 1, fifteen at 0: sum = 255^2, the raw estimate about
    0.0027 < 2.5 * 16 with empty registers, so Estimate() = 16 ln(16 / 15)."""
    h = ref.HLLRef(4)
    h.Reg[7] = 1
    alpha = 0.7213 / (1.0 + 1.079 / 16.0)
    raw = alpha * 256.0 / (255.0 * 255.0)
    assert 0.0026 < raw < 0.0028
    assert h.Estimate() == 16.0 * math.log(16.0 / 15.0)
    assert h.EstimateStandard() == 16.0 * math.log(16.0 / 15.0)  # 16 alpha / 15.5 < 40 as well


def test_estimate_of_an_empty_hll_is_nan():
    for p in (4, 16):
        assert math.isnan(ref.HLLRef(p).Estimate())


def test_estimate_without_empty_registers_is_the_quirk():
    """Every register at 5: the reference's sum is M * 251^2, not M * 2^-5."""
    h = ref.HLLRef(4)
    h.Reg = [5] * 16
    alpha = 0.7213 / (1.0 + 1.079 / 16.0)
    assert h.Estimate() == alpha * 256.0 / (16 * 251.0 * 251.0)
    assert h.EstimateStandard() == alpha * 256.0 / (16 * 2.0 ** -5)


def test_precision_bounds():
    for p in (3, 17, -1):
        with pytest.raises(ValueError, match=f"precision must be between 4 and 16, but {p} was given"):
            ref.HLLRef(p)


def test_cms_sizing():
    assert (ref.calculateM(0.1), ref.calculateK(0.1)) == (28, 3)
    assert (ref.calculateM(0.001), ref.calculateK(0.01)) == (2719, 5)
    assert (ref.calculateM(0.0001), ref.calculateK(1e-6)) == (27183, 14)


def test_cms_counter_wraps_and_empty_query(oracle):
    c = ref.CMSRef(28, 3, 7)
    assert c.HashSeeds == [7, 8, 9]
    assert c.Query(b"never inserted") == 0
    key = b"\x01\x02"
    idx = [oracle.murmur3_32(key, 7 + i) % 28 for i in range(3)]
    c.Contents[1][idx[1]] = 0xFFFFFFFF
    c.Insert(key)
    assert [c.Contents[i][idx[i]] for i in range(3)] == [1, 0, 1]
    assert c.Query(key) == 0
    c.Insert(key)
    assert c.Query(key) == 1
    assert ref.CMSRef(5, 3, 2**32 - 1).HashSeeds == [2**32 - 1, 0, 1]


def test_batch_forms_equal_the_per_key_classes(oracle):
    rng = np.random.default_rng(0x736B31)
    keys = [b"", b"x" * 4097] + [rng.bytes(int(n)) for n in rng.integers(0, 41, 400)]
    keys += keys[5:60]  # repeats
    data, off, ln = _spans(keys)
    for seed in (0, 99, 2**32 - 1):
        got = ref.murmur3_32_many(data, off, ln, seed)
        assert got.tolist() == [oracle.murmur3_32(k, seed) for k in keys]
    for p in (4, 11, 16):
        h = ref.HLLRef(p)
        for k in keys:
            h.Add(k)
        assert ref.hll_add_many(np.zeros(1 << p, np.uint8), data, off, ln, p).tolist() == h.Reg
    for m, k, seed0 in ((1, 1, 0), (28, 3, 5), (3, 33, 2**32 - 2)):
        c = ref.CMSRef(m, k, seed0)
        for key in keys:
            c.Insert(key)
        table = ref.cms_insert_many(np.zeros((k, m), np.uint32), data, off, ln, seed0)
        assert table.tolist() == c.Contents
        assert ref.cms_query_many(table, data, off, ln, seed0).tolist() == [c.Query(key) for key in keys]
    pre = np.zeros((3, 28), np.uint32)
    pre[:] = 0xFFFFFFFF
    assert (ref.cms_insert_many(pre, data, off[:1], ln[:1], 5) == 0).sum() == 3  # wraps


def _estimate(L, reg, p, mode):
    out = ctypes.c_double(-1.0)
    rc = L.nkv_hll_estimate(reg.ctypes.data, p, mode, ctypes.byref(out))
    return rc, out.value


def _same_double(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


@pytest.mark.parametrize("p", [4, 10, 16])
def test_library_estimate_equals_the_restatement(L, p):
    rng = np.random.default_rng(p)
    M = 1 << p
    files = [np.zeros(M, np.uint8), np.full(M, 33, np.uint8), rng.integers(0, 34, M).astype(np.uint8),
             rng.integers(1, 20, M).astype(np.uint8),
             (rng.integers(0, 34, M) * (rng.random(M) < 0.1)).astype(np.uint8)]
    one = np.zeros(M, np.uint8)
    one[M // 2] = 1
    files.append(one)
    for reg in files:
        h = ref.HLLRef(p)
        h.Reg = reg.tolist()
        for mode, want in ((0, h.Estimate()), (1, h.EstimateStandard())):
            rc, got = _estimate(L, reg, p, mode)
            assert rc == 0
            assert _same_double(got, want), (mode, got, want)
    assert math.isnan(_estimate(L, files[0], p, 0)[1])


def test_library_estimate_refuses_bad_arguments(L):
    reg = np.zeros(16, np.uint8)
    out = ctypes.c_double(0)
    assert L.nkv_hll_estimate(reg.ctypes.data, 3, 0, ctypes.byref(out)) == 2
    assert L.nkv_hll_estimate(reg.ctypes.data, 17, 0, ctypes.byref(out)) == 2
    assert L.nkv_hll_estimate(reg.ctypes.data, 4, 2, ctypes.byref(out)) == 2
    assert L.nkv_hll_estimate(None, 4, 0, ctypes.byref(out)) == 2
    assert L.nkv_hll_estimate(reg.ctypes.data, 4, 0, None) == 2


def test_library_cms_params_equal_the_restatement(L):
    eps = [0.0, 1e-12, 1e-10, 6.4e-10, 1e-9, 1e-4, 0.001, 0.01, 0.1, 0.25, 0.5, 1.0, 1.0000001, 2.0, -0.1,
           math.nan, math.inf]
    dels = [0.0, 1e-300, 1e-9, 1e-6, 0.01, 0.1, 0.3678794411714423, 0.5, 0.9, 1.0 - 2**-53, 1.0, 1.5, -0.5,
            math.nan]
    for e in eps:
        for d in dels:
            m, k = ctypes.c_uint32(77), ctypes.c_uint32(77)
            rc = L.nkv_cms_params(e, d, ctypes.byref(m), ctypes.byref(k))
            if ref.cms_new_accepted(e, d):
                assert rc == 0 and (m.value, k.value) == (ref.calculateM(e), ref.calculateK(d)), (e, d)
                assert m.value >= 1 and k.value >= 1
            else:
                assert rc == 2 and (m.value, k.value) == (77, 77), (e, d)
    m = ctypes.c_uint32(0)
    assert L.nkv_cms_params(0.1, 0.1, None, ctypes.byref(m)) == 2
    assert L.nkv_cms_params(0.1, 0.1, ctypes.byref(m), None) == 2


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_estimate_standard_within_4_standard_errors(L, seed):
    """50,000 distinct keys at P = 14: within 4 * 1.04 / sqrt(M) = 3.25 % of the
    truth (the restatement alone on these keys: 0.46 %, 0.19 %, 0.22 % for seeds 0-2)."""
    p, n = 14, 50000
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 256, (n, 16), dtype=np.uint8)
    data[:, :4] = np.arange(n, dtype=np.uint32).view(np.uint8).reshape(n, 4)  # a counter: the keys are distinct
    data = data.reshape(-1)
    off, ln = np.arange(n, dtype=np.uint64) * 16, np.full(n, 16, np.uint64)
    reg = ref.hll_add_many(np.zeros(1 << p, np.uint8), data, off, ln, p)
    bound = 4 * 1.04 / math.sqrt(1 << p)
    assert abs(bound - 0.0325) < 1e-5
    h = ref.HLLRef(p)
    h.Reg = reg.tolist()
    assert abs(h.EstimateStandard() - n) / n <= bound
    rc, got = _estimate(L, reg, p, 1)
    assert rc == 0 and got == h.EstimateStandard()
    assert abs(got - n) / n <= bound
    from nakevaleng_amd import sketch
    mirror = sketch.HLL(1 << p, p, Reg=reg.tobytes())  # nothing pending: no device is touched
    assert mirror.EstimateStandard() == got
    assert _same_double(mirror.Estimate(), h.Estimate())


def test_mirror_refusals_need_no_device():
    from nakevaleng_amd import sketch
    for p in (3, 17):
        with pytest.raises(sketch.HLLError, match=f"precision must be between 4 and 16, but {p} was given"):
            sketch.New(p)
    with pytest.raises(sketch.CMSError, match="epsilon must be between"):
        sketch.NewCMS(1.5, 0.1)
    with pytest.raises(sketch.CMSError, match="delta must be between"):
        sketch.NewCMS(0.1, -0.5)
    for e, d in ((0.0, 0.1), (0.1, 0.0), (0.1, 1.0)):  # accepted by the reference, refused here
        with pytest.raises(sketch.CMSError):
            sketch.NewCMS(e, d)
    c = sketch.NewCMS(0.1, 0.1, seed=2**32 - 1)
    assert (c.M, c.K, c.HashSeeds) == (28, 3, [2**32 - 1, 0, 1])
    assert sketch.New(4).EncodeToDict() == {"M": 16, "P": 4, "Reg": bytes(16)}
