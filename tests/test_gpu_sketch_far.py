"""GPU: the sketches over keys more than 4 GiB apart.

As in tests/test_gpu_encode_far.py one allocation of far.ALLOC bytes is never
filled as a whole: a case uploads a few KiB into islands at far.BASES, and every
key of every case lies inside that one allocation (tests/far.py's allocation
rule), so an address built from a wrapped 32-bit offset would read wrong bytes
inside it, never unmapped memory.

The sketch kernels (csrc/sketch.hip) address every key with 64-bit quantities
and contain no near/far guard, so there are no two sides of one to hold; each
far case is compared with tests/sketch_ref.py over the compact layout and with
its near twin, the same compact layout uploaded into an ordinary small tensor.
Key i lies in island i % 3, so any 64 consecutive keys -- one wave of either
tier -- touch all three islands.
"""
import numpy as np
import pytest

from tests import far
from tests import sketch_ref as ref

pytestmark = pytest.mark.gpu

N = 390  # two workgroups of the direct tier


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible device"
    return torch


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


@pytest.fixture(scope="module")
def big():
    """The one big allocation.  Never filled as a whole; a failed allocation fails the tests."""
    torch = _torch()
    buf = torch.empty(far.ALLOC, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    yield buf
    del buf
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def case(big):
    """N ragged keys dealt to the three islands at every byte alignment, uploaded
    far (into `big`) and near; returns what both tests share."""
    torch = _torch()
    rng = np.random.default_rng(0x66617235)
    lens = rng.integers(0, 41, N).astype(np.uint64)
    lens[:4] = [1000, 4097, 3, 0]
    off, ranges = far.deal(lens, np.arange(N) % 4, 3, align=4)
    islands = [(s, e, far.BASES[k]) for k, (s, e) in enumerate(ranges)]
    compact = rng.integers(0, 256, ranges[-1][1], dtype=np.uint8)
    far_off, uploads = far.place(off, lens, islands)
    assert int(far_off.max()) - int(far_off.min()) > 2 * far.G32
    for w in range(0, N - 63):
        assert int(far_off[w:w + 64].max()) - int(far_off[w:w + 64].min()) > far.G32
    spans = []
    for base, sl in uploads:
        chunk = compact[sl]
        assert 0 <= base and base + chunk.size <= far.ALLOC
        big[base:base + chunk.size].copy_(torch.from_numpy(chunk.copy()))
        spans.append((base, chunk.tobytes()))
    d_near = [_dev(compact), _dev(off), _dev(lens)]
    d_far_off = _dev(far_off)
    torch.cuda.synchronize()

    def unchanged():
        for base, data in spans:
            assert big[base:base + len(data)].cpu().numpy().tobytes() == data

    return {"keys": (compact, off, lens), "near": d_near, "far_off": d_far_off, "unchanged": unchanged}


def _paths(nkv, run):
    _lib, ctx = nkv
    out = []
    try:
        for path in (0, 1, 2):
            ctx.set_option(_lib.NKV_OPT_SKETCH_PATH, path)
            out.append(run())
    finally:
        ctx.set_option(_lib.NKV_OPT_SKETCH_PATH, 0)
    return out


def test_hll_keys_of_one_call_4_gib_apart(nkv, big, case):
    torch = _torch()
    _lib, ctx = nkv
    L = _lib.lib()
    p = 11
    want = ref.hll_add_many(np.zeros(1 << p, np.uint8), *case["keys"], p)

    def run(d_keys, d_off):
        def go():
            d_reg = torch.zeros(1 << p, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            _lib.check(L.nkv_hll_add_dev(ctx.h, d_keys, d_off.data_ptr(), case["near"][2].data_ptr(), N, p,
                                         d_reg.data_ptr()))
            ctx.sync()
            return d_reg.cpu().numpy()
        return go

    for got in _paths(nkv, run(big.data_ptr(), case["far_off"])):
        assert np.array_equal(got, want)
    case["unchanged"]()
    for got in _paths(nkv, run(case["near"][0].data_ptr(), case["near"][1])):  # the near twin
        assert np.array_equal(got, want)


def test_cms_keys_of_one_call_4_gib_apart(nkv, big, case):
    torch = _torch()
    _lib, ctx = nkv
    L = _lib.lib()
    m, k, seed0 = 2719, 5, 0xFA5
    want = ref.cms_insert_many(np.zeros((k, m), np.uint32), *case["keys"], seed0)
    want_q = ref.cms_query_many(want, *case["keys"], seed0)

    def run(d_keys, d_off):
        def go():
            d_tab = torch.zeros(4 * m * k, dtype=torch.uint8, device="cuda")
            d_out = torch.zeros(4 * N, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            _lib.check(L.nkv_cms_insert_dev(ctx.h, d_keys, d_off.data_ptr(), case["near"][2].data_ptr(), N, m, k,
                                            seed0, d_tab.data_ptr()))
            _lib.check(L.nkv_cms_query_dev(ctx.h, d_keys, d_off.data_ptr(), case["near"][2].data_ptr(), N, m, k,
                                           seed0, d_tab.data_ptr(), d_out.data_ptr()))
            ctx.sync()
            return d_tab.cpu().numpy().view(np.uint32).reshape(k, m), d_out.cpu().numpy().view(np.uint32)
        return go

    for tab, q in _paths(nkv, run(big.data_ptr(), case["far_off"])):
        assert np.array_equal(tab, want) and np.array_equal(q, want_q)
    case["unchanged"]()
    for tab, q in _paths(nkv, run(case["near"][0].data_ptr(), case["near"][1])):  # the near twin
        assert np.array_equal(tab, want) and np.array_equal(q, want_q)
