"""GPU: the record encoder over sources more than 4 GiB apart and over an
output longer than 4 GiB.

As in tests/test_gpu_far.py one allocation of far.ALLOC bytes is never filled
as a whole: a case uploads a few KiB into islands at far.BASES and every span
of every case, the output included, lies inside that one allocation
(tests/far.py's allocation rule), so an address built from a wrapped 32-bit
offset would read or write wrong bytes inside it, never unmapped memory.

The encoder's kernels (csrc/encode.hip) address everything with 64-bit
quantities and contain no near/far guard, so there are no two sides of one to
hold; each far case is compared with the reference and with its near twin, the
same compact layout uploaded contiguously into an ordinary small tensor.
"""
import ctypes
import struct
import zlib

import numpy as np
import pytest

from tests import far
from tests.encode_ref import encode_many_ref

pytestmark = pytest.mark.gpu

M16 = 1 << 24


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


def _batch(n=130):
    """n puts, value lengths cycling through far.RAGGED, key lengths through 0..33."""
    rng = np.random.default_rng(0x66617233)
    keys = [rng.bytes(i % 34) for i in range(n)]
    vals = [rng.bytes(far.RAGGED[(i + i // 3) % len(far.RAGGED)]) for i in range(n)]
    ts = rng.integers(-2**62, 2**62, n)
    return keys, vals, ts, (np.arange(n) & 1).astype(np.uint8), ((np.arange(n) * 5) & 0xFF).astype(np.uint8)


def _encode(nkv, p_keys, keys_len, koff, klen, p_vals, vals_len, voff, vlen, ts, status, type_info, nbytes):
    """The device call over arrays given on the host; returns (stream, offsets, checksums)."""
    torch = _torch()
    _lib, ctx = nkv
    n = len(koff)
    held = [_dev(np.asarray(x, np.uint64)) for x in (koff, klen, voff, vlen)]
    held += [_dev(np.asarray(ts, np.int64)), _dev(status), _dev(type_info)]
    puts = _lib.NkvPuts(p_keys, keys_len, held[0].data_ptr(), held[1].data_ptr(), p_vals, vals_len,
                        held[2].data_ptr(), held[3].data_ptr(), held[4].data_ptr(), 0, held[5].data_ptr(),
                        held[6].data_ptr(), n)
    d_out = torch.zeros(nbytes + 16, dtype=torch.uint8, device="cuda")
    d_off = torch.zeros(8 * n, dtype=torch.uint8, device="cuda")
    d_crc = torch.zeros(4 * n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    out_len = ctypes.c_uint64(0)
    _lib.check(_lib.lib().nkv_encode_records_dev(ctx.h, ctypes.byref(puts), d_out.data_ptr() + 3, nbytes,
                                                 d_off.data_ptr(), d_crc.data_ptr(), ctypes.byref(out_len)))
    torch.cuda.synchronize()
    assert out_len.value == nbytes
    return (d_out.cpu().numpy()[3:3 + nbytes].tobytes(), d_off.cpu().numpy().view(np.uint64),
            d_crc.cpu().numpy().view(np.uint32))


def _place(big, spans):
    """Upload [(offset in big, bytes)] and return a function that asserts they are unchanged."""
    torch = _torch()
    for at, data in spans:
        assert 0 <= at and at + len(data) <= far.ALLOC
        big[at:at + len(data)].copy_(torch.from_numpy(np.frombuffer(data, np.uint8).copy()))
    torch.cuda.synchronize()

    def unchanged():
        for at, data in spans:
            assert big[at:at + len(data)].cpu().numpy().tobytes() == data

    return unchanged


def _check(got, want):
    assert got[0] == want[0]
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])


def test_keys_in_island_0_values_in_island_1(nkv, big):
    keys, vals, ts, st, ty = _batch()
    want = encode_many_ref(keys, vals, ts, st, ty)
    kb, vb = b"".join(keys), b"".join(vals)
    klen, vlen = [len(k) for k in keys], [len(v) for v in vals]
    koff, voff = np.cumsum([0] + klen[:-1]), np.cumsum([0] + vlen[:-1])
    k_at, v_at = far.BASES[0] + 5, far.BASES[1] + 9
    unchanged = _place(big, [(k_at, kb), (v_at, vb)])
    got = _encode(nkv, big.data_ptr() + k_at, len(kb), koff, klen, big.data_ptr() + v_at, len(vb), voff, vlen, ts, st,
                  ty, len(want[0]))
    unchanged()
    _check(got, want)
    # the near twin: the same two blobs in ordinary small tensors
    d_k, d_v = _dev(np.frombuffer(b"\0" * 5 + kb, np.uint8)), _dev(np.frombuffer(b"\0" * 9 + vb, np.uint8))
    near = _encode(nkv, d_k.data_ptr() + 5, len(kb), koff, klen, d_v.data_ptr() + 9, len(vb), voff, vlen, ts, st, ty,
                   len(want[0]))
    _check(near, want)


def test_values_of_one_wave_alternate_between_two_islands(nkv, big):
    """Even puts take their value from island 0, odd ones from island 1: the
    values of neighbouring records, in one tile's list, lie more than 4 GiB
    apart inside the one value blob, whose offsets pass 2^32."""
    keys, vals, ts, st, ty = _batch()
    want = encode_many_ref(keys, vals, ts, st, ty)
    kb = b"".join(keys)
    klen, vlen = [len(k) for k in keys], [len(v) for v in vals]
    koff = np.cumsum([0] + klen[:-1])
    half = [b"".join(vals[0::2]), b"".join(vals[1::2])]
    cur, voff_near, voff_far = [0, 0], [], []
    gap = len(half[0]) + 64  # the near twin: island 1's bytes right behind island 0's
    for i, v in enumerate(vals):
        voff_far.append((far.BASES[1] if i % 2 else 7) + cur[i % 2])
        voff_near.append((gap if i % 2 else 7) + cur[i % 2])
        cur[i % 2] += len(v)
    k_at = far.BASES[0] + (1 << 20)  # keys in island 0 too, past the even values
    assert 7 + len(half[0]) < (1 << 20) and max(voff_far) > far.G32
    unchanged = _place(big, [(7, half[0]), (far.BASES[1], half[1]), (k_at, kb)])
    vals_len = far.BASES[1] + len(half[1])
    got = _encode(nkv, big.data_ptr() + k_at, len(kb), koff, klen, big.data_ptr(), vals_len, voff_far, vlen, ts, st,
                  ty, len(want[0]))
    unchanged()
    _check(got, want)
    compact = b"\0" * 7 + half[0] + b"\0" * (gap - 7 - len(half[0])) + half[1]
    d_k, d_v = _dev(np.frombuffer(kb, np.uint8)), _dev(np.frombuffer(compact, np.uint8))
    near = _encode(nkv, d_k.data_ptr(), len(kb), koff, klen, d_v.data_ptr(), len(compact), voff_near, vlen, ts, st, ty,
                   len(want[0]))
    _check(near, want)


def test_output_offsets_past_4_gib(nkv, big):
    """258 records that share one 16 MiB value span and one key: out_len passes
    2^32 + 2^24, verified on the device.  Sources and output lie in the one
    allocation; the inputs are compact as they are, so the case is its own near
    twin on the input side."""
    torch = _torch()
    _lib, ctx = nkv
    rng = np.random.default_rng(0x66617234)
    n, key = 258, b"the one key"
    value = rng.bytes(M16)
    size = 30 + len(key) + M16
    total = n * size
    assert total > far.G32 + M16
    v_at, k_at, out_at = 64, 64 + M16 + 13, 2 * M16 + 5
    assert out_at + total + 4096 <= far.ALLOC
    unchanged = _place(big, [(v_at, value), (k_at, key)])
    held = [_dev(np.full(n, 0, np.uint64)), _dev(np.full(n, len(key), np.uint64)), _dev(np.full(n, 0, np.uint64)),
            _dev(np.full(n, M16, np.uint64)), _dev(np.arange(n, dtype=np.int64) - 100)]
    puts = _lib.NkvPuts(big.data_ptr() + k_at, len(key), held[0].data_ptr(), held[1].data_ptr(),
                        big.data_ptr() + v_at, M16, held[2].data_ptr(), held[3].data_ptr(), held[4].data_ptr(), 0,
                        None, None, n)
    d_off = torch.zeros(8 * n, dtype=torch.uint8, device="cuda")
    d_crc = torch.zeros(4 * n, dtype=torch.uint8, device="cuda")
    big[out_at - 64:out_at].fill_(0xA5)
    big[out_at + total:out_at + total + 64].fill_(0xA5)
    torch.cuda.synchronize()
    out_len = ctypes.c_uint64(0)
    _lib.check(_lib.lib().nkv_encode_records_dev(ctx.h, ctypes.byref(puts), big.data_ptr() + out_at, total,
                                                 d_off.data_ptr(), d_crc.data_ptr(), ctypes.byref(out_len)))
    torch.cuda.synchronize()
    assert out_len.value == total
    unchanged()
    assert bool((big[out_at - 64:out_at] == 0xA5).all()) and bool((big[out_at + total:out_at + total + 64] == 0xA5).all())
    off = d_off.cpu().numpy().view(np.uint64)
    assert np.array_equal(off, np.arange(n, dtype=np.uint64) * np.uint64(size))
    crc = zlib.crc32(key + value)
    assert (d_crc.cpu().numpy().view(np.uint32) == crc).all()
    mark = far.G32 // size  # the record that holds output byte 2^32
    assert 0 < mark < n - 1 and mark * size <= far.G32 < (mark + 1) * size
    d_value = big[v_at:v_at + M16]
    for i in (0, mark - 1, mark, mark + 1, n - 1):
        at = out_at + i * size
        head = big[at:at + 30 + len(key)].cpu().numpy().tobytes()
        assert head == struct.pack("<IqBBQQ", crc, i - 100, 0, 0, len(key), M16) + key, i
        assert torch.equal(big[at + 30 + len(key):at + size], d_value), i
