"""GPU: framing a stream whose offsets pass 2^32.

One stream inside one allocation of far.ALLOC bytes, filled on the device by
nkv_fill_splitmix64_dev; a handful of headers and keys are then written into
it so that it reads: a few small records, one record whose Value is longer
than 4 GiB (the fill's bytes as they lie), a few small records behind it, and
the end of the stream.  The offsets of the records behind the long one, the
segment offsets, seg_first, seg_len and the stats all need more than 32 bits.
Expected values follow from the construction (the host never holds the
stream); both paths must give them, compared as 64-bit numbers.  Whatever the
fill's bytes decode to inside the long Value lies on no chain that starts at a
segment start, so it cannot change the answer.
"""
import ctypes
import struct

import numpy as np
import pytest

from tests import far

pytestmark = pytest.mark.gpu

NONE = 2**64 - 1
VALUE = far.G32 + (1 << 20) + 5  # the long record's Value
BASE_AT = 3  # the stream's base, bytes past the allocation's start


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible device"
    return torch


@pytest.fixture(scope="module")
def placed(nkv):
    """The allocation with the stream in it: (tensor, stream length, record offsets)."""
    torch = _torch()
    _lib, ctx = nkv
    small = [(b"k%d" % i, 40 + 7 * i) for i in range(6)]  # (key, Value length): three in front, three behind
    heads, at = [], 0
    for i, (key, vlen) in enumerate(small[:3] + [(b"the long one", VALUE)] + small[3:]):
        heads.append((at, struct.pack("<IqBBQQ", 0, i, 0, 0, len(key), vlen) + key))
        at += 30 + len(key) + vlen
    length = at
    assert length > far.G32 and BASE_AT + length + 64 <= far.ALLOC
    buf = torch.empty(far.ALLOC, dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib().nkv_fill_splitmix64_dev(ctx.h, buf.data_ptr(), BASE_AT + length + 64, 0x6672616D65))
    ctx.sync()
    for off, head in heads:
        buf[BASE_AT + off:BASE_AT + off + len(head)].copy_(torch.from_numpy(np.frombuffer(head, np.uint8).copy()))
    torch.cuda.synchronize()
    yield buf, length, [off for off, _ in heads]
    del buf
    torch.cuda.empty_cache()


def _frame(nkv, buf, length, seg, path):
    torch = _torch()
    _lib, ctx = nkv
    S = 0 if seg is None else len(seg)
    d_seg = torch.from_numpy(np.asarray(seg if S else [0], np.uint64).view(np.uint8).copy()).cuda()
    d_off = torch.full((8 * 16,), 0xA5, dtype=torch.uint8, device="cuda")
    d_first = torch.full((8 * (S + 2),), 0xA5, dtype=torch.uint8, device="cuda")
    d_len = torch.full((8 * (S + 1),), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    n_out, stats = ctypes.c_uint64(0), (ctypes.c_uint64 * 4)()
    ctx.set_option(_lib.NKV_OPT_FRAME_PATH, path)
    try:
        _lib.check(_lib.lib().nkv_frame_records_dev(ctx.h, buf.data_ptr() + BASE_AT, length,
                                                    d_seg.data_ptr() if S else None, S, _lib.NKV_FRAME_STRICT,
                                                    d_off.data_ptr(), 16, d_first.data_ptr(), d_len.data_ptr(),
                                                    ctypes.byref(n_out), stats))
        took = ctx.last_path()
    finally:
        ctx.set_option(_lib.NKV_OPT_FRAME_PATH, 0)
    torch.cuda.synchronize()
    u64 = lambda t: t.cpu().numpy().view(np.uint64)
    return n_out.value, [int(x) for x in stats], u64(d_off), u64(d_first), u64(d_len), took


@pytest.mark.parametrize("path", [1, 2], ids=["walk", "speculative"])
def test_offsets_past_4_gib(nkv, placed, path):
    _lib = nkv[0]
    buf, length, offs = placed
    assert offs[4] > far.G32
    n, stats, off, first, _, took = _frame(nkv, buf, length, None, path)
    assert took == (_lib.NKV_PATH_FRAME_WALK if path == 1 else _lib.NKV_PATH_FRAME_SPECULATIVE)
    assert n == 7 and stats == [7, length, 0, NONE]
    assert [int(x) for x in off[:7]] == offs
    assert (off[7:] == np.uint64(0xA5A5A5A5A5A5A5A5)).all()
    assert int(first[0]) == 7


@pytest.mark.parametrize("path", [1, 2], ids=["walk", "speculative"])
def test_segments_past_4_gib(nkv, placed, path):
    """Segments cut at the record starts, the long record alone in its own, an
    empty one past 2^32 and one at the stream's end."""
    buf, length, offs = placed
    seg = [0, offs[3], offs[4], offs[4], offs[6], length]
    n, stats, off, first, seg_len, _ = _frame(nkv, buf, length, seg, path)
    assert n == 7 and stats == [7, length, 0, NONE]
    assert [int(x) for x in off[:7]] == offs
    assert [int(x) for x in first[:7]] == [0, 3, 4, 4, 6, 7, 7]
    ends = seg[1:] + [length]
    assert [int(x) for x in seg_len[:6]] == [e - a for a, e in zip(seg, ends)]
    assert int(seg_len[1]) > far.G32
