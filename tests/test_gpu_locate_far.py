"""GPU: nkv_index_open_dev and nkv_locate_dev with their buffers more than
4 GiB apart.

One allocation of far.ALLOC bytes holds everything, as in tests/far.py: the
Index images near its start, the Summaries and the query keys past 2^32, the
entry offsets and every locate output past 2^33.  Every address the kernels form --
a Summary entry's link into the Index, a probed key, an output slot -- then
needs the full 64 bits, and one built from a wrapped 32-bit difference would
still land inside the allocation: wrong bytes, never unmapped memory.  The
allocation is never filled as a whole; only the placed bytes are uploaded.

Each case is held to tests/index_open_ref.py and to its near twin: the same
images and queries in ordinary small tensors, whose bytes must be the same.
"""
import ctypes

import numpy as np
import pytest

from tests import far
from tests import index_open_ref as ref
from tests.test_gpu_locate import _dev, dev_locate, dev_open, make_world, pack_keys, queries_of, upload, want_of

pytestmark = pytest.mark.gpu

MiB = 1 << 20


@pytest.fixture(scope="module")
def big():
    """The one big allocation.  Never filled as a whole; a failed allocation fails the tests."""
    import torch
    buf = torch.empty(far.ALLOC, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    yield buf
    del buf
    torch.cuda.empty_cache()


def put(big, at, data):
    """Upload `data` (bytes or array) at byte `at` of the allocation; returns its address and a check that it is unchanged."""
    import torch
    host = np.frombuffer(bytes(data), np.uint8).copy() if isinstance(data, (bytes, bytearray)) \
        else np.ascontiguousarray(data).view(np.uint8).copy()
    assert at + host.size <= far.ALLOC
    big[at:at + host.size].copy_(torch.from_numpy(host))
    torch.cuda.synchronize()

    def unchanged():
        assert np.array_equal(big[at:at + host.size].cpu().numpy(), host)

    return big.data_ptr() + at, unchanged


def take(big, at, nbytes, fill=0xA5):
    """An output region: nbytes at `at` with 64 guard bytes on both sides, all holding `fill`."""
    big[at - 64:at + nbytes + 64].fill_(fill)

    def read():
        got = big[at - 64:at + nbytes + 64].cpu().numpy()
        assert (got[:64] == fill).all() and (got[64 + nbytes:] == fill).all()
        return got[64:64 + nbytes].copy()

    return big.data_ptr() + at, read


@pytest.mark.parametrize("path", [1, 2])
def test_open_and_locate_4_gib_apart(nkv, oracle, big, path):
    import torch
    _lib, ctx = nkv
    L = _lib.lib()
    w = make_world(oracle, 0x4A00 + path, (300, 65), ("real", None))
    queries = queries_of(w, 130) + w.tabs[0][0][:40]
    q, T = len(queries), 2
    # three regions of at most 64 MiB, each more than 4 GiB from the next
    B0, C0 = far.G32 + 64 * MiB, 2 * far.G32 + 256 * MiB
    assert B0 - 64 * MiB >= far.G32 and C0 - (B0 + 64 * MiB) > far.G32 and C0 + 64 * MiB <= far.ALLOC
    i_at = (256 + 1, 8 * MiB + 7)        # the two Index images
    s_at = (B0 + 3, B0 + 8 * MiB + 15)   # the Summaries (and, below, the query keys)
    e_at = (C0, C0 + 8 * MiB)            # the entry offsets (and every locate output)

    structs = (_lib.NkvIndexTable * T)()
    same, far_ent = [], []
    ctx.set_option(_lib.NKV_OPT_INDEX_OPEN_PATH, path)
    ctx.set_option(_lib.NKV_OPT_INDEX_OPEN_CHUNK, 64 if path == 2 else 0)  # many chunks per table
    try:
        for t, (index, summary) in enumerate(w.pairs):
            want_ent, n, s, _ = ref.open(index, summary)
            p_i, ok_i = put(big, i_at[t], index)
            p_s, ok_s = put(big, s_at[t], summary)
            p_e, read_e = take(big, e_at[t], 8 * n)
            torch.cuda.synchronize()
            gn, gs, v = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint32(0)
            assert L.nkv_index_open_dev(ctx.h, p_i, len(index), p_s, len(summary), p_e, n, ctypes.byref(gn),
                                        ctypes.byref(gs), ctypes.byref(v)) == 0
            ctx.sync()
            assert (gn.value, gs.value, v.value) == (n, s, 0)
            ent = read_e()
            assert ent.view(np.uint64).tolist() == want_ent
            ok_i(), ok_s()
            f = w.filters[t]
            d_bits = _dev(f.words()) if f is not None else None
            same += [ok_i, d_bits]
            structs[t] = _lib.NkvIndexTable(p_i, len(index), p_e, n, d_bits.data_ptr() if f else None,
                                            f.m if f else 0, f.k if f else 0, f.seed0 if f else 0)
            far_ent.append(ent.tobytes())
    finally:
        ctx.set_option(_lib.NKV_OPT_INDEX_OPEN_PATH, 0)
        ctx.set_option(_lib.NKV_OPT_INDEX_OPEN_CHUNK, 0)
    for (index, summary), far_bytes in zip(w.pairs, far_ent):  # the near twin writes the same bytes
        rc, ent, n, s, v, whole = dev_open(nkv, index, summary, path, 64 if path == 2 else 0)
        assert rc == 0 and whole[:n].tobytes() == far_bytes

    # locate: the keys in the second region, every output in the third
    host, koff, klen = pack_keys(queries, 5)
    p_keys, ok_keys = put(big, B0 + 16 * MiB, host)
    p_koff, ok_koff = put(big, B0 + 24 * MiB, koff)
    p_klen, ok_klen = put(big, B0 + 32 * MiB, klen)
    o = C0 + 16 * MiB
    p_hit, r_hit = take(big, o, 8 * q)
    p_off, r_off = take(big, o + MiB, 8 * q)
    p_status, r_status = take(big, o + 2 * MiB + 1, q)
    p_stage, r_stage = take(big, o + 3 * MiB + 3, q * T)
    p_err, r_err = take(big, o + 4 * MiB + 4, 4)
    torch.cuda.synchronize()
    assert L.nkv_locate_dev(ctx.h, structs, T, 5, p_keys + 5, p_koff, p_klen, q, 0, p_hit, p_off, p_status, p_stage,
                            p_err) == 0
    ctx.sync()
    for ok in (ok_keys, ok_koff, ok_klen, same[0], same[2]):
        ok()
    got = (r_hit().view(np.uint64).tolist(), r_off().view(np.int64).tolist(), r_status().tolist(),
           r_stage().reshape(q, T).tolist())
    assert int(r_err().view(np.uint32)[0]) == 0
    assert got == want_of(w, queries, 5)
    rc, hit, off, status, stage, err = dev_locate(nkv, upload(nkv, w), queries, base=5, key_at=5)  # the near twin
    assert (rc, err) == (0, 0) and got == (hit, off, status, stage)
