"""GPU: the device paths over data more than 4 GiB apart.

The leaf kernels address a wave's 64 values as 32-bit offsets from a
wave-uniform base and fall back to 64-bit addresses when the values lie too
far apart (csrc/sha1_feed_dev.hpp: ring_vc_blocks, sha1_blocks_pair,
sha1_blocks_shift; csrc/leaf.hip: k_leaf's fallthroughs).  Here one allocation of 9 GiB is
never filled as a whole: each case uploads a few MiB into islands at 0, about
2^32 and about 2 * 2^32 (tests/far.py) and asserts that
  1. the device result equals the oracle's over the compact host array,
  2. so does the same call over the compact layout in an ordinary small tensor
     (the near twin: a far failure then points at the far branch, not the shape),
  3. the uploaded islands read back unchanged.

Allocation rule (tests/far.py, checked by tests/test_far_layout.py): all values
of a case live in the one allocation, which reaches at least 2^32 + the longest
value past the lowest address of any wave, so an address built from a wrapped
32-bit offset still lies inside it: a wrong branch reads wrong bytes, never
unmapped memory.

Batches of at most 64 values run in input order through k_leaf whatever
NKV_OPT_BUCKET says; the work-queue kernel (ring_vc_blocks) takes sorted
batches of more than 64.  The cases that are about ring_vc_blocks therefore
carry 64 or more one-compression fillers behind the wave they are about: the
sort is by compression count, so that wave is the queue's first group.
"""
import ctypes
import struct

import numpy as np
import pytest

from tests import far

pytestmark = pytest.mark.gpu

SEED = 0x66617230
FILL = 0xA5
PIECE = 256 << 20


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
def fctx(nkv):
    """A context of this module's own on torch's current stream, every option at its default."""
    _lib, _ = nkv
    ctx = _lib.Context(0)
    ctx.set_stream(_torch().cuda.current_stream().cuda_stream)
    yield _lib, ctx
    ctx.close()


DEFAULTS = {"NKV_OPT_LEAF_LOAD": 4, "NKV_OPT_BUCKET": 2, "NKV_OPT_SIDE_GATE": 1, "NKV_OPT_RECORDS_FUSED": 1,
            "NKV_OPT_CRC_LOAD": 0, "NKV_OPT_BLOOM_PATH": 2}


class _options:
    """Set options for a block and put the defaults back (context.hpp) afterwards."""

    def __init__(self, _lib, ctx, **opts):
        self._lib, self.ctx, self.opts = _lib, ctx, opts

    def __enter__(self):
        for k, v in self.opts.items():
            self.ctx.set_option(getattr(self._lib, k), v)

    def __exit__(self, *exc):
        for k in self.opts:
            self.ctx.set_option(getattr(self._lib, k), DEFAULTS[k])


def _upload(big, compact, uploads):
    torch = _torch()
    for base, sl in uploads:
        big[base:base + sl.stop - sl.start].copy_(torch.from_numpy(compact[sl].copy()))


def _unchanged(big, compact, uploads):
    for base, sl in uploads:
        assert np.array_equal(big[base:base + sl.stop - sl.start].cpu().numpy(), compact[sl])


def _nodes(torch, L, n):
    return torch.zeros(L.nkv_total_nodes(n) * 20, dtype=torch.uint8, device="cuda")


def _np20(t):
    return t.cpu().numpy().reshape(-1, 20)


# ---------------------------------------------------------------------------
# values

_value_ref = {}


def _value_reference(oracle, case):
    """(compact bytes, oracle tree), computed once per case and left unchanged."""
    if case.name not in _value_ref:
        data = oracle.splitmix64_bytes(case.compact_bytes, SEED + len(_value_ref))
        want = oracle.tree_from_digests(oracle.leaf_hashes(data, case.off, case.lens, threads=8))
        data.setflags(write=False)
        want.setflags(write=False)
        _value_ref[case.name] = (data, want)
    return _value_ref[case.name]


def _values_calls(torch, _lib, ctx, base_ptr, d_off, d_len, n):
    """(level 0 of nkv_leaf_hash_dev, all levels of nkv_tree_from_values_dev)."""
    L = _lib.lib()
    d_leaf = torch.zeros(n * 20, dtype=torch.uint8, device="cuda")
    d_tree = _nodes(torch, L, n)
    _lib.check(L.nkv_leaf_hash_dev(ctx.h, base_ptr, d_off.data_ptr(), d_len.data_ptr(), n, d_leaf.data_ptr()))
    _lib.check(L.nkv_tree_from_values_dev(ctx.h, base_ptr, d_off.data_ptr(), d_len.data_ptr(), n, d_tree.data_ptr()))
    torch.cuda.synchronize()
    return _np20(d_leaf), _np20(d_tree)


@pytest.mark.parametrize("bucket", [0, 1, 2])
@pytest.mark.parametrize("load", [4, 11])
@pytest.mark.parametrize("case", far.value_cases(), ids=lambda c: c.name)
def test_values(fctx, oracle, big, case, load, bucket):
    torch = _torch()
    _lib, ctx = fctx
    data, want = _value_reference(oracle, case)
    n = case.n
    dev_off, uploads = case.placed()
    _upload(big, data, uploads)
    d_len = _dev(case.lens)
    d_far_off, d_near_off, d_near = _dev(dev_off), _dev(case.off), _dev(data)
    # both sides of the auto order's second stream where the auto gate applies
    gates = (1, 0) if n >= 4096 and bucket == 2 else (1,)
    for side_gate in gates:
        with _options(_lib, ctx, NKV_OPT_LEAF_LOAD=load, NKV_OPT_BUCKET=bucket, NKV_OPT_SIDE_GATE=side_gate):
            far_leaf, far_tree = _values_calls(torch, _lib, ctx, big.data_ptr(), d_far_off, d_len, n)
            near_leaf, near_tree = _values_calls(torch, _lib, ctx, d_near.data_ptr(), d_near_off, d_len, n)
        assert np.array_equal(near_leaf, want[:n]) and np.array_equal(near_tree, want), "near twin"
        bad = np.nonzero((far_leaf != want[:n]).any(axis=1))[0]
        assert bad.size == 0, f"nkv_leaf_hash_dev: {bad.size} of {n} far digests differ, first at {bad[:8].tolist()}"
        assert np.array_equal(far_tree, want), "nkv_tree_from_values_dev over the far layout"
    _unchanged(big, data, uploads)


# ---------------------------------------------------------------------------
# strided

def _strided_calls(torch, _lib, ctx, ptr, stride, length, n):
    L = _lib.lib()
    d_leaf = torch.zeros(n * 20, dtype=torch.uint8, device="cuda")
    d_tree = _nodes(torch, L, n)
    _lib.check(L.nkv_leaf_hash_strided_dev(ctx.h, ptr, stride, length, n, d_leaf.data_ptr()))
    _lib.check(L.nkv_tree_from_strided_dev(ctx.h, ptr, stride, length, n, d_tree.data_ptr()))
    torch.cuda.synchronize()
    return _np20(d_leaf), _np20(d_tree)


def _strided_setup(torch, oracle, big, case, seed):
    """Write the values with one strided copy; returns (compact (n, L) host array,
    oracle tree, far view, near tensor, near pointer, near stride)."""
    n, length = case.n, case.L
    compact = oracle.splitmix64_bytes(n * length, seed).reshape(n, length)
    want = oracle.tree_from_digests(oracle.leaf_hashes(compact.reshape(-1), np.arange(n, dtype=np.uint64) * length,
                                                       np.full(n, length, np.uint64)))
    view = torch.as_strided(big, (n, length), (case.stride, 1), case.base)
    view.copy_(torch.from_numpy(compact))
    ns = case.near_stride()
    near = torch.zeros(case.base % 64 + n * ns + 64, dtype=torch.uint8, device="cuda")
    assert near.data_ptr() % 64 == 0
    torch.as_strided(near, (n, length), (ns, 1), case.base % 64).copy_(torch.from_numpy(compact))
    return compact, want, view, near, near.data_ptr() + case.base % 64, ns


@pytest.mark.parametrize("case,load", [(c, ld) for c in far.strided_cases() for ld in c.loads],
                         ids=lambda v: v.name if isinstance(v, far.Strided) else f"load{v}")
def test_strided(fctx, oracle, big, case, load):
    torch = _torch()
    _lib, ctx = fctx
    n = case.n
    compact, want, view, near, near_ptr, ns = _strided_setup(torch, oracle, big, case, SEED + case.L)
    with _options(_lib, ctx, NKV_OPT_LEAF_LOAD=load):
        far_leaf, far_tree = _strided_calls(torch, _lib, ctx, big.data_ptr() + case.base, case.stride, case.L, n)
        near_leaf, near_tree = _strided_calls(torch, _lib, ctx, near_ptr, ns, case.L, n)
    assert np.array_equal(near_leaf, want[:n]) and np.array_equal(near_tree, want), "near twin"
    bad = np.nonzero((far_leaf != want[:n]).any(axis=1))[0]
    assert bad.size == 0, f"nkv_leaf_hash_strided_dev: {bad.size} of {n} far digests differ, first at {bad[:8].tolist()}"
    assert np.array_equal(far_tree, want), "nkv_tree_from_strided_dev over the far layout"
    assert np.array_equal(view.cpu().numpy(), compact)


@pytest.mark.parametrize("load", [4, 11])
def test_trees_strided_far_next_to_values_near(fctx, oracle, big, load):
    """nkv_trees_dev: a STRIDED table whose waves span 4 GiB beside a near VALUES table."""
    torch = _torch()
    _lib, ctx = fctx
    L = _lib.lib()
    case = next(c for c in far.strided_cases() if c.name == "b0-s0+1-len200")
    compact, want, view, _, _, _ = _strided_setup(torch, oracle, big, case, SEED + 77)
    vcase = next(c for c in far.value_cases() if c.name == "ragged-n64")
    vdata, vwant = _value_reference(oracle, vcase)
    d_v, d_off, d_len = _dev(vdata), _dev(vcase.off), _dev(vcase.lens)
    nodes_s, nodes_v = _nodes(torch, L, case.n), _nodes(torch, L, vcase.n)
    with _options(_lib, ctx, NKV_OPT_LEAF_LOAD=load):
        ctx.trees([_lib.table(_lib.NKV_TABLE_STRIDED, nodes_s.data_ptr(), case.n, base=big.data_ptr() + case.base,
                              stride=case.stride, length=case.L),
                   _lib.table(_lib.NKV_TABLE_VALUES, nodes_v.data_ptr(), vcase.n, base=d_v.data_ptr(),
                              off=d_off.data_ptr(), lens=d_len.data_ptr())])
        torch.cuda.synchronize()
    assert np.array_equal(_np20(nodes_v), vwant)
    assert np.array_equal(_np20(nodes_s), want)
    assert np.array_equal(view.cpu().numpy(), compact)


# ---------------------------------------------------------------------------
# records dealt to the three islands

# (NKV_OPT_RECORDS_FUSED, NKV_OPT_BUCKET, NKV_OPT_CRC_LOAD, NKV_OPT_BLOOM_PATH): every value of
# every option, every (fused, bucket) pair, each CRC load and filter path under both fused settings
RECORD_COMBOS = [(1, 2, 0, 2), (1, 0, 8, 0), (1, 1, 0, 1), (0, 2, 8, 1), (0, 0, 0, 2), (0, 1, 8, 0)]
_record_ref = {}


def _record_reference(oracle, case):
    """The compact table (sealed records) and everything the oracle says about it."""
    if case.name not in _record_ref:
        lay = case.layout
        n = case.n
        data = oracle.splitmix64_bytes(lay.compact_bytes, SEED + 100 + len(_record_ref))
        for i in range(n):
            struct.pack_into("<IqBBQQ", data, int(lay.off[i]), 0, 1 + i % 3, 0, 0, int(case.ks[i]), int(case.vs[i]))
        oracle.seal_records(data, lay.off, threads=8)
        koff = lay.off + np.uint64(30)
        voff = koff + case.ks
        ref = {"data": data, "koff": koff, "voff": voff,
               "tree": oracle.tree_from_digests(oracle.leaf_hashes(data, voff, case.vs, threads=8))}
        ref["crc"], ok, bad = oracle.record_crcs(data, lay.off)
        assert bad == 0 and ok.all()
        ref["m"], ref["k"] = oracle.bloom_params(n, 0.01)
        ref["bits"] = oracle.bloom_insert(data, koff, case.ks, ref["m"], ref["k"], 0xFA4)
        ref["hit_values"] = oracle.bloom_query(data, voff, np.minimum(case.vs, 24), ref["m"], ref["k"], 0xFA4,
                                               ref["bits"])
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _record_ref[case.name] = ref
    return _record_ref[case.name]


def _record_calls(torch, _lib, ctx, ref, case, stream_ptr, stream_len, rec_off, shift):
    """Every record call over the table at stream_ptr; `shift` = device offset
    minus compact offset of each record (what the plain-span calls add)."""
    L = _lib.lib()
    n, m, k = case.n, ref["m"], ref["k"]
    u8 = lambda size: torch.zeros(size, dtype=torch.uint8, device="cuda")
    d_rec = _dev(rec_off)
    out = {}
    d_tree, d_err = _nodes(torch, L, n), u8(4)
    _lib.check(L.nkv_tree_from_records_dev(ctx.h, stream_ptr, stream_len, d_rec.data_ptr(), n, d_tree.data_ptr(),
                                           d_err.data_ptr()))
    d_vtree, d_vcrc, d_vstats = _nodes(torch, L, n), u8(4 * n), u8(24)
    _lib.check(L.nkv_tree_verify_records_dev(ctx.h, stream_ptr, stream_len, d_rec.data_ptr(), n, d_vtree.data_ptr(),
                                             d_vcrc.data_ptr(), d_vstats.data_ptr()))
    d_crc, d_stats = u8(4 * n), u8(24)
    _lib.check(L.nkv_record_crc_dev(ctx.h, stream_ptr, stream_len, d_rec.data_ptr(), n, d_crc.data_ptr(),
                                    d_stats.data_ptr()))
    d_voff, d_vlen = u8(8 * n), u8(8 * n)
    _lib.check(L.nkv_locate_values_dev(ctx.h, stream_ptr, stream_len, d_rec.data_ptr(), n, d_voff.data_ptr(),
                                       d_vlen.data_ptr()))
    words = ((m + 31) // 32) * 4
    d_bits_rec, d_bits, d_hit_keys, d_hit_values = u8(words), u8(words), u8(n), u8(n)
    _lib.check(L.nkv_bloom_insert_records_dev(ctx.h, stream_ptr, stream_len, d_rec.data_ptr(), n, m, k, 0xFA4,
                                              d_bits_rec.data_ptr()))
    # plain spans: Key ++ Value for the checksum, the keys for the filter, value prefixes as strangers
    d_koff, d_kvlen, d_klen = _dev(ref["koff"] + shift), _dev(case.ks + case.vs), _dev(case.ks)
    d_qoff, d_qlen = _dev(ref["voff"] + shift), _dev(np.minimum(case.vs, 24))
    d_span_crc = u8(4 * n)
    _lib.check(L.nkv_crc32_dev(ctx.h, stream_ptr, d_koff.data_ptr(), d_kvlen.data_ptr(), n, d_span_crc.data_ptr()))
    _lib.check(L.nkv_bloom_insert_dev(ctx.h, stream_ptr, d_koff.data_ptr(), d_klen.data_ptr(), n, m, k, 0xFA4,
                                      d_bits.data_ptr()))
    _lib.check(L.nkv_bloom_query_dev(ctx.h, stream_ptr, d_koff.data_ptr(), d_klen.data_ptr(), n, m, k, 0xFA4,
                                     d_bits.data_ptr(), d_hit_keys.data_ptr()))
    _lib.check(L.nkv_bloom_query_dev(ctx.h, stream_ptr, d_qoff.data_ptr(), d_qlen.data_ptr(), n, m, k, 0xFA4,
                                     d_bits.data_ptr(), d_hit_values.data_ptr()))
    torch.cuda.synchronize()
    u64 = lambda t: t.cpu().numpy().view(np.uint64)
    return {"tree": _np20(d_tree), "err": int(d_err.cpu().numpy().view(np.uint32)[0]),
            "vtree": _np20(d_vtree), "vcrc": d_vcrc.cpu().numpy().view(np.uint32), "vstats": u64(d_vstats).tolist(),
            "crc": d_crc.cpu().numpy().view(np.uint32), "stats": u64(d_stats).tolist(),
            "voff": u64(d_voff), "vlen": u64(d_vlen), "bits_rec": d_bits_rec.cpu().numpy(),
            "bits": d_bits.cpu().numpy(), "span_crc": d_span_crc.cpu().numpy().view(np.uint32),
            "hit_keys": d_hit_keys.cpu().numpy(), "hit_values": d_hit_values.cpu().numpy().astype(bool)}


def _check_records(got, ref, case, rec_off, what, bad=None):
    """bad = the one record whose stored Crc was flipped, or None."""
    nbytes = (ref["m"] + 7) // 8
    clear = [0, 2**64 - 1, 0] if bad is None else [1, bad, 0]
    assert np.array_equal(got["tree"], ref["tree"]) and got["err"] == 0, what + ": nkv_tree_from_records_dev"
    assert np.array_equal(got["vtree"], ref["tree"]), what + ": nkv_tree_verify_records_dev tree"
    assert np.array_equal(got["vcrc"], ref["crc"]) and got["vstats"] == clear, what + ": nkv_tree_verify_records_dev"
    assert np.array_equal(got["crc"], ref["crc"]) and got["stats"] == clear, what + ": nkv_record_crc_dev"
    assert np.array_equal(got["voff"], rec_off + np.uint64(30) + case.ks), what + ": nkv_locate_values_dev offsets"
    assert np.array_equal(got["vlen"], case.vs), what + ": nkv_locate_values_dev lengths"
    assert np.array_equal(got["span_crc"], ref["crc"]), what + ": nkv_crc32_dev"
    for name in ("bits_rec", "bits"):
        assert np.array_equal(got[name][:nbytes], ref["bits"]) and not got[name][nbytes:].any(), f"{what}: {name}"
    assert (got["hit_keys"] == 1).all(), what + ": nkv_bloom_query_dev over the inserted keys"
    assert np.array_equal(got["hit_values"], ref["hit_values"]), what + ": nkv_bloom_query_dev over strangers"


@pytest.mark.parametrize("combo", RECORD_COMBOS, ids=lambda c: "fused%d-bucket%d-crc%d-bloom%d" % c)
@pytest.mark.parametrize("case", far.record_cases(), ids=lambda c: c.name)
def test_records(fctx, oracle, big, case, combo):
    torch = _torch()
    _lib, ctx = fctx
    ref = _record_reference(oracle, case)
    data, lay = ref["data"], case.layout
    dev_off, uploads = lay.placed()
    assert (dev_off[np.arange(case.n) % 3 != 0] >= far.G32).all()
    _upload(big, data, uploads)
    d_near = _dev(data)
    shift = dev_off - lay.off
    zero = np.zeros(case.n, np.uint64)
    fused, bucket, crc_load, bloom_path = combo
    opts = dict(NKV_OPT_RECORDS_FUSED=fused, NKV_OPT_BUCKET=bucket, NKV_OPT_CRC_LOAD=crc_load,
                NKV_OPT_BLOOM_PATH=bloom_path)
    with _options(_lib, ctx, **opts):
        got_far = _record_calls(torch, _lib, ctx, ref, case, big.data_ptr(), far.ALLOC, dev_off, shift)
        got_near = _record_calls(torch, _lib, ctx, ref, case, d_near.data_ptr(), data.size, lay.off, zero)
    _check_records(got_near, ref, case, lay.off, "near twin")
    _check_records(got_far, ref, case, dev_off, "far")
    _unchanged(big, data, uploads)
    # one stored Crc flipped in the far island
    j = case.n - 1 - (case.n - 1 - 2) % 3
    assert j % 3 == 2 and dev_off[j] >= 2 * far.G32
    big[int(dev_off[j])] ^= 0x01
    d_near[int(lay.off[j])] ^= 0x01
    with _options(_lib, ctx, **opts):
        got_far = _record_calls(torch, _lib, ctx, ref, case, big.data_ptr(), far.ALLOC, dev_off, shift)
        got_near = _record_calls(torch, _lib, ctx, ref, case, d_near.data_ptr(), data.size, lay.off, zero)
    big[int(dev_off[j])] ^= 0x01
    _check_records(got_near, ref, case, lay.off, "near twin, one Crc flipped", bad=j)
    _check_records(got_far, ref, case, dev_off, "far, one Crc flipped", bad=j)
    _unchanged(big, data, uploads)


# ---------------------------------------------------------------------------
# a Data table longer than 4 GiB

def _key(i):
    return b"far-key-%08d" % i  # 16 bytes


def _device_equal(big, a, b, size):
    """big[a : a + size] == big[b : b + size], in pieces of at most 256 MiB."""
    torch = _torch()
    for at in range(0, size, PIECE):
        m = min(PIECE, size - at)
        if not torch.equal(big[a + at:a + at + m], big[b + at:b + at + m]):
            return False
    return True


def _device_all(big, a, size, byte):
    for at in range(0, size, PIECE):
        m = min(PIECE, size - at)
        if not bool((big[a + at:a + at + m] == byte).all()):
            return False
    return True


@pytest.mark.parametrize("giant_wins", [True, False], ids=["giant-newer", "giant-older"])
def test_data_table_longer_than_4_gib(fctx, oracle, big, giant_wins):
    """nkv_merge_records_dev over a contiguous run with one record whose value
    is 2^32 + 5 bytes; then its output through the calls that take it as it is.
    The giant value is copied and compared, never hashed or checksummed."""
    from nakevaleng_amd import record
    from tests import sstable_ref
    from tests.merge_ref import merge_closed
    torch = _torch()
    _lib, ctx = fctx
    L = _lib.lib()
    # run 0: two small records, the giant one, two small ones; every Value is the fill's bytes
    small = 100
    ids0, vs0 = [10, 20, 30, 40, 50], [small, small + 1, far.GIANT_VALUE, small + 2, small + 3]
    ts0 = [5, 5, 9 if giant_wins else 1, 5, 5]
    size0 = [30 + 16 + v for v in vs0]
    off0 = np.concatenate([[0], np.cumsum(size0)[:-1]]).astype(np.uint64)
    len0 = int(sum(size0))
    assert off0[3] > far.G32 and len0 <= far.GIANT_VALUE + far.GIANT_SMALL
    # run 1: interleaving keys; 30 is the giant's key, 50 a trailing key of run 0 with a newer Timestamp
    ids1 = [5, 15, 30, 35, 50, 60]
    rng = np.random.default_rng(0x67696E74)
    run1 = [record.New(_key(i), rng.integers(0, 256, 60 + i, dtype=np.uint8).tobytes(), 7) for i in ids1]
    data1, size1 = record.data_table(run1)
    data1 = np.frombuffer(data1, np.uint8)
    off1 = np.concatenate([[0], np.cumsum(size1)[:-1]]).astype(np.uint64)
    assert data1.size <= far.GIANT_SMALL

    r0, r1, out_at = far.GIANT_RUN0_AT, far.GIANT_RUN1_AT, far.GIANT_OUT_AT
    _lib.check(L.nkv_fill_splitmix64_dev(ctx.h, big.data_ptr() + r0, len0, SEED))
    heads = [np.frombuffer(struct.pack("<IqBBQQ", 0, ts0[i], 0, 0, 16, vs0[i]) + _key(ids0[i]), np.uint8)
             for i in range(5)]
    for i in range(5):
        big[r0 + int(off0[i]):r0 + int(off0[i]) + 46].copy_(torch.from_numpy(heads[i].copy()))
    big[r1:r1 + data1.size].copy_(torch.from_numpy(data1.copy()))
    big[out_at:out_at + far.GIANT_OUT_CAP + 4096].fill_(FILL)
    d_off0, d_off1 = _dev(off0), _dev(off1)
    runs = (_lib.NkvRun * 2)(_lib.NkvRun(big.data_ptr() + r0, len0, d_off0.data_ptr(), 5),
                             _lib.NkvRun(big.data_ptr() + r1, data1.size, d_off1.data_ptr(), len(ids1)))
    d_out_off = torch.zeros(8 * 11, dtype=torch.uint8, device="cuda")
    d_out_src = torch.zeros(8 * 11, dtype=torch.uint8, device="cuda")
    n_out, out_len = ctypes.c_uint64(7), ctypes.c_uint64(7)
    torch.cuda.synchronize()
    _lib.check(L.nkv_merge_records_dev(ctx.h, runs, 2, big.data_ptr() + out_at, far.GIANT_OUT_CAP,
                                       d_out_off.data_ptr(), d_out_src.data_ptr(), ctypes.byref(n_out),
                                       ctypes.byref(out_len)))
    torch.cuda.synchronize()

    # expected order and sources from stand-ins with the same keys and Timestamps
    stand0 = [record.Record(0, ts0[i], 0, 0, 16, 0, _key(ids0[i]), b"") for i in range(5)]
    _, src = merge_closed([stand0, run1])
    assert ((0, 2) in src) == giant_wins and (1, 4) in src and (0, 4) not in src
    sizes = [int(size0[i]) if r == 0 else int(size1[i]) for r, i in src]
    want_off = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)
    n = len(src)
    assert n_out.value == n and out_len.value == sum(sizes)
    assert (out_len.value > far.G32) == giant_wins
    assert np.array_equal(d_out_off.cpu().numpy().view(np.uint64)[:n], want_off)
    assert np.array_equal(d_out_src.cpu().numpy().view(np.uint64)[:n],
                          np.asarray([(r << 32) | i for r, i in src], np.uint64))
    assert any(r == 0 and off0[i] > far.G32 for r, i in src), "a source past 2^32 of its run"
    for (r, i), o, s in zip(src, want_off.tolist(), sizes):
        at = r0 + int(off0[i]) if r == 0 else r1 + int(off1[i])
        assert _device_equal(big, at, out_at + o, s), f"output record from run {r} index {i}"
    # nothing past out_len was written
    assert _device_all(big, out_at + out_len.value, far.GIANT_OUT_CAP + 4096 - out_len.value, FILL)
    # the inputs: run 1 and run 0's headers and keys
    assert np.array_equal(big[r1:r1 + data1.size].cpu().numpy(), data1)
    for i in range(5):
        assert np.array_equal(big[r0 + int(off0[i]):r0 + int(off0[i]) + 46].cpu().numpy(), heads[i])
    if not giant_wins:
        return

    # the merged table, longer than 4 GiB, as it is
    keys = [_key(ids0[i]) if r == 0 else run1[i].Key for r, i in src]
    assert keys == sorted(keys)
    stream_ptr = big.data_ptr() + out_at
    want_index, want_summary = sstable_ref.make_index_and_summary(
        [sstable_ref.KeyContext(k, s) for k, s in zip(keys, sizes)], 2)
    assert max(struct.unpack_from("<q", want_index, 32 * e + 8)[0] for e in range(n)) > far.G32
    ilen, slen = ctypes.c_uint64(7), ctypes.c_uint64(7)
    d_index = torch.full((len(want_index) + 8,), FILL, dtype=torch.uint8, device="cuda")
    d_summary = torch.full((len(want_summary) + 8,), FILL, dtype=torch.uint8, device="cuda")
    _lib.check(L.nkv_index_summary_dev(ctx.h, stream_ptr, out_len.value, d_out_off.data_ptr(), n, 2,
                                       d_index.data_ptr(), len(want_index), d_summary.data_ptr(), len(want_summary),
                                       ctypes.byref(ilen), ctypes.byref(slen)))
    ctx.sync()
    assert (ilen.value, slen.value) == (len(want_index), len(want_summary))
    assert d_index.cpu().numpy().tobytes() == want_index + bytes([FILL] * 8)
    assert d_summary.cpu().numpy().tobytes() == want_summary + bytes([FILL] * 8)

    d_voff = torch.zeros(8 * n, dtype=torch.uint8, device="cuda")
    d_vlen = torch.zeros(8 * n, dtype=torch.uint8, device="cuda")
    _lib.check(L.nkv_locate_values_dev(ctx.h, stream_ptr, out_len.value, d_out_off.data_ptr(), n, d_voff.data_ptr(),
                                       d_vlen.data_ptr()))
    torch.cuda.synchronize()
    assert np.array_equal(d_voff.cpu().numpy().view(np.uint64), want_off + np.uint64(46))
    assert d_vlen.cpu().numpy().view(np.uint64).tolist() == [s - 46 for s in sizes]
    assert max(s - 46 for s in sizes) == far.GIANT_VALUE

    m, k = oracle.bloom_params(n, 0.01)
    kdata = np.frombuffer(b"".join(keys), np.uint8)
    want_bits = oracle.bloom_insert(kdata, np.arange(n, dtype=np.uint64) * 16, np.full(n, 16, np.uint64), m, k, 0xFA4)
    d_bits = torch.zeros(((m + 31) // 32) * 4, dtype=torch.uint8, device="cuda")
    _lib.check(L.nkv_bloom_insert_records_dev(ctx.h, stream_ptr, out_len.value, d_out_off.data_ptr(), n, m, k, 0xFA4,
                                              d_bits.data_ptr()))
    torch.cuda.synchronize()
    bits = d_bits.cpu().numpy()
    assert np.array_equal(bits[:want_bits.size], want_bits) and not bits[want_bits.size:].any()
