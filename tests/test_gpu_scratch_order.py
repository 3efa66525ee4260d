"""GPU: the host-pointer entries' results do not depend on the order they are
called in on one context.

The entries share a context's scratch buffers, and five of those buffers carry
state from one call to the next (csrc/context.hpp, "state buffers").  The rest
of the suite runs every entry on one session-wide context, but always in the
same order.  Here every host-pointer entry of the binding runs on a fresh
context (create, one call, destroy) for its baseline, and then all of them run
on one context in three orders: forward, reverse and one fixed shuffle.  Every
output must equal its baseline byte for byte.

That is all this module checks: call-order independence.  Whether the outputs
are right is the business of the per-entry tests against the oracle.

Inputs: two Data tables of 4,100 records (more than the 64-value sort
threshold, the 4,096 of the gated plan and the staged bloom insert, and
small_max_n = 1,024, so the grid path runs), keys of 1 to 24 bytes.  The wide
table has values of 0, 1 to 300 and a handful of 5 KiB bytes (the gate opens:
sort and queue run); the narrow one has every value at 146 bytes (the gate
stays closed).
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 4100
_u32p = ctypes.POINTER(ctypes.c_uint32)


class _Table:
    """One Data table and the views of it the entries take."""

    def __init__(self, name, keys, values, rng):
        from nakevaleng_amd import record
        self.name = name
        self.n = n = len(keys)
        recs = [record.New(k, v, timestamp=7) for k, v in zip(keys, values)]
        stream, self.sizes = record.data_table(recs)
        self.stream = np.frombuffer(stream, np.uint8).copy()
        self.roff = np.zeros(n, np.uint64)
        self.roff[1:] = np.cumsum(self.sizes[:-1])
        self.klen = np.fromiter((len(k) for k in keys), np.uint64, n)
        self.vlen = np.fromiter((len(v) for v in values), np.uint64, n)
        self.koff = self.roff + np.uint64(30)       # spans into the stream
        self.voff = self.koff + self.klen
        self.puts = record.pack_puts(keys, values, timestamps=7)
        # a write log: the same records in a fixed arrival order
        arrival = rng.permutation(n)
        self.log = np.frombuffer(b"".join(recs[i].ToBytes() for i in arrival), np.uint8).copy()
        self.log_sizes = self.sizes[arrival].copy()
        # two sorted runs: the even and the odd records
        self.runs = []
        for h in (0, 1):
            part = recs[h::2]
            s, z = record.data_table(part)
            self.runs.append((np.frombuffer(s, np.uint8).copy(), z))
        self.leaf20 = rng.integers(0, 256, 20 * n, dtype=np.uint8)
        self.cms_table = rng.integers(0, 1000, 272 * 5, dtype=np.uint32)
        self.generic_root = None  # from the fresh-context baseline of tree_generic (validate's argument)


def _make_tables():
    rng = np.random.default_rng(4100)
    keys = set()
    while len(keys) < N:
        keys.add(rng.integers(0, 256, int(rng.integers(1, 25)), dtype=np.uint8).tobytes())
    keys = sorted(keys)
    vl = rng.integers(1, 301, N)
    vl[rng.choice(N, 200, replace=False)] = 0
    vl[rng.choice(N, 6, replace=False)] = 5120
    wide = [rng.integers(0, 256, int(v), dtype=np.uint8).tobytes() for v in vl]
    narrow = [rng.integers(0, 256, 146, dtype=np.uint8).tobytes() for _ in range(N)]
    return [_Table("wide", keys, wide, rng), _Table("narrow", keys, narrow, rng)]


def _cat(*arrays):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in arrays)


# ---- the entries: (lib module, ctypes library, context, table) -> every output byte ----

def _leaf_hash(_lib, L, ctx, t):
    out = np.zeros(20 * t.n, np.uint8)
    _lib.check(L.nkv_leaf_hash(ctx.h, _lib.p8(t.stream), _lib.p64(t.voff), _lib.p64(t.vlen), t.n, _lib.p8(out)))
    return _cat(out)


def _tree_outputs(L, n):
    return (np.zeros(20, np.uint8), np.zeros(20 * L.nkv_total_nodes(n), np.uint8),
            np.zeros(L.nkv_bfs_size(n), np.uint8))


def _tree_from_values(_lib, L, ctx, t):
    root, nodes, img = _tree_outputs(L, t.n)
    _lib.check(L.nkv_tree_from_values(ctx.h, _lib.p8(t.stream), _lib.p64(t.voff), _lib.p64(t.vlen), t.n,
                                      _lib.p8(root), _lib.p8(nodes), _lib.p8(img)))
    return _cat(root, nodes, img)


def _tree_build(_lib, L, ctx, t):
    root, nodes, img = _tree_outputs(L, t.n)
    _lib.check(L.nkv_tree_build(ctx.h, _lib.p8(t.leaf20), t.n, _lib.p8(root), _lib.p8(nodes), _lib.p8(img)))
    return _cat(root, nodes, img)


def _tree_generic(_lib, L, ctx, t):
    n1 = (t.n + 1) // 2
    root = np.zeros(20, np.uint8)
    upper = np.zeros(20 * L.nkv_total_nodes(n1), np.uint8)
    img = np.zeros(L.nkv_generic_bfs_size(_lib.p64(t.vlen), t.n), np.uint8)
    _lib.check(L.nkv_tree_generic(ctx.h, _lib.p8(t.stream), _lib.p64(t.voff), _lib.p64(t.vlen), t.n, _lib.p8(root),
                                  _lib.p8(upper), _lib.p8(img)))
    return _cat(root, upper, img)


def _tree_validate(_lib, L, ctx, t):
    ok = ctypes.c_int(-1)
    _lib.check(L.nkv_tree_validate(ctx.h, _lib.p8(t.stream), _lib.p64(t.voff), _lib.p64(t.vlen), t.n,
                                   _lib.p8(t.generic_root), ctypes.byref(ok)))
    return bytes([ok.value & 0xFF])


def _tree_from_records(_lib, L, ctx, t):
    root, nodes, img = _tree_outputs(L, t.n)
    _lib.check(L.nkv_tree_from_records(ctx.h, _lib.p8(t.stream), t.stream.size, _lib.p64(t.sizes), t.n,
                                       _lib.p8(root), _lib.p8(nodes), _lib.p8(img)))
    return _cat(root, nodes, img)


def _record_crc(_lib, L, ctx, t):
    crc = np.zeros(t.n, np.uint32)
    bad = np.zeros(2, np.uint64)
    _lib.check(L.nkv_record_crc(ctx.h, _lib.p8(t.stream), t.stream.size, _lib.p64(t.sizes), t.n,
                                crc.ctypes.data_as(_u32p), _lib.p64(bad[:1]), _lib.p64(bad[1:])))
    return _cat(crc, bad)


def _bloom_shape(L):
    m, k = ctypes.c_uint32(0), ctypes.c_uint32(0)
    assert L.nkv_bloom_params(N, 0.01, ctypes.byref(m), ctypes.byref(k)) == 0
    return m.value, k.value


def _bloom_build(_lib, L, ctx, t):
    m, k = _bloom_shape(L)
    bits = np.zeros((m + 7) // 8, np.uint8)
    _lib.check(L.nkv_bloom_build(ctx.h, _lib.p8(t.stream), _lib.p64(t.koff), _lib.p64(t.klen), t.n, m, k, 5,
                                 _lib.p8(bits)))
    return _cat(bits)


def _bloom_from_records(_lib, L, ctx, t):
    m, k = _bloom_shape(L)
    bits = np.zeros((m + 7) // 8, np.uint8)
    _lib.check(L.nkv_bloom_from_records(ctx.h, _lib.p8(t.stream), t.stream.size, _lib.p64(t.sizes), t.n, m, k, 5,
                                        _lib.p8(bits)))
    return _cat(bits)


def _hll_add(_lib, L, ctx, t):
    reg = np.zeros(1 << 12, np.uint8)
    _lib.check(L.nkv_hll_add(ctx.h, t.stream.ctypes.data, t.koff.ctypes.data, t.klen.ctypes.data, t.n, 12,
                             reg.ctypes.data))
    return _cat(reg)


def _hll_add_records(_lib, L, ctx, t):
    reg = np.zeros(1 << 12, np.uint8)
    _lib.check(L.nkv_hll_add_records(ctx.h, t.stream.ctypes.data, t.stream.size, t.sizes.ctypes.data, t.n, 12,
                                     reg.ctypes.data))
    return _cat(reg)


def _cms_insert(_lib, L, ctx, t):
    table = t.cms_table.copy()
    _lib.check(L.nkv_cms_insert(ctx.h, t.stream.ctypes.data, t.koff.ctypes.data, t.klen.ctypes.data, t.n, 272, 5, 9,
                                table.ctypes.data))
    return _cat(table)


def _cms_insert_records(_lib, L, ctx, t):
    table = t.cms_table.copy()
    _lib.check(L.nkv_cms_insert_records(ctx.h, t.stream.ctypes.data, t.stream.size, t.sizes.ctypes.data, t.n, 272,
                                        5, 9, table.ctypes.data))
    return _cat(table)


def _cms_query(_lib, L, ctx, t):
    out = np.zeros(t.n, np.uint32)
    _lib.check(L.nkv_cms_query(ctx.h, t.stream.ctypes.data, t.koff.ctypes.data, t.klen.ctypes.data, t.n, 272, 5, 9,
                               t.cms_table.ctypes.data, out.ctypes.data))
    return _cat(out)


def _index_summary(_lib, L, ctx, t):
    index, summary = np.zeros(t.stream.size, np.uint8), np.zeros(t.stream.size, np.uint8)
    ilen, slen = ctypes.c_uint64(0), ctypes.c_uint64(0)
    _lib.check(L.nkv_index_summary_from_records(ctx.h, t.stream.ctypes.data, t.stream.size, t.sizes.ctypes.data, t.n,
                                                16, index.ctypes.data, index.size, summary.ctypes.data, summary.size,
                                                ctypes.byref(ilen), ctypes.byref(slen)))
    return _cat(np.array([ilen.value, slen.value], np.uint64), index[:ilen.value], summary[:slen.value])


def _sort_records(_lib, L, ctx, t):
    out, sizes = np.zeros(t.log.size, np.uint8), np.zeros(t.n, np.uint64)
    n_out, out_len = ctypes.c_uint64(0), ctypes.c_uint64(0)
    _lib.check(L.nkv_sort_records(ctx.h, t.log.ctypes.data, t.log.size, t.log_sizes.ctypes.data, t.n,
                                  out.ctypes.data, out.size, sizes.ctypes.data, ctypes.byref(n_out),
                                  ctypes.byref(out_len)))
    return _cat(np.array([n_out.value, out_len.value], np.uint64), out[:out_len.value], sizes[:n_out.value])


def _merge_records(_lib, L, ctx, t):
    (sa, za), (sb, zb) = t.runs
    streams = (ctypes.c_void_p * 2)(sa.ctypes.data, sb.ctypes.data)
    rec_size = (ctypes.c_void_p * 2)(za.ctypes.data, zb.ctypes.data)
    lens = np.array([sa.size, sb.size], np.uint64)
    ns = np.array([za.size, zb.size], np.uint64)
    out, sizes = np.zeros(sa.size + sb.size, np.uint8), np.zeros(t.n, np.uint64)
    n_out, out_len = ctypes.c_uint64(0), ctypes.c_uint64(0)
    _lib.check(L.nkv_merge_records(ctx.h, streams, _lib.p64(lens), rec_size, _lib.p64(ns), 2, out.ctypes.data,
                                   out.size, sizes.ctypes.data, ctypes.byref(n_out), ctypes.byref(out_len)))
    return _cat(np.array([n_out.value, out_len.value], np.uint64), out[:out_len.value], sizes[:n_out.value])


def _encode_records(_lib, L, ctx, t):
    p = t.puts
    puts = _lib.NkvPuts(p["keys"].ctypes.data, p["keys"].size, p["koff"].ctypes.data, p["klen"].ctypes.data,
                        p["vals"].ctypes.data, p["vals"].size, p["voff"].ctypes.data, p["vlen"].ctypes.data,
                        None, p["ts_all"], None, None, t.n)
    out, sizes, crc = np.zeros(t.stream.size, np.uint8), np.zeros(t.n, np.uint64), np.zeros(t.n, np.uint32)
    out_len = ctypes.c_uint64(0)
    _lib.check(L.nkv_encode_records(ctx.h, ctypes.byref(puts), out.ctypes.data, out.size, sizes.ctypes.data,
                                    crc.ctypes.data, ctypes.byref(out_len)))
    return _cat(np.array([out_len.value], np.uint64), out[:out_len.value], sizes, crc)


def _frame_records(_lib, L, ctx, t):
    seg_off = np.zeros(1, np.uint64)
    sizes, first, seg_len = np.zeros(t.n, np.uint64), np.zeros(2, np.uint64), np.zeros(1, np.uint64)
    stats = np.zeros(4, np.uint64)
    n_out = ctypes.c_uint64(0)
    _lib.check(L.nkv_frame_records(ctx.h, t.stream.ctypes.data, t.stream.size, seg_off.ctypes.data, 1,
                                   _lib.NKV_FRAME_STRICT, sizes.ctypes.data, sizes.size, first.ctypes.data,
                                   seg_len.ctypes.data, ctypes.byref(n_out), _lib.p64(stats)))
    return _cat(np.array([n_out.value], np.uint64), sizes[:n_out.value], first, seg_len, stats)


ENTRIES = [_leaf_hash, _tree_from_values, _tree_build, _tree_generic, _tree_validate, _tree_from_records,
           _record_crc, _bloom_build, _bloom_from_records, _hll_add, _hll_add_records, _cms_insert,
           _cms_insert_records, _cms_query, _index_summary, _sort_records, _merge_records, _encode_records,
           _frame_records]


@pytest.fixture(scope="module")
def baseline(nkv):
    """(tables, calls, {call: output on a fresh context}); calls = every entry on
    either table, in the forward order."""
    _lib, _ = nkv
    L = _lib.lib()
    tables = _make_tables()
    calls = [(t, e) for t in tables for e in ENTRIES]
    want = {}
    for t, e in calls:
        if e is _tree_validate:  # a root that validates: the generic tree's, from its own fresh context
            t.generic_root = np.frombuffer(want[(t.name, "_tree_generic")][:20], np.uint8).copy()
        with _lib.Context(0) as fresh:
            want[(t.name, e.__name__)] = e(_lib, L, fresh, t)
    for t in tables:
        assert want[(t.name, "_tree_validate")] == b"\x01"
    return tables, calls, want


def _ordered(calls, order):
    if order == "forward":
        return list(calls)
    if order == "reverse":
        return list(calls)[::-1]
    idx = np.random.default_rng(19).permutation(len(calls))
    return [calls[i] for i in idx]


@pytest.mark.parametrize("order", ["forward", "reverse", "shuffle"])
def test_outputs_do_not_depend_on_call_order(nkv, baseline, order):
    _lib, _ = nkv
    L = _lib.lib()
    _, calls, want = baseline
    differ = []
    with _lib.Context(0) as ctx:
        for t, e in _ordered(calls, order):
            if e(_lib, L, ctx, t) != want[(t.name, e.__name__)]:
                differ.append(f"{e.__name__}({t.name})")
    assert not differ, f"{order}: outputs that differ from a fresh context's: {differ}"
