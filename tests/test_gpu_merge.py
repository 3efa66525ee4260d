"""GPU: compaction's k-way merge on the device (nkv_merge_records_dev, its host
form nkv_merge_records / lsmtree.merge, and lsmtree.compact) against
tests/merge_ref.merge_closed, bit for bit: the merged stream, d_out_off,
d_out_src, n_out and out_len."""
import ctypes

import numpy as np
import pytest

from nakevaleng_amd import record
from tests.merge_ref import merge_closed
from tests.test_merge_ref import BOUNDARY_SEEDS, HAND_CASES, boundary_case, boundary_coverage, rec

pytestmark = pytest.mark.gpu

INVALID = 2  # NKV_ERR_INVALID


def _torch():
    import torch
    return torch


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


def _offsets(sizes):
    off = np.zeros(len(sizes), np.uint64)
    if len(sizes) > 1:
        off[1:] = np.cumsum(np.asarray(sizes, np.uint64)[:-1])
    return off


def expected(runs):
    """merge_closed's output as (stream bytes, offsets, (run << 32) | index)."""
    out, src = merge_closed(runs)
    parts = [r.ToBytes() for r in out]
    return (b"".join(parts), _offsets([len(p) for p in parts]),
            np.asarray([(r << 32) | i for r, i in src], dtype=np.uint64))


def merge_raw(nkv, tabs, shift_in=0, shift_out=0, want_src=True, out_cap=None):
    """nkv_merge_records_dev over tabs = [(stream bytes, offsets array)]: run r's
    stream lies shift_in + r bytes (mod 16) past an aligned address when
    shift_in is set, d_out shift_out bytes past one.  Returns (rc, stream,
    offsets, sources, n_out, out_len)."""
    torch = _torch()
    _lib, ctx = nkv
    k = len(tabs)
    runs = (_lib.NkvRun * max(k, 1))()
    keep = []
    total = n_all = 0
    for r, (data, off) in enumerate(tabs):
        sh = (shift_in + r) % 16 if shift_in else 0
        buf = np.zeros(sh + len(data), np.uint8)
        buf[sh:] = np.frombuffer(data, np.uint8)
        d_data, d_off = _dev(buf if buf.size else np.zeros(1, np.uint8)), _dev(off if len(off) else np.zeros(1, np.uint64))
        keep += [d_data, d_off]
        runs[r] = _lib.NkvRun(d_data.data_ptr() + sh if len(off) else None, len(data),
                              d_off.data_ptr() if len(off) else None, len(off))
        total += len(data)
        n_all += len(off)
    cap = total if out_cap is None else out_cap
    d_out = torch.full((total + shift_out + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    d_out_off = torch.zeros(8 * max(n_all, 1), dtype=torch.uint8, device="cuda")
    d_out_src = torch.zeros(8 * max(n_all, 1), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    n_out, out_len = ctypes.c_uint64(7), ctypes.c_uint64(7)
    rc = _lib.lib().nkv_merge_records_dev(ctx.h, runs, k, d_out.data_ptr() + shift_out, cap, d_out_off.data_ptr(),
                                          d_out_src.data_ptr() if want_src else None, ctypes.byref(n_out),
                                          ctypes.byref(out_len))
    torch.cuda.synchronize()
    if rc != 0:
        return rc, None, None, None, n_out.value, out_len.value
    n, nb = n_out.value, out_len.value
    full = d_out.cpu().numpy()
    # nothing outside [shift_out, shift_out + out_len) was written
    assert (full[:shift_out] == 0xA5).all() and (full[shift_out + nb:] == 0xA5).all()
    return (rc, full[shift_out:shift_out + nb].tobytes(), d_out_off.cpu().numpy().view(np.uint64)[:n],
            d_out_src.cpu().numpy().view(np.uint64)[:n], n, nb)


def tables_of(runs):
    out = []
    for run in runs:
        data, sizes = record.data_table(run)
        out.append((data, _offsets(sizes)))
    return out


def check_merge(nkv, runs, **kw):
    want_stream, want_off, want_src = expected(runs)
    rc, stream, off, src, n, nb = merge_raw(nkv, tables_of(runs), **kw)
    assert rc == 0
    assert n == len(want_off) and nb == len(want_stream)
    assert np.array_equal(off, want_off)
    if kw.get("want_src", True):
        assert np.array_equal(src, want_src)
    assert stream == want_stream
    return want_src


@pytest.mark.parametrize("name", sorted(HAND_CASES))
def test_hand_cases(nkv, name):
    runs, want = HAND_CASES[name]
    src = check_merge(nkv, runs)
    assert [(int(s) >> 32, int(s) & 0xFFFFFFFF) for s in src] == want


def fuzz_runs(rng, k, nmax=300, vmax=3000):
    """Keys of 0..40 bytes that share long prefixes (a fixed 36-byte stem cut
    anywhere, then up to 4 letters of a 3-letter alphabet), drawn per run from
    one pool so that exact duplicates across runs are common; values of 0..vmax
    bytes; three adjacent timestamps around zero; some tombstones."""
    stem = bytes(rng.integers(97, 99, 36, dtype=np.uint8))
    pool = sorted({stem[:int(rng.integers(0, 37))] + bytes(rng.integers(97, 100, int(rng.integers(0, 5)), dtype=np.uint8))
                   for _ in range(500)})
    runs = []
    for _ in range(k):
        n = int(rng.integers(0, min(nmax, len(pool)) + 1))
        pick = sorted(rng.choice(len(pool), n, replace=False).tolist())
        run = []
        for j in pick:
            val = rng.integers(0, 256, int(rng.integers(0, vmax + 1)), dtype=np.uint8).tobytes()
            run.append(rec(pool[j], int(rng.integers(-1, 2)), val, tomb=bool(rng.random() < 0.1)))
        runs.append(run)
    return runs


@pytest.mark.parametrize("seed", range(20))
def test_fuzz(nkv, seed):
    rng = np.random.default_rng(0x6D72 + seed)
    k = [1, 2, 3, 4, 6, 16][seed % 6]
    check_merge(nkv, fuzz_runs(rng, k), shift_in=seed % 3, shift_out=(5 * seed) % 16, want_src=seed % 4 != 3)


@pytest.mark.parametrize("seed", range(BOUNDARY_SEEDS))
def test_fuzz_keys_at_prefix_boundary(nkv, seed):
    """Keys over {0x00, 'a', 0xFF} that differ at or just past byte 8 (every
    prefix of an 8-byte stem, the stem plus tails of 0..3 bytes, a second stem
    that differs in byte 8): cmp_key's dense zero-padded prefix, its shortcut on
    the lengths when a key has at most 8 bytes, and the byte loop behind it.
    The CPU side (tests/test_merge_ref.py) asserts that merge_literal and
    merge_closed agree for k <= 6 and that the 12 seeds hold at least 100 key
    pairs with equal padded prefixes of either sort; here every seed's case
    holds some."""
    k, runs = boundary_case(seed)
    short, long_, _, _ = boundary_coverage(runs)
    assert short >= 1 and long_ >= 1
    check_merge(nkv, runs, shift_in=seed % 3, shift_out=(5 * seed) % 16, want_src=seed % 4 != 3)


def test_compact_of_empty_runs_raises_the_reference_error(nkv):
    """Every run empty: the merge itself returns no records, and the tree step
    that follows refuses with New's text (merkletree.go:20)."""
    from nakevaleng_amd import lsmtree
    from nakevaleng_amd.merkletree import MerkleTreeError
    for k in (1, 3):
        with pytest.raises(MerkleTreeError) as e:
            lsmtree.compact([(b"", np.zeros(0, np.uint64))] * k, device=0)
        assert str(e.value) == "cannot build Merkle Tree from 0 nodes"
    _good(nkv)


def test_sstable_shape_many_tiles(nkv):
    """4 runs of 16 Ki records (16-byte keys, 4,050-byte values; about a quarter
    of the keys in two runs): many scan tiles and copy tiles."""
    rng = np.random.default_rng(0x4B31)
    n, ks, vs, k = 16384, 16, 4050, 4
    pool = np.unique(rng.integers(0, 1 << 40, int(k * n * 0.8)).astype(np.uint64))
    runs = []
    for r in range(k):
        ids = np.sort(rng.choice(pool, n, replace=False))
        body = rng.integers(0, 256, (n, 30 + ks + vs), dtype=np.uint8)
        ts = rng.integers(0, 3, n)
        body[:, 4:12] = ts.astype("<i8").view(np.uint8).reshape(n, 8)
        body[:, 14:22] = np.frombuffer(np.uint64(ks).tobytes(), np.uint8)
        body[:, 22:30] = np.frombuffer(np.uint64(vs).tobytes(), np.uint8)
        body[:, 30:38] = 0
        body[:, 38:46] = ids.astype(">u8").view(np.uint8).reshape(n, 8)
        raw = body.tobytes()
        runs.append([_record_at(raw, i * (30 + ks + vs)) for i in range(n)])
    check_merge(nkv, runs)


def _record_at(buf, off):
    crc, ts, st, ti, ks, vs = record._HDR.unpack_from(buf, off)
    k0 = off + record.HEADER_SIZE
    return record.Record(crc, ts, st, ti, ks, vs, buf[k0:k0 + ks], buf[k0 + ks:k0 + ks + vs])


def test_tiny_records_many_per_tile(nkv):
    """Header-only records (keys of 0..2 bytes, the empty key once per run, no
    values): hundreds of records in every 16 KiB of output."""
    rng = np.random.default_rng(0x7469)
    runs = []
    for r in range(4):
        keys = {b""} | {bytes(rng.integers(0, 256, int(rng.integers(1, 3)), dtype=np.uint8)) for _ in range(3000)}
        runs.append([rec(key, int(rng.integers(0, 3)), b"") for key in sorted(keys)])
    check_merge(nkv, runs, shift_out=9)


def test_one_record_spans_many_tiles(nkv):
    rng = np.random.default_rng(0x6C6F)
    big = rng.integers(0, 256, 300 * 1024, dtype=np.uint8).tobytes()
    runs = [[rec(b"a", 1, b"x" * 7), rec(b"m", 1, big), rec(b"z", 1, b"y" * 11)],
            [rec(b"b", 1, b"q"), rec(b"m", 0, b"old"), rec(b"n", 2, b"r" * 33)]]
    check_merge(nkv, runs, shift_in=1, shift_out=3)


@pytest.mark.parametrize("residue", range(16))
def test_every_source_residue(nkv, residue):
    """The second output record is copied from source offset 31 + residue of run
    0 (behind a leading record that loses to run 1's), so its bytes take the
    funnel shift of every source residue mod 16 against an aligned output and a
    misaligned one."""
    rng = np.random.default_rng(residue)
    body = rng.integers(0, 256, 5000, dtype=np.uint8).tobytes()
    runs = [[rec(b"a", 0, b"L" * residue), rec(b"b", 0, body)], [rec(b"a", 5, b"")]]
    for shift_out in (0, 7):
        src = check_merge(nkv, runs, shift_out=shift_out)
        assert src.tolist() == [(1 << 32) | 0, 1]


def test_host_form_and_lsmtree_merge(nkv):
    _lib, ctx = nkv
    from nakevaleng_amd import lsmtree
    rng = np.random.default_rng(0x686F)
    runs = fuzz_runs(rng, 4)
    want_stream, want_off, _ = expected(runs)
    tabs = [record.data_table(run) for run in runs]
    stream, sizes = lsmtree.merge(tabs, device=0)
    assert stream == want_stream
    assert np.array_equal(_offsets(sizes), want_off) and int(sizes.sum()) == len(want_stream)
    rc, d_stream, d_off, _, n, nb = merge_raw(nkv, tables_of(runs))
    assert rc == 0 and d_stream == stream and np.array_equal(d_off, want_off)
    # the C entry itself: a size list that does not add up to its stream is refused
    k = len(tabs)
    bufs = [np.frombuffer(t[0] + b"\0", np.uint8) for t in tabs]
    szs = [np.ascontiguousarray(t[1] if len(t[1]) else np.zeros(1, np.uint64), dtype=np.uint64) for t in tabs]
    lens = np.asarray([len(t[0]) for t in tabs], np.uint64)
    ns = np.asarray([len(t[1]) for t in tabs], np.uint64)
    out = np.zeros(int(lens.sum()) + 1, np.uint8)
    osz = np.zeros(int(ns.sum()) + 1, np.uint64)
    a, b = ctypes.c_uint64(), ctypes.c_uint64()

    def call(lens_):
        return _lib.lib().nkv_merge_records(
            ctx.h, (ctypes.c_void_p * k)(*[x.ctypes.data for x in bufs]), _lib.p64(lens_),
            (ctypes.c_void_p * k)(*[x.ctypes.data for x in szs]), _lib.p64(ns), k, out.ctypes.data,
            out.size - 1, osz.ctypes.data, ctypes.byref(a), ctypes.byref(b))

    assert call(lens) == 0
    assert out[:b.value].tobytes() == want_stream and np.array_equal(osz[:a.value], sizes)
    short = lens.copy()
    short[[i for i in range(k) if ns[i]][0]] -= 1
    assert call(short) == INVALID
    assert call(lens) == 0


def test_compact_pipeline(nkv, oracle):
    from nakevaleng_amd import lsmtree, sstable
    _lib, ctx = nkv
    rng = np.random.default_rng(0x7069)
    runs = fuzz_runs(rng, 3)
    tabs = [record.data_table(run) for run in runs]
    got = lsmtree.compact(tabs, device=0, seed=4242)
    want_stream, want_off, want_src = expected(runs)
    stream, sizes = got["table"]
    assert stream == want_stream and np.array_equal(_offsets(sizes), want_off)
    assert np.array_equal(got["sources"], want_src)
    merged, _ = merge_closed(runs)
    n = len(merged)
    buf = np.frombuffer(want_stream + b"\0", np.uint8)
    voff, vlen = record.value_spans(want_stream, sizes)
    nodes = oracle.tree_from_digests(oracle.leaf_hashes(buf, voff, vlen))
    assert got["root"] == nodes[-1].tobytes()
    assert got["image"] == oracle.bfs_image(nodes, n)
    assert record.checksums(stream, sizes, ctx)[1] == 0
    want_bf = sstable.make_filter_from_records(want_stream, sizes, seed=4242, ctx=ctx)
    assert (got["filter"].M, got["filter"].K, got["filter"].HashSeeds) == (want_bf.M, want_bf.K, want_bf.HashSeeds)
    assert got["filter"].Contents == want_bf.Contents
    assert lsmtree.compact(tabs, device=0)["filter"] is None

    # one corrupted value byte in the longest run: the checksum error, and no merge launched
    r = max(range(3), key=lambda j: len(tabs[j][1]))
    run = runs[r]
    i = next(j for j, x in enumerate(run) if x.ValueSize > 0)
    at = int(tabs[r][1][:i].sum()) + 30 + run[i].KeySize
    data = bytearray(tabs[r][0])
    data[at] ^= 0x40
    bad = list(tabs)
    bad[r] = (bytes(data), tabs[r][1])
    calls = []
    L = _lib.lib()
    real = L.nkv_merge_records_dev

    class Spy:
        def __getattr__(self, name):
            if name == "nkv_merge_records_dev":
                return lambda *a: calls.append(a) or real(*a)
            return getattr(L, name)

    import zlib
    key, val = run[i].Key, bytearray(run[i].Value)
    val[0] ^= 0x40
    msg = f"Bad Record checksum (got {zlib.crc32(key + bytes(val))}, expected {run[i].Crc})"
    saved = _lib._lib
    _lib._lib = Spy()
    try:
        with pytest.raises(ValueError) as e:
            lsmtree.compact(bad, device=0)
    finally:
        _lib._lib = saved
    assert str(e.value) == msg
    assert calls == []


def _good(nkv):
    check_merge(nkv, HAND_CASES["newer_in_run0"][0])


def _tab(recs):
    return tables_of([recs])[0]


def _patch(tab, at, raw):
    data = bytearray(tab[0])
    data[at:at + len(raw)] = raw
    return bytes(data), tab[1]


BAD_RUNS = {
    "equal_adjacent": lambda: _tab([rec(b"a"), rec(b"b"), rec(b"b", 1), rec(b"c")]),
    "descending": lambda: _tab([rec(b"a"), rec(b"c"), rec(b"b")]),
    # long keys that differ after the dense 8-byte prefix only
    "descending_long": lambda: _tab([rec(b"0123456789b"), rec(b"0123456789a")]),
    # the same 8 bytes: the longer key first
    "descending_at_8": lambda: _tab([rec(b"abcdefgh\x00"), rec(b"abcdefgh")]),
    # equal zero-padded prefixes, decided by the lengths: the longer key first
    "equal_padded": lambda: _tab([rec(b"ab\x00"), rec(b"ab")]),
    "value_size_2_63": lambda: _patch(_tab([rec(b"a"), rec(b"b")]), 22, (1 << 63).to_bytes(8, "little")),
    "value_size_wraps": lambda: _patch(_tab([rec(b"a"), rec(b"b")]), 22, (2**64 - 20).to_bytes(8, "little")),
    "key_past_stream": lambda: _patch(_tab([rec(b"a"), rec(b"b")]), 32 + 14, (1000).to_bytes(8, "little")),
    "rec_off_mismatch": lambda: (_tab([rec(b"a"), rec(b"b"), rec(b"c")])[0], np.asarray([0, 31, 64], np.uint64)),
    "rec_off_wild": lambda: (_tab([rec(b"a"), rec(b"b")])[0], np.asarray([0, 2**64 - 8], np.uint64)),
    "first_not_at_zero": lambda: (_tab([rec(b"a"), rec(b"b")])[0], np.asarray([32], np.uint64)),
    "stream_longer_than_records": lambda: (_tab([rec(b"a")])[0] + b"\0" * 5, np.asarray([0], np.uint64)),
}


@pytest.mark.parametrize("name", sorted(BAD_RUNS))
def test_bad_runs_are_refused(nkv, name):
    """Each is refused by the validation kernel with NKV_ERR_INVALID, as run 1
    of two and alone; the context merges correctly right after."""
    bad = BAD_RUNS[name]()
    good = _tab([rec(b"a", 1), rec(b"k", 2, b"value")])
    for tabs in ([good, bad], [bad]):
        rc, *_ , n, nb = merge_raw(nkv, tabs)
        assert rc == INVALID and n == 0 and nb == 0
    _good(nkv)


def test_bad_arguments_are_refused(nkv):
    _lib, ctx = nkv
    torch = _torch()
    L = _lib.lib()
    good = _tab([rec(b"a", 1), rec(b"k", 2, b"value")])
    total = len(good[0])
    assert merge_raw(nkv, [])[0] == INVALID  # k = 0
    assert merge_raw(nkv, [good] * 17)[0] == INVALID
    assert merge_raw(nkv, [good] * 16)[0] == 0
    assert merge_raw(nkv, [good, good], out_cap=2 * total - 1)[0] == INVALID
    assert merge_raw(nkv, [good, good], out_cap=2 * total)[0] == 0
    d_data, d_off = _dev(np.frombuffer(good[0], np.uint8)), _dev(good[1])
    d_out = torch.zeros(total, dtype=torch.uint8, device="cuda")
    d_oo = torch.zeros(16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    a, b = ctypes.c_uint64(), ctypes.c_uint64()
    run = (_lib.NkvRun * 1)(_lib.NkvRun(d_data.data_ptr(), total, d_off.data_ptr(), 2))
    ok = dict(runs=run, out=d_out.data_ptr(), off=d_oo.data_ptr(), n=ctypes.byref(a), ln=ctypes.byref(b))

    def call(**kw):
        p = dict(ok, **kw)
        return L.nkv_merge_records_dev(ctx.h, p["runs"], 1, p["out"], total, p["off"], None, p["n"], p["ln"])

    assert call() == 0 and (a.value, b.value) == (2, total)
    for name in ("runs", "out", "off", "n", "ln"):
        assert call(**{name: None}) == INVALID, name
    assert call(runs=(_lib.NkvRun * 1)(_lib.NkvRun(None, total, d_off.data_ptr(), 2))) == INVALID
    assert call(runs=(_lib.NkvRun * 1)(_lib.NkvRun(d_data.data_ptr(), total, None, 2))) == INVALID
    assert L.nkv_merge_records_dev(None, run, 1, ok["out"], total, ok["off"], None, ok["n"], ok["ln"]) == INVALID
    assert call() == 0
    _good(nkv)


def test_offsets_from_the_library_feed_the_merge(nkv):
    """rec_off as nkv_record_offsets_dev writes it, and the merged table straight
    into nkv_record_crc_dev: every stored Crc still matches."""
    _lib, ctx = nkv
    torch = _torch()
    L = _lib.lib()
    rng = np.random.default_rng(0x6F66)
    runs = fuzz_runs(rng, 3, nmax=120)
    run_arr = (_lib.NkvRun * 3)()
    keep = []
    total = n_all = 0
    for r, run in enumerate(runs):
        data, sizes = record.data_table(run)
        d_data = _dev(np.frombuffer(data + b"\0", np.uint8))
        d_size = _dev(sizes if len(sizes) else np.zeros(1, np.uint64))
        d_off = torch.zeros(8 * max(len(sizes), 1), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        _lib.check(L.nkv_record_offsets_dev(ctx.h, d_size.data_ptr(), len(sizes), d_off.data_ptr()))
        keep += [d_data, d_size, d_off]
        run_arr[r] = _lib.NkvRun(d_data.data_ptr() if len(sizes) else None, len(data),
                                 d_off.data_ptr() if len(sizes) else None, len(sizes))
        total += len(data)
        n_all += len(sizes)
    d_out = torch.zeros(total + 16, dtype=torch.uint8, device="cuda")
    d_oo = torch.zeros(8 * n_all + 8, dtype=torch.uint8, device="cuda")
    d_stats = torch.zeros(24, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    a, b = ctypes.c_uint64(), ctypes.c_uint64()
    _lib.check(L.nkv_merge_records_dev(ctx.h, run_arr, 3, d_out.data_ptr(), total, d_oo.data_ptr(), None,
                                       ctypes.byref(a), ctypes.byref(b)))
    want_stream, want_off, _ = expected(runs)
    assert (a.value, b.value) == (len(want_off), len(want_stream))
    _lib.check(L.nkv_record_crc_dev(ctx.h, d_out.data_ptr(), b.value, d_oo.data_ptr(), a.value, None,
                                    d_stats.data_ptr()))
    ctx.sync()
    assert d_stats.cpu().numpy().view(np.uint64).tolist() == [0, 2**64 - 1, 0]
    assert d_out.cpu().numpy()[:b.value].tobytes() == want_stream
