"""GPU: the SSTable Index and Summary tables on the device
(nkv_index_summary_dev, its host form nkv_index_summary_from_records, the
sstable / lsmtree functions over them) against tests/sstable_ref's literal
restatement of makeIndexAndSummary, bit for bit.  Every device call writes
into tests/guarded buffers: the images lie at the given byte offsets, the
guards around them stay intact and the inputs are unchanged."""
import ctypes
import os
import struct

import numpy as np
import pytest

from nakevaleng_amd import record
from tests import sstable_ref as ref
from tests.guarded import frozen, guarded
from tests.test_sstable_ref import HAND_INDEX, HAND_KEYS, HAND_PAGE, HAND_SIZES, HAND_SUMMARY

pytestmark = pytest.mark.gpu

INVALID = 2  # NKV_ERR_INVALID
FILL = 0xA5
KEY_LENGTHS = (0, 1, 7, 8, 9, 15, 16, 17, 40, 300)


def _torch():
    import torch
    return torch


def _dev(a):
    t = _torch().from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()
    _torch().cuda.synchronize()
    return t


def _offsets(sizes):
    off = np.zeros(len(sizes), np.uint64)
    if len(sizes) > 1:
        off[1:] = np.cumsum(np.asarray(sizes, np.uint64)[:-1])
    return off


def table_of(keys, values):
    """(stream, RecSize array) of records key_i / value_i as record.Serialize writes them."""
    return record.data_table(record.New(k, v, 7) for k, v in zip(keys, values))


def hand_table():
    return table_of(HAND_KEYS, [bytes(s - 30 - len(k)) for k, s in zip(HAND_KEYS, HAND_SIZES)])


def ragged(rng, n, lengths=KEY_LENGTHS, vmax=200):
    keys = [bytes(rng.integers(0, 256, int(rng.choice(lengths)), dtype=np.uint8)) for _ in range(n)]
    vals = [bytes(rng.integers(0, 256, int(rng.integers(0, vmax + 1)), dtype=np.uint8)) for _ in range(n)]
    return keys, vals


def dev_call(nkv, stream, off, page, residue=0, index_at=0, summary_at=0, caps=None, room=None, query=True):
    """nkv_index_summary_dev over `stream` placed `residue` bytes past a
    256-byte boundary, the images into guarded buffers at byte offsets index_at
    / summary_at.  room = (index bytes, summary bytes) of the payloads (default:
    what a size query reports), caps = the capacities passed (default: room).
    Returns (rc, index payload, summary payload, index_len, summary_len)."""
    _lib, ctx = nkv
    L = _lib.lib()
    n = len(off)
    host = np.zeros(residue + len(stream) + 1, np.uint8)
    host[residue:residue + len(stream)] = np.frombuffer(stream, np.uint8)
    d_data = _dev(host)
    d_off = _dev(np.asarray(off, np.uint64) if n else np.zeros(1, np.uint64))
    same = [frozen(d_data), frozen(d_off)]
    ilen, slen = ctypes.c_uint64(7), ctypes.c_uint64(7)
    args = (ctx.h, d_data.data_ptr() + residue if n else None, len(stream), d_off.data_ptr() if n else None, n, page)
    if query:
        rc = L.nkv_index_summary_dev(*args, None, 0, None, 0, ctypes.byref(ilen), ctypes.byref(slen))
        if rc != 0:
            return rc, None, None, ilen.value, slen.value
    room = room or (ilen.value, slen.value)
    caps = caps or room
    p_index, check_index = guarded(room[0], index_at, fill=FILL)
    p_summary, check_summary = guarded(room[1], summary_at, fill=FILL)
    a, b = ctypes.c_uint64(7), ctypes.c_uint64(7)
    rc = L.nkv_index_summary_dev(*args, p_index, caps[0], p_summary, caps[1], ctypes.byref(a), ctypes.byref(b))
    ctx.sync()
    for intact in same:
        intact()
    if query and rc == 0:
        assert (a.value, b.value) == (ilen.value, slen.value)
    return rc, check_index().tobytes(), check_summary().tobytes(), a.value, b.value


def host_call(nkv, stream, sizes, page):
    from nakevaleng_amd import sstable
    return sstable.index_and_summary(stream, sizes, page, device=0)


def check_table(nkv, stream, sizes, page, host=True, **kw):
    want = ref.from_table(stream, sizes, page)
    rc, index, summary, ilen, slen = dev_call(nkv, stream, _offsets(sizes), page, **kw)
    assert rc == 0
    assert (ilen, slen) == (len(want[0]), len(want[1]))
    assert index == want[0]
    assert summary == want[1]
    if host:
        assert host_call(nkv, stream, sizes, page) == want
    return want


def test_hand_case(nkv):
    stream, sizes = hand_table()
    assert sizes.tolist() == HAND_SIZES
    want = check_table(nkv, stream, sizes, HAND_PAGE)
    assert want == (HAND_INDEX, HAND_SUMMARY)


@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 65, 257, 4097])
def test_sizes_and_pages(nkv, n):
    rng = np.random.default_rng(0x6E00 + n)
    keys, vals = ragged(rng, n)
    stream, sizes = table_of(keys, vals)
    for j, page in enumerate((1, 3, 64, 4096, n + 5)):
        check_table(nkv, stream, sizes, page, host=j % 2 == 0, index_at=(0, 1, 7, 13)[j % 4],
                    summary_at=(13, 7, 1, 0)[j % 4])


def test_every_key_length_and_a_key_longer_than_a_tile(nkv):
    _lib, _ = nkv
    rng = np.random.default_rng(0x6B6C)
    tile = _lib.INDEX_WRITE_TILE
    lengths = list(KEY_LENGTHS) + [2 * tile + 1234]
    for order in (lengths, lengths[::-1]):
        keys = [bytes(rng.integers(0, 256, ln, dtype=np.uint8)) for ln in order]
        vals = [bytes(rng.integers(0, 256, int(rng.integers(0, 201)), dtype=np.uint8)) for _ in keys]
        stream, sizes = table_of(keys, vals)
        for page, at in ((1, 0), (3, 5), (len(keys) - 1, 11)):
            check_table(nkv, stream, sizes, page, index_at=at, summary_at=at + 1, residue=at)
    # the long key as MinKey, MaxKey and the only key: the header holds it twice
    big =bytes(rng.integers(0, 256, tile + 77, dtype=np.uint8))
    stream, sizes = table_of([big], [b"v"])
    check_table(nkv, stream, sizes, 3, summary_at=3)


def test_uniform_records(nkv):
    """The reference's own shape in small: 16-byte keys, 100-byte values."""
    rng = np.random.default_rng(0x756E)
    n = 3000
    keys = [bytes(rng.integers(0, 256, 16, dtype=np.uint8)) for _ in range(n)]
    stream, sizes = table_of(keys, [bytes(100)] * n)
    for at in (0, 9):
        check_table(nkv, stream, sizes, 3, index_at=at, summary_at=at, host=at == 0)


def test_tiny_records_span_many_tiles(nkv):
    """65,537 records with keys of 0..2 bytes and no values: over a MiB of Index
    in 16 to 18-byte entries, a thousand per tile."""
    rng = np.random.default_rng(0x7469)
    n = 65537
    lens = rng.integers(0, 3, n)
    raw = rng.integers(0, 256, (n, 2), dtype=np.uint8)
    keys = [raw[i, :lens[i]].tobytes() for i in range(n)]
    stream, sizes = table_of(keys, [b""] * n)
    check_table(nkv, stream, sizes, 3, index_at=7, summary_at=1, host=False)
    check_table(nkv, stream, sizes, 1, host=False)  # every record selected: the Summary spans many tiles too


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_index_length_at_the_tile_size(nkv, delta):
    _lib, _ = nkv
    tile = _lib.INDEX_WRITE_TILE
    rng = np.random.default_rng(0x746C + delta)
    n = 100
    last = tile + delta - 16 * n - 99 * 100
    keys = [bytes(rng.integers(0, 256, 100, dtype=np.uint8)) for _ in range(99)]
    keys.append(bytes(rng.integers(0, 256, last, dtype=np.uint8)))
    stream, sizes = table_of(keys, [b"xy"] * n)
    for at in (0, 1, 15):
        want = check_table(nkv, stream, sizes, 3, index_at=at, summary_at=at, host=False)
        assert len(want[0]) == tile + delta


@pytest.mark.parametrize("residue", range(16))
def test_every_stream_residue(nkv, residue):
    """Keys of 40 and 17 bytes: whole 16-byte chunks of key bytes at every
    source alignment against an aligned output and a misaligned one."""
    rng = np.random.default_rng(0x7273 + residue)
    keys, vals = ragged(rng, 60, lengths=(40, 17, 33), vmax=50)
    stream, sizes = table_of(keys, vals)
    for at in (0, 7):
        check_table(nkv, stream, sizes, 3, residue=residue, index_at=at, summary_at=(at + 6) % 16, host=False)


@pytest.mark.parametrize("index_at", [0, 1, 7, 13])
@pytest.mark.parametrize("summary_at", [0, 1, 7, 13])
def test_outputs_at_their_minimum_alignment(nkv, index_at, summary_at):
    rng = np.random.default_rng(0x6F75)
    keys, vals = ragged(rng, 500)
    stream, sizes = table_of(keys, vals)
    check_table(nkv, stream, sizes, 3, index_at=index_at, summary_at=summary_at, host=False)


def test_unsorted_and_duplicate_keys_are_encoded_verbatim(nkv):
    keys = [b"zebra", b"apple", b"apple", b"", b"mango", b"", b"apple", b"aardvark" * 5]
    stream, sizes = table_of(keys, [bytes([i]) * i for i in range(len(keys))])
    for page in (1, 2, 3):
        want = check_table(nkv, stream, sizes, page)
        assert want == ref.closed_index_and_summary(keys, sizes.tolist(), page)


def _good(nkv):
    stream, sizes = hand_table()
    check_table(nkv, stream, sizes, HAND_PAGE, host=False)


def test_size_query_with_null_outputs(nkv):
    _lib, ctx = nkv
    L = _lib.lib()
    stream, sizes = hand_table()
    d_data, d_off = _dev(np.frombuffer(stream, np.uint8)), _dev(_offsets(sizes))
    a, b = ctypes.c_uint64(7), ctypes.c_uint64(7)
    assert L.nkv_index_summary_dev(ctx.h, d_data.data_ptr(), len(stream), d_off.data_ptr(), 4, 2, None, 0, None, 0,
                                   ctypes.byref(a), ctypes.byref(b)) == 0
    assert (a.value, b.value) == (71, 79)
    # an empty table: no Index, the 24 zero bytes of an empty header
    assert L.nkv_index_summary_dev(ctx.h, None, 0, None, 0, 3, None, 0, None, 0, ctypes.byref(a), ctypes.byref(b)) == 0
    assert (a.value, b.value) == (0, 24)
    # the host form's query
    buf = np.frombuffer(stream, np.uint8).copy()
    assert L.nkv_index_summary_from_records(ctx.h, buf.ctypes.data, buf.size, sizes.ctypes.data, 4, 2, None, 0, None,
                                            0, ctypes.byref(a), ctypes.byref(b)) == 0
    assert (a.value, b.value) == (71, 79)
    # null length pointers, a null context, too many records
    assert L.nkv_index_summary_dev(ctx.h, d_data.data_ptr(), len(stream), d_off.data_ptr(), 4, 2, None, 0, None, 0,
                                   None, ctypes.byref(b)) == INVALID
    assert L.nkv_index_summary_dev(ctx.h, d_data.data_ptr(), len(stream), d_off.data_ptr(), 4, 2, None, 0, None, 0,
                                   ctypes.byref(a), None) == INVALID
    assert L.nkv_index_summary_dev(None, d_data.data_ptr(), len(stream), d_off.data_ptr(), 4, 2, None, 0, None, 0,
                                   ctypes.byref(a), ctypes.byref(b)) == INVALID
    assert L.nkv_index_summary_dev(ctx.h, d_data.data_ptr(), len(stream), d_off.data_ptr(), 2**31, 2, None, 0, None,
                                   0, ctypes.byref(a), ctypes.byref(b)) == INVALID
    _good(nkv)


def test_a_capacity_one_byte_short_writes_nothing(nkv):
    stream, sizes = hand_table()
    off = _offsets(sizes)
    for caps in ((70, 79), (71, 78)):
        rc, index, summary, ilen, slen = dev_call(nkv, stream, off, HAND_PAGE, room=(71, 79), caps=caps, query=False,
                                                  index_at=1, summary_at=7)
        assert rc == INVALID
        assert (ilen, slen) == (71, 79)  # still reported: the caller can retry
        assert index == bytes([FILL]) * 71 and summary == bytes([FILL]) * 79
    rc, index, summary, _, _ = dev_call(nkv, stream, off, HAND_PAGE, room=(71, 79), caps=(71, 79), query=False)
    assert rc == 0 and (index, summary) == (HAND_INDEX, HAND_SUMMARY)
    # more room than needed: only the reported extents are written
    rc, index, summary, ilen, slen = dev_call(nkv, stream, off, HAND_PAGE, room=(100, 100), query=False, index_at=13)
    assert rc == 0 and (ilen, slen) == (71, 79)
    assert index == HAND_INDEX + bytes([FILL]) * 29 and summary == HAND_SUMMARY + bytes([FILL]) * 21
    # the host form reports the lengths too and leaves its outputs alone
    _lib, ctx = nkv
    buf = np.frombuffer(stream, np.uint8).copy()
    oi, os_ = np.full(71, FILL, np.uint8), np.full(79, FILL, np.uint8)
    a, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
    assert _lib.lib().nkv_index_summary_from_records(ctx.h, buf.ctypes.data, buf.size, sizes.ctypes.data, 4, 2,
                                                     oi.ctypes.data, 71, os_.ctypes.data, 78, ctypes.byref(a),
                                                     ctypes.byref(b)) == INVALID
    assert (a.value, b.value) == (71, 79) and (oi == FILL).all() and (os_ == FILL).all()
    _good(nkv)


BAD_TABLES = {
    # record 1's KeySize reaches past the end of the stream
    "key_past_stream": lambda s, off: (s[:off[1] + 14] + struct.pack("<Q", len(s) - off[1] - 30 + 1) + s[off[1] + 22:], off),
    "key_size_wraps": lambda s, off: (s[:off[2] + 14] + struct.pack("<Q", 2**64 - 8) + s[off[2] + 22:], off),
    "rec_off_past_stream": lambda s, off: (s, off[:3] + [len(s) - 29]),
    "rec_off_wild": lambda s, off: (s, off[:2] + [2**64 - 8] + off[3:]),
}


@pytest.mark.parametrize("name", sorted(BAD_TABLES))
def test_bounds_the_measure_kernel_refuses(nkv, name):
    """A header or key span outside the stream is refused by the measure kernel
    before any writer is launched: NKV_ERR_INVALID, lengths 0, both payloads
    still the fill byte, and the context builds the hand case right after."""
    stream, sizes = hand_table()
    s, off = BAD_TABLES[name](stream, _offsets(sizes).tolist())
    rc, index, summary, ilen, slen = dev_call(nkv, s, off, HAND_PAGE, room=(200, 200), query=False, index_at=7)
    assert rc == INVALID and (ilen, slen) == (0, 0)
    assert index == bytes([FILL]) * 200 and summary == bytes([FILL]) * 200
    rc, _, _, ilen, slen = dev_call(nkv, s, off, HAND_PAGE)  # the size query refuses as well
    assert rc == INVALID and (ilen, slen) == (0, 0)
    _good(nkv)


def test_a_key_that_ends_exactly_at_the_stream_end_is_accepted(nkv):
    stream, sizes = table_of([b"a", b"bb", b"the-last-key"], [b"v", b"", b""])
    check_table(nkv, stream, sizes, 2)


def test_page_zero(nkv):
    one = table_of([b"only"], [b"value"])
    want = check_table(nkv, *one, 0)
    assert want == ref.from_table(*one, 3)
    two = table_of([b"a", b"b"], [b"", b""])
    rc, index, summary, ilen, slen = dev_call(nkv, two[0], _offsets(two[1]), 0, room=(64, 64), query=False)
    assert rc == INVALID and (ilen, slen) == (0, 0)
    assert index == bytes([FILL]) * 64 and summary == bytes([FILL]) * 64
    with pytest.raises(nkv[0].NkvError):
        host_call(nkv, *two, 0)
    rc, _, summary, ilen, slen = dev_call(nkv, b"", [], 0)
    assert rc == 0 and (ilen, slen) == (0, 24) and summary == bytes(24)
    _good(nkv)


def test_host_form_refuses_sizes_that_do_not_add_up(nkv):
    _lib, ctx = nkv
    stream, sizes = hand_table()
    buf = np.frombuffer(stream, np.uint8).copy()
    oi, os_ = np.zeros(128, np.uint8), np.zeros(128, np.uint8)
    a, b = ctypes.c_uint64(0), ctypes.c_uint64(0)

    def call(nbytes):
        return _lib.lib().nkv_index_summary_from_records(ctx.h, buf.ctypes.data, nbytes, sizes.ctypes.data, 4, 2,
                                                         oi.ctypes.data, 128, os_.ctypes.data, 128, ctypes.byref(a),
                                                         ctypes.byref(b))

    assert call(buf.size - 1) == INVALID
    assert call(buf.size) == 0
    assert (oi[:a.value].tobytes(), os_[:b.value].tobytes()) == (HAND_INDEX, HAND_SUMMARY)


def test_timing_intervals(nkv):
    """Under NKV_TIMING_EVENTS the call records its two intervals."""
    _lib, ctx = nkv
    stream, sizes = hand_table()
    ctx.set_timing(True)
    try:
        check_table(nkv, stream, sizes, HAND_PAGE, host=False, query=False, room=(71, 79))
        leaf, reduce_ = ctx.last_timing()
        assert leaf > 0 and reduce_ > 0
    finally:
        ctx.set_timing(False)


@pytest.mark.parametrize("chunk", range(10))
def test_fuzz(nkv, chunk):
    """200 seeded cases in all: n <= 300, any page, keys of the listed lengths or
    of any length up to 64, values of 0..200 bytes, every placement."""
    for seed in range(20 * chunk, 20 * chunk + 20):
        rng = np.random.default_rng(0x667A + seed)
        n = int(rng.integers(0, 301))
        page = int(rng.choice((1, 2, 3, 4, 7, 64, 299, 300, 1000)))
        lengths = KEY_LENGTHS if seed % 2 else tuple(range(65))
        keys, vals = ragged(rng, n, lengths=lengths)
        stream, sizes = table_of(keys, vals)
        check_table(nkv, stream, sizes, page, host=seed % 5 == 0, residue=seed % 16,
                    index_at=int(rng.integers(0, 16)), summary_at=int(rng.integers(0, 16)))


def test_compact_carries_index_and_summary(nkv):
    from nakevaleng_amd import lsmtree
    from tests.test_gpu_merge import fuzz_runs
    rng = np.random.default_rng(0x6369)
    runs = fuzz_runs(rng, 3, nmax=150, vmax=400)
    tabs = [record.data_table(run) for run in runs]
    plain = lsmtree.compact(tabs, device=0, seed=99)
    assert "index" not in plain and "summary" not in plain
    assert sorted(plain) == ["filter", "image", "root", "sources", "table"]
    got = lsmtree.compact(tabs, device=0, seed=99, summary_page_size=3)
    stream, sizes = got["table"]
    assert (stream, sizes.tolist()) == (plain["table"][0], plain["table"][1].tolist())
    assert (got["root"], got["image"]) == (plain["root"], plain["image"])
    assert (got["index"], got["summary"]) == ref.from_table(stream, sizes, 3)
    # the files resolve every merged key to its record
    off = _offsets(sizes).tolist()
    for kc, o in zip(ref.keyctx_of(stream, sizes), off):
        assert ref.lookup(got["index"], got["summary"], kc.Key) == o


def test_files_are_truncated(nkv, tmp_path):
    from nakevaleng_amd import sstable
    path = str(tmp_path) + "/"
    stream, sizes = hand_table()
    f_index, f_summary = path + "db-1-0-index.db", path + "db-1-0-summary.db"
    for f in (f_index, f_summary):
        with open(f, "wb") as fh:
            fh.write(b"S" * 500)
    assert sstable.make_index_and_summary_from_records(path, "db", HAND_PAGE, 1, 0, stream, sizes, device=0) is None
    assert open(f_index, "rb").read() == HAND_INDEX
    assert open(f_summary, "rb").read() == HAND_SUMMARY
    assert sorted(os.listdir(path)) == ["db-1-0-index.db", "db-1-0-summary.db"]


def test_table_secondaries_from_records(nkv, tmp_path):
    from nakevaleng_amd import sstable
    from nakevaleng_amd.merkletree import MerkleTreeError
    _lib, ctx = nkv
    rng = np.random.default_rng(0x7365)
    keys, vals = ragged(rng, 300)
    stream, sizes = table_of(sorted(set(keys)), vals[:len(set(keys))])
    a, b = str(tmp_path / "a") + "/", str(tmp_path / "b") + "/"
    os.mkdir(a)
    os.mkdir(b)
    for kind in ("index", "summary"):
        with open(f"{a}db-2-1-{kind}.db", "wb") as fh:
            fh.write(b"S" * (1 << 20))
    root, bf = sstable.make_table_secondaries_from_records(a, "db", 3, 2, 1, stream, sizes, device=0, seed=77)
    assert sorted(os.listdir(a)) == ["db-2-1-index.db", "db-2-1-metadata.db", "db-2-1-summary.db"]
    want = ref.from_table(stream, sizes, 3)
    assert open(a + "db-2-1-index.db", "rb").read() == want[0]
    assert open(a + "db-2-1-summary.db", "rb").read() == want[1]
    assert root == sstable.make_metadata_from_records(b, "db", 2, 1, stream, sizes, device=0)
    assert open(a + "db-2-1-metadata.db", "rb").read() == open(b + "db-2-1-metadata.db", "rb").read()
    want_bf = sstable.make_filter_from_records(stream, sizes, seed=77, ctx=ctx)
    assert (bf.M, bf.K, bf.HashSeeds, bf.Contents) == (want_bf.M, want_bf.K, want_bf.HashSeeds, want_bf.Contents)
    root2, none = sstable.make_table_secondaries_from_records(a, "db", 3, 2, 1, stream, sizes, device=0)
    assert root2 == root and none is None
    # no records: the reference writes the two files, then New panics
    c = str(tmp_path / "c") + "/"
    os.mkdir(c)
    with pytest.raises(MerkleTreeError):
        sstable.make_table_secondaries_from_records(c, "db", 3, 1, 0, b"", np.zeros(0, np.uint64), device=0)
    assert open(c + "db-1-0-index.db", "rb").read() == b""
    assert open(c + "db-1-0-summary.db", "rb").read() == bytes(24)
