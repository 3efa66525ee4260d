"""GPU: the Index/Summary readers on the device (nkv_index_open_dev,
nkv_locate_dev, sstable.open_index[_files], lsmtree.locate_many /
get_many_on_disk) against tests/index_open_ref: every entry offset, n, s and
verdict of the open -- on the one-lane path (NKV_OPT_INDEX_OPEN_PATH 1) and the
chunked one (2), whose bytes must be the same -- and every hit, Data offset,
status and stage byte of the locate.  Outputs lie in tests/guarded buffers at
the minimum alignment the header promises; the guards stay intact and every
input comes back unchanged."""
import ctypes
import struct
from dataclasses import dataclass, field
from typing import Callable, List

import numpy as np
import pytest

from nakevaleng_amd import record
from tests import index_open_ref as ref
from tests import lookup_ref, sstable_ref
from tests.guarded import frozen, guarded
from tests.test_gpu_lookup import key_pool, make_filter, make_queries, pack_keys

pytestmark = pytest.mark.gpu

INVALID = 2  # NKV_ERR_INVALID
FILL = 0xA5
K = 4096  # the chunked path's default bytes per lane
PATHS = (1, 2)


def _torch():
    import torch
    return torch


def _dev(a):
    a = np.ascontiguousarray(a).view(np.uint8)
    t = _torch().from_numpy((a if a.size else np.zeros(1, np.uint8)).copy()).cuda()
    _torch().cuda.synchronize()
    return t


def place(buf: bytes, at: int):
    """`buf` on the device `at` bytes past a 256-byte boundary: (tensor, address)."""
    host = np.zeros(at + len(buf) + 1, np.uint8)
    host[at:at + len(buf)] = np.frombuffer(buf, np.uint8)
    t = _dev(host)
    return t, t.data_ptr() + at


# ---------------------------------------------------------------------------
# open

def dev_open(nkv, index, summary, path, chunk=0, at=(0, 0), cap=None, query=False):
    """(rc, ent_off as written, n, s, verdict, the whole d_ent_off buffer)."""
    _lib, ctx = nkv
    d_i, p_i = place(index, at[0])
    d_s, p_s = place(summary, at[1])
    same = [frozen(d_i), frozen(d_s)]
    cap = len(index) // 16 if cap is None else cap
    p_ent, c_ent = guarded(8 * cap, 8, fill=FILL)
    n, s, v = ctypes.c_uint64(77), ctypes.c_uint64(77), ctypes.c_uint32(77)
    ctx.set_option(_lib.NKV_OPT_INDEX_OPEN_PATH, path)
    ctx.set_option(_lib.NKV_OPT_INDEX_OPEN_CHUNK, chunk)
    try:
        rc = _lib.lib().nkv_index_open_dev(ctx.h, p_i, len(index), p_s, len(summary), None if query else p_ent, cap,
                                           ctypes.byref(n), ctypes.byref(s), ctypes.byref(v))
        ctx.sync()
    finally:
        ctx.set_option(_lib.NKV_OPT_INDEX_OPEN_PATH, 0)
        ctx.set_option(_lib.NKV_OPT_INDEX_OPEN_CHUNK, 0)
    for intact in same:
        intact()
    whole = c_ent().view(np.uint64)
    return rc, whole[:n.value].tolist() if n.value <= cap else None, n.value, s.value, v.value, whole


def check_open(nkv, index, summary, chunks=(0,), at=(0, 0)):
    """Both paths (the chunked one at every chunk size given) against the
    reference; exactly n entries written when the verdict is 0, none otherwise."""
    want_ent, want_n, want_s, want_v = ref.open(index, summary)
    fill64 = int.from_bytes(bytes([FILL]) * 8, "little")
    seen = []
    for path, chunk in [(1, 0)] + [(2, c) for c in chunks] + [(0, 0)]:
        rc, ent, n, s, v, whole = dev_open(nkv, index, summary, path, chunk, at)
        assert rc == 0, (path, chunk)
        assert (v & -v, n, s) == (want_v, want_n, want_s), (path, chunk, v)
        assert ent == want_ent
        assert (whole[n:] == fill64).all()
        seen.append(whole.tobytes())
    assert all(b == seen[0] for b in seen)
    return want_n, want_s


@pytest.mark.parametrize("name", sorted(ref.hand_made()))
def test_open_hand_made_refusals(nkv, name):
    index, summary, bit = ref.hand_made()[name]
    assert bit in (1, 2, 4, 8, 16, 32)
    check_open(nkv, index, summary, chunks=(0, 16, 32))


@pytest.mark.parametrize("n", [1, 2, 3, 4, 7])
def test_open_written_pairs(nkv, n):
    rng = np.random.default_rng(0x10E0 + n)
    keys = key_pool(rng, n + 3)[:n]
    sizes = [30 + len(k) + 5 for k in keys]
    for page in sorted({1, 2, 3, n, n + 1}):
        index, summary = ref.written(keys, sizes, page)
        assert check_open(nkv, index, summary, chunks=(0, 16, 48)) == (n, sstable_ref.summary_entries(n, page))


def random_pair(rng, n, lens=None):
    pool = key_pool(rng, n + 8)
    keys = sorted(pool[i] for i in rng.choice(len(pool), n, replace=False))
    if lens is not None:
        keys = sorted({bytes(rng.integers(0, 256, ln, dtype=np.uint8)) for ln in lens for _ in range(3)})
    offs = [int(o) for o in rng.choice([-1, 0, 5, 7, 2**40, -7], len(keys))]
    named = sorted({0, len(keys) - 1, *[j for j in range(len(keys)) if rng.random() < 0.4]})
    return keys, offs, named


@pytest.mark.parametrize("seed", range(4))
def test_open_random_partitions_small_chunks(nkv, seed):
    """Chunks of 16..80 bytes make every table many chunks: entries straddle
    boundaries, keys longer than a chunk leave chunks no chain position starts in."""
    rng = np.random.default_rng(0x10F0 + seed)
    for n in (1, 2, 5, 33, 120):
        keys, offs, named = random_pair(rng, n)
        index, summary = ref.canonical(keys, offs, named)
        check_open(nkv, index, summary, chunks=(16, 32, 80), at=(seed, 3 * seed))


def test_open_key_lengths_and_prefixes(nkv):
    rng = np.random.default_rng(0x1100)
    keys, offs, named = random_pair(rng, 0, lens=(0, 1, 7, 8, 9, 16, 17))
    assert {len(k) for k in keys} == {0, 1, 7, 8, 9, 16, 17}
    check_open(nkv, *ref.canonical(keys, offs, named), chunks=(0, 32))
    # every key a proper prefix of its successor, across the 8-byte prefix
    chain = [b"samehead-and-more"[:ln] for ln in range(18)]
    check_open(nkv, *ref.canonical(chain, list(range(18)), [0, 5, 17]), chunks=(0, 32))
    # the same keys descending by one step behind the prefix: refused
    swapped = chain[:10] + [chain[11], chain[10]] + chain[12:]
    index, summary = ref.canonical(swapped, list(range(18)), [0, 5, 17])
    assert ref.open(index, summary)[3] == ref.BAD_ORDER
    check_open(nkv, index, summary, chunks=(0, 32))


@pytest.mark.parametrize("ia,sa", [(0, 0), (1, 7), (7, 15), (15, 1)])
def test_open_images_at_any_alignment(nkv, ia, sa):
    rng = np.random.default_rng(0x1110 + ia)
    keys, offs, named = random_pair(rng, 200)
    check_open(nkv, *ref.canonical(keys, offs, named), chunks=(0, 64), at=(ia, sa))


def counter_keys(n, length=16):
    return [struct.pack(">Q", i) + b"\x11" * (length - 8) for i in range(n)]


@pytest.mark.parametrize("total", [K - 1, K, K + 1, 2 * K + 1])
def test_open_payload_at_the_chunk_edges(nkv, total):
    keys = [b"\x01" + k[1:] for k in counter_keys((total - 16) // 32 - 1)]  # 32 bytes each
    rest = total - 32 * len(keys)  # 48..79 bytes for two more entries: one of 32, one of 16..47
    keys += [b"\xfe" * 16, b"\xff" * (rest - 48)]
    keys = sorted(keys)
    index, summary = ref.canonical(keys, list(range(len(keys))), list(range(len(keys))))
    assert struct.unpack_from("<Q", summary, 16)[0] == total
    check_open(nkv, index, summary)


def test_open_entry_straddles_a_chunk_boundary(nkv):
    keys = [b"\x00" * 15] + [b"\x01" + k[1:] for k in counter_keys(300)]  # 31 bytes, then 32 each: 4095 | 4127
    index, summary = ref.canonical(keys, list(range(301)), list(range(301)))
    check_open(nkv, index, summary)
    check_open(nkv, *ref.canonical(keys, list(range(301)), [0, 1, 128, 129, 300]))


def test_open_key_longer_than_a_chunk(nkv):
    keys = counter_keys(100)
    keys[50] = keys[50] + b"\x22" * (2 * K + 100)  # chunks no chain position starts in
    index, summary = ref.canonical(keys, list(range(100)), list(range(100)))
    check_open(nkv, index, summary)
    check_open(nkv, *ref.canonical(keys, list(range(100)), [0, 49, 50, 51, 99]), chunks=(0, 64))


def test_open_decoy_behind_a_chunk_boundary(nkv):
    """A key whose bytes hold the exact image of a real Summary entry, placed so
    that the image is the first position of chunk 1 that passes the link test:
    lane 1 starts on the decoy, the stitch refuses it, and the one-lane walk
    gives the exact answer."""
    keys = counter_keys(200)
    at = K // 32 - 1  # entry `at` starts at payload byte K - 32; its key bytes start at K - 16
    decoy = ref.ent(keys[3], 3 * 32)  # the Summary entry of key 3: it names Index offset 96
    keys[at] = keys[at] + decoy + b"\x33" * 7
    named = list(range(200))
    index, summary = ref.canonical(keys, list(range(200)), named)
    payload = summary[24 + len(keys[0]) + len(keys[-1]):]
    assert payload[K:K + 32] == decoy and payload[3 * 32:4 * 32] == decoy
    check_open(nkv, index, summary)


def test_open_capacity_and_size_query(nkv):
    rng = np.random.default_rng(0x1120)
    keys, offs, named = random_pair(rng, 40)
    index, summary = ref.canonical(keys, offs, named)
    want_ent, n, s, _ = ref.open(index, summary)
    fill64 = int.from_bytes(bytes([FILL]) * 8, "little")
    for path in PATHS:
        rc, ent, gn, gs, v, whole = dev_open(nkv, index, summary, path, cap=n - 1)
        assert (rc, gn, gs, v) == (INVALID, n, s, 0) and (whole == fill64).all()  # n reported, nothing written
        rc, ent, gn, gs, v, whole = dev_open(nkv, index, summary, path, cap=n)
        assert (rc, ent, gn, gs, v) == (0, want_ent, n, s, 0)
        rc, ent, gn, gs, v, whole = dev_open(nkv, index, summary, path, query=True)
        assert (rc, gn, gs, v) == (0, n, s, 0) and (whole == fill64).all()


def test_open_refuses_bad_arguments(nkv):
    _lib, ctx = nkv
    L = _lib.lib()
    index, summary = ref.canonical([b"a"], [0], [0])
    d_i, p_i = place(index, 0)
    d_s, p_s = place(summary, 0)
    n, s, v = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint32(0)
    ok = (ctx.h, p_i, len(index), p_s, len(summary), None, 0, ctypes.byref(n), ctypes.byref(s), ctypes.byref(v))
    assert L.nkv_index_open_dev(*ok) == 0 and (n.value, s.value, v.value) == (1, 1, 0)
    for at, bad in ((0, None), (1, None), (2, 0), (3, None), (4, 0), (7, None), (8, None), (9, None)):
        args = list(ok)
        args[at] = bad
        assert L.nkv_index_open_dev(*args) == INVALID, at
    for key, bad in ((_lib.NKV_OPT_INDEX_OPEN_PATH, 3), (_lib.NKV_OPT_INDEX_OPEN_PATH, -1),
                     (_lib.NKV_OPT_INDEX_OPEN_CHUNK, 8), (_lib.NKV_OPT_INDEX_OPEN_CHUNK, 4100)):
        assert L.nkv_ctx_set_option(ctx.h, key, bad) == INVALID


@pytest.mark.parametrize("page", [3, 1024])
def test_open_65536_entries(nkv, page):
    n = 65536
    keys = counter_keys(n)
    index, summary = ref.written(keys, [146] * n, page)
    assert check_open(nkv, index, summary) == (n, sstable_ref.summary_entries(n, page))


# ---------------------------------------------------------------------------
# locate

@dataclass
class World:
    pairs: list  # (index, summary) per table
    tabs: list   # (keys, stored offsets) per table
    filters: list
    pool: list
    rng: object


def make_world(oracle, seed, ns, kinds=("real", "tiny", None, "other", "k17"), minus_one=0.1):
    rng = np.random.default_rng(seed)
    pool = key_pool(rng, max(ns) * 3 // 2 + 40)
    w = World([], [], [], pool, rng)
    for t, n in enumerate(ns):
        keys = [pool[i] for i in sorted(rng.choice(len(pool), n, replace=False).tolist())]
        held = set(keys)
        offs = [-1 if rng.random() < minus_one else int(o) for o in rng.integers(-9, 2**41, n)]
        named = sorted({0, n - 1, *[j for j in range(n) if j % 3 == 0]})
        w.pairs.append(ref.canonical(keys, offs, named))
        w.tabs.append((keys, offs))
        w.filters.append(make_filter(oracle, kinds[t % len(kinds)], keys, [k for k in pool if k not in held],
                                     int(rng.integers(0, 2**32))))
    return w


@dataclass
class Up:
    structs: object
    T: int
    keep: List[object] = field(default_factory=list)
    intact: List[Callable] = field(default_factory=list)


def upload(nkv, w: World) -> Up:
    """Every Index at an odd base offset, opened on the device: the locate
    searches the offsets the open wrote."""
    _lib, ctx = nkv
    up = Up((_lib.NkvIndexTable * len(w.pairs))(), len(w.pairs))
    for t, (index, summary) in enumerate(w.pairs):
        d_i, p_i = place(index, 2 * t + 1)
        d_s, p_s = place(summary, t % 16)
        want_ent, n, _, _ = ref.open(index, summary)
        d_ent = _dev(np.zeros(n, np.uint64))
        gn, gs, v = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint32(0)
        assert _lib.lib().nkv_index_open_dev(ctx.h, p_i, len(index), p_s, len(summary), d_ent.data_ptr(), n,
                                             ctypes.byref(gn), ctypes.byref(gs), ctypes.byref(v)) == 0
        assert (gn.value, v.value) == (n, 0)
        assert d_ent.cpu().numpy().view(np.uint64).tolist() == want_ent
        f = w.filters[t]
        d_bits = _dev(f.words()) if f is not None else None
        up.structs[t] = _lib.NkvIndexTable(p_i, len(index), d_ent.data_ptr(), n, d_bits.data_ptr() if f else None,
                                           f.m if f else 0, f.k if f else 0, f.seed0 if f else 0)
        for d in (d_i, d_ent, d_bits):
            if d is not None:
                up.keep.append(d)
                up.intact.append(frozen(d))
    return up


def dev_locate(nkv, up, queries, base=0, overlay=0, preset=None, key_at=0, stage=True, err=True):
    """(rc, hit, data_off, status, stage rows, err word); preset = (hit, data_off,
    status) the outputs hold beforehand.  d_hit and d_data_off at 8-byte, d_err
    at 4-byte, the byte arrays at odd addresses."""
    _lib, ctx = nkv
    q, T = len(queries), up.T
    host, koff, klen = pack_keys(queries, key_at)
    d_keys, d_koff, d_klen = _dev(host), _dev(koff), _dev(klen)
    same = up.intact + [frozen(d_keys), frozen(d_koff), frozen(d_klen)]
    init = (None, None, None) if preset is None else (np.asarray(preset[0], np.uint64),
                                                      np.asarray(preset[1], np.int64), np.asarray(preset[2], np.uint8))
    p_hit, c_hit = guarded(8 * q, 8, fill=FILL, init=init[0])
    p_off, c_off = guarded(8 * q, 8, fill=FILL, init=init[1])
    p_status, c_status = guarded(q, 1, fill=FILL, init=init[2])
    p_stage, c_stage = guarded(q * T, 3, fill=FILL)
    p_err, c_err = guarded(4, 4, fill=FILL)
    rc = _lib.lib().nkv_locate_dev(ctx.h, up.structs, T, base, d_keys.data_ptr() + key_at, d_koff.data_ptr(),
                                   d_klen.data_ptr(), q, overlay, p_hit, p_off, p_status,
                                   p_stage if stage else None, p_err if err else None)
    ctx.sync()
    for intact in same:
        intact()
    return (rc, c_hit().view(np.uint64).tolist(), c_off().view(np.int64).tolist(), c_status().tolist(),
            c_stage().reshape(q, T).tolist(), int(c_err().view(np.uint32)[0]) if err else None)


def want_of(w: World, queries, base=0):
    passes = [lookup_ref.filter_query(f, queries) for f in w.filters]
    return ref.closed_locate_many(w.tabs, queries, passes, base)


def queries_of(w: World, q):
    """Every kind of query: below the minimum and above the maximum of every
    table, between neighbours, equal to held keys, the empty key, duplicates."""
    some = [k for keys, _ in w.tabs for k in (keys[0], keys[-1], keys[len(keys) // 2])]
    out = [b"", b"\xff" * 41, w.pool[1], w.pool[1]] + some + make_queries(w.rng, w.pool, q)
    order = w.rng.permutation(len(out))
    return [out[i] for i in order][:q]


def check_locate(nkv, w, queries, up=None, base=0, **kw):
    up = up or upload(nkv, w)
    rc, hit, off, status, stage, err = dev_locate(nkv, up, queries, base=base, **kw)
    w_hit, w_off, w_status, w_stage = want_of(w, queries, base)
    assert rc == 0 and err in (0, None)
    assert (hit, off, status) == (w_hit, w_off, w_status)
    if kw.get("stage", True):
        assert stage == w_stage
    return w_stage


def test_locate_closed_form_is_the_reader(nkv, oracle):
    """Small tables, every key of the pool: the device against the literal
    restatement of Filter.Query + FindSummaryTableEntry + FindIndexTableEntry."""
    w = make_world(oracle, 0x1200, (1, 2, 7), (None, "tiny", "other"))
    queries = w.pool + [b"\xff" * 9]
    rc, hit, off, status, stage, err = dev_locate(nkv, upload(nkv, w), queries)
    assert rc == 0 and err == 0
    for i, key in enumerate(queries):
        answered = False
        for t, (index, summary) in enumerate(w.pairs):
            if answered:
                want = ref.NOT_SEARCHED
            elif not lookup_ref.filter_query(w.filters[t], [key])[0]:
                want = ref.FILTER
            else:
                ste = sstable_ref.find_summary_table_entry(summary, key)
                ite = sstable_ref.find_index_table_entry(index, key, ste.Offset) if ste.Offset != -1 else None
                want = ref.SUMMARY if ite is None else (ref.INDEX if ite.Offset == -1 else ref.FOUND)
                if want == ref.FOUND:
                    answered = True
                    assert off[i] == ite.Offset and hit[i] >> 32 == t and status[i] == ref.LOCATED
            assert stage[i][t] == want, (key, t)
        if not answered:
            assert (hit[i], off[i], status[i]) == (ref.HIT_NONE, -1, ref.ABSENT)


@pytest.mark.parametrize("T", [1, 2, 32])
@pytest.mark.parametrize("q", [1, 63, 64, 65])
def test_locate_shapes(nkv, oracle, T, q):
    ns = tuple((1, 2, 3, 63, 64, 65, 300)[(T + t) % 7] for t in range(T))
    w = make_world(oracle, 0x1210 + T, ns)
    base = 5 if (T + q) % 2 else 0
    stages = check_locate(nkv, w, queries_of(w, q), base=base, key_at=q % 16)
    assert len(stages) == q


def test_locate_every_key_and_every_stage(nkv, oracle):
    w = make_world(oracle, 0x1220, (300, 64, 65, 7, 120))
    queries = sorted({k for keys, _ in w.tabs for k in keys}) + queries_of(w, 200)
    stages = np.asarray(check_locate(nkv, w, queries, base=5))
    assert set(np.unique(stages).tolist()) == {0, 1, 2, 3, 4}  # every stage code occurs
    up = upload(nkv, w)
    check_locate(nkv, w, queries[:100], up=up, stage=False)
    check_locate(nkv, w, queries[:100], up=up, err=False)


def test_locate_filter_rejects_a_held_key_and_minus_one_moves_on(nkv, oracle):
    rng = np.random.default_rng(0x1230)
    pool = key_pool(rng, 60)
    keys = pool[10:40]
    w = World([], [], [], pool, rng)
    # table 0: a filter built from other keys; table 1: every stored Offset -1; table 2 answers
    for offs, kind in (([7] * 30, "other"), ([-1] * 30, None), (list(range(100, 130)), "real")):
        w.pairs.append(ref.canonical(keys, offs, [0, 29]))
        w.tabs.append((keys, offs))
        w.filters.append(make_filter(oracle, kind, keys, pool[40:] + pool[:10], 5))
    stages = check_locate(nkv, w, keys + pool[:10])
    rejected = [r for r in stages[:30] if r[0] == ref.FILTER]
    assert rejected and all(r == [ref.FILTER, ref.INDEX, ref.FOUND] for r in rejected)


def test_locate_overlays_lookup_and_memtable_answers(nkv, oracle):
    """Rows that nkv_lookup_dev or nkv_memtable_find_dev answered come back
    byte-identical, with a stage row of NOT_SEARCHED; ABSENT rows are searched."""
    from tests import test_gpu_lookup as tl
    from tests import test_gpu_memtable as tm
    tabs, pool, rng = tl.make_world(oracle, 0x1240, (64, 20))
    w = make_world(oracle, 0x1240, (64, 30))  # the same seed: the same pool
    assert w.pool == pool
    queries = tl.make_queries(rng, pool, 65) + pool[:20]
    got = tl.dev_lookup(nkv, tl.upload(nkv, tabs), queries)
    assert got.rc == 0 and 0 < int((got.status == 0).sum()) < len(queries)
    sentinel = [-(i + 2) for i in range(len(queries))]  # d_data_off of answered rows: left as it was
    for preset_hit, preset_status in ((got.hit, got.status), (None, None)):
        if preset_hit is None:  # the memtable's answers over the same queries
            records = [record.New(k, b"v", 7) for k in pool[5:45:2]]
            records[3].Status |= record.RECORD_TOMBSTONE_REMOVED
            dev = tm.Dev.of(nkv, records)
            assert dev.add(0, len(records))[0] == 0
            preset_hit, preset_status, err = dev.find(queries, table_id=9)
            assert err == 0 and 0 < int((preset_status == 0).sum()) < len(queries)
        rc, hit, off, status, stage, err = dev_locate(nkv, upload(nkv, w), queries, base=11, overlay=1,
                                                      preset=(preset_hit, sentinel, preset_status))
        assert rc == 0 and err == 0
        w_hit, w_off, w_status, w_stage = want_of(w, queries, 11)
        for i in range(len(queries)):
            if preset_status[i] != 0:
                assert (hit[i], off[i], status[i]) == (int(preset_hit[i]), sentinel[i], int(preset_status[i]))
                assert stage[i] == [0, 0]
            else:
                assert (hit[i], off[i], status[i], stage[i]) == (w_hit[i], w_off[i], w_status[i], w_stage[i])


def test_locate_flags_an_entry_outside_the_image(nkv, oracle):
    """ent_off shifted by one entry: the last offset is index_len itself, so the
    range probe of entry n - 1 reaches outside the image.  No match, the flag."""
    _lib, ctx = nkv
    w = make_world(oracle, 0x1250, (20,), (None,), minus_one=0)
    up = upload(nkv, w)
    index = w.pairs[0][0]
    ent = ref.open(*w.pairs[0])[0]
    d_ent = _dev(np.asarray(ent[1:] + [len(index)], np.uint64))
    up.structs[0].ent_off = d_ent.data_ptr()
    queries = [w.tabs[0][0][-1], w.tabs[0][0][5]]
    rc, hit, off, status, stage, err = dev_locate(nkv, up, queries)
    assert (rc, err) == (0, 1) and status == [0, 0] and hit == [ref.HIT_NONE] * 2 and off == [-1, -1]
    assert stage == [[ref.INDEX], [ref.INDEX]]
    rc, *_ = dev_locate(nkv, up, queries, err=False)
    assert rc == INVALID


def test_locate_refuses_bad_arguments_and_q_0_writes_nothing(nkv, oracle):
    _lib, ctx = nkv
    L = _lib.lib()
    w = make_world(oracle, 0x1260, (5,), (None,))
    up = upload(nkv, w)
    rc, hit, off, status, stage, err = dev_locate(nkv, up, [])
    assert rc == 0 and hit == [] and err == int.from_bytes(bytes([FILL]) * 4, "little")
    d_in, d_out = _dev(np.zeros(64, np.uint8)), _dev(np.zeros(64, np.uint8))  # one empty key; the outputs apart
    p, o = d_in.data_ptr(), d_out.data_ptr()
    same = frozen(d_in)
    ok = [ctx.h, up.structs, 1, 0, p, p, p, 1, 0, o, o + 8, o + 16, None, o + 32]
    assert L.nkv_locate_dev(*ok) == 0
    ctx.sync()
    for at, bad in ((1, None), (2, 0), (2, 33), (3, 65536), (4, None), (5, None), (6, None), (7, 2**31),
                    (9, None), (10, None), (11, None)):
        args = list(ok)
        args[at] = bad
        assert L.nkv_locate_dev(*args) == INVALID, at
    many = (_lib.NkvIndexTable * 32)(*[up.structs[0]] * 32)
    out = (o, o + 8, o + 16, None, o + 32)
    assert L.nkv_locate_dev(ctx.h, many, 32, 65536 - 32, p, p, p, 1, 0, *out) == 0
    assert L.nkv_locate_dev(ctx.h, many, 32, 65536 - 31, p, p, p, 1, 0, *out) == INVALID
    ctx.sync()
    same()
    for fld, bad in (("n", 0), ("n", 2**31), ("index", None), ("ent_off", None)):
        one = (_lib.NkvIndexTable * 1)(up.structs[0])
        setattr(one[0], fld, bad)
        assert L.nkv_locate_dev(ctx.h, one, 1, 0, p, p, p, 1, 0, *out) == INVALID, fld


@pytest.mark.parametrize("filtered", [False, True], ids=["no-filter", "filter"])
@pytest.mark.parametrize("T", [1, 2])
def test_lookup_and_locate_agree_over_written_tables(nkv, oracle, T, filtered):
    """The two instantiations of the search layer's kernel over the same
    tables: nkv_lookup_dev over written Data tables and nkv_locate_dev (overlay
    0) over the Indexes sstable.index_summary_dev makes of them where they lie,
    the same filters and the same query batch.  The stage arrays and the hit
    words are the same; the statuses differ only as LIVE / TOMBSTONE against
    LOCATED (a written Index holds no -1 Offset), and a LOCATED key's Data
    offset is its record's."""
    from nakevaleng_amd import sstable
    from tests import test_gpu_lookup as tl
    _lib, ctx = nkv
    dev = _torch().device("cuda", 0)
    seen = set()
    for n in (1, 2, 3, 64):
        tabs, pool, rng = tl.make_world(oracle, 0x1280 + 8 * n + T, (n,) * T,
                                        kinds=("real", "tiny") if filtered else (None,))
        data = tl.upload(nkv, tabs)
        index = Up((_lib.NkvIndexTable * T)(), T)
        for t, tab in enumerate(tabs):
            s = data.structs[t]
            d_index, d_summary = sstable.index_summary_dev(ctx, dev, s.stream, s.stream_len, s.rec_off, n, 3)
            ctx.sync()
            assert d_index.cpu().numpy().tobytes() == tab.index
            d_ent = _dev(np.zeros(n, np.uint64))
            gn, gs, v = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint32(0)
            index_len = int(d_index.numel())
            assert _lib.lib().nkv_index_open_dev(ctx.h, d_index.data_ptr(), index_len, d_summary.data_ptr(),
                                                 d_summary.numel(), d_ent.data_ptr(), n, ctypes.byref(gn),
                                                 ctypes.byref(gs), ctypes.byref(v)) == 0
            assert (gn.value, v.value) == (n, 0)
            index.structs[t] = _lib.NkvIndexTable(d_index.data_ptr(), index_len, d_ent.data_ptr(), n, s.bits, s.m,
                                                  s.k, s.seed0)
            index.keep += [d_index, d_ent]
        held = [k for tab in tabs for k in tab.keys]
        for q in (1, 64, 65):
            queries = (held + tl.make_queries(rng, pool, q))[-q:] if q > 1 else [held[-1]]
            got = tl.dev_lookup(nkv, data, queries)
            rc, hit, off, status, stage, err = dev_locate(nkv, index, queries)
            assert (got.rc, got.err, rc, err) == (0, 0, 0, 0)
            assert stage == got.stage.tolist() and hit == got.hit.tolist()
            assert [ref.LOCATED if s in (1, 2) else s for s in got.status.tolist()] == status
            want_off = [-1 if h == ref.HIT_NONE else int(tabs[h >> 32].offsets[h & 0xFFFFFFFF]) for h in hit]
            assert off == want_off
            seen |= set(status)
    assert seen == {ref.ABSENT, ref.LOCATED}  # hits and misses both occurred


# ---------------------------------------------------------------------------
# Python, end to end

def test_open_index_raises_naming_the_bit(nkv):
    from nakevaleng_amd import sstable
    index, summary, _ = ref.hand_made()["link-one-byte-off"]
    with pytest.raises(ValueError, match="NKV_INDEX_BAD_LINK"):
        sstable.open_index(index, summary)
    with pytest.raises(ValueError, match="NKV_INDEX_BAD_HEADER"):
        sstable.open_index(index, summary[:20])


def test_get_many_on_disk_equals_get_many(nkv, tmp_path):
    """compact writes a table's files; with only its Index and filter on the
    device and its Data file on disk, get_many_on_disk gives the values get_many
    gives over the resident table -- alone, under a second resident table, and
    under a memtable."""
    from nakevaleng_amd import lsmtree, memtable, sstable
    rng = np.random.default_rng(0x1270)
    pool = key_pool(rng, 400)

    def run(keys, ts):
        recs = [record.New(k, bytes(rng.integers(0, 256, int(rng.integers(0, 300)), np.uint8)), ts) for k in keys]
        for r in recs[::7]:
            r.Status |= record.RECORD_TOMBSTONE_REMOVED
        return record.data_table(recs)

    cold = [run(pool[0:300:2], 1), run(pool[100:400:3], 2)]
    out, resident = lsmtree.compact(cold, seed=11, summary_page_size=3, resident=True)
    path = str(tmp_path) + "/"
    for ftype, data in (("data", out["table"][0]), ("index", out["index"]), ("summary", out["summary"])):
        with open(sstable.table_filename(path, "db", 2, 0, ftype), "wb") as f:
            f.write(data)
    indexed = sstable.open_index_files(path, "db", 2, 0, filter=out["filter"])
    assert indexed.n == len(out["table"][1]) and indexed.s == sstable_ref.summary_entries(indexed.n, 3)
    data_file = sstable.table_filename(path, "db", 2, 0, "data")
    queries = pool[::3] + [b"\xff" * 30, b"", pool[7], pool[7]]
    want = lsmtree.get_many([resident], queries)
    assert any(v is not None for v in want) and any(v is None for v in want)
    assert lsmtree.get_many_on_disk([indexed], [data_file], queries) == want
    located = lsmtree.locate_many([indexed], queries, base=4)
    assert all(loc is not None for loc, v in zip(located, want) if v is not None)
    assert {loc[0] for loc in located if loc is not None} == {4}

    hot = lsmtree.upload_table(run(pool[50:90], 3))
    want = lsmtree.get_many([hot, resident], queries)
    assert lsmtree.get_many_on_disk([indexed], [data_file], queries, resident=[hot]) == want

    mt = memtable.Memtable(64, 1 << 16, 0)
    mt.put_many(pool[0:30:3], [b"new-%d" % i for i in range(10)], 5)
    want = lsmtree.get_many([hot, resident], queries, memtable=mt)
    assert lsmtree.get_many_on_disk([indexed], [data_file], queries, resident=[hot], memtable=mt) == want
    assert lsmtree.get_many_on_disk([indexed], [data_file], queries, memtable=mt) == \
        lsmtree.get_many([resident], queries, memtable=mt)
