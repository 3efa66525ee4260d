"""GPU: the record encoder (nkv_encode_records_dev, its host form
nkv_encode_records / record.encode_many, and lsmtree.flush_puts) against
tests/encode_ref.py, bit for bit: the stream, d_out_off, d_crc and out_len.
Outputs lie in guarded buffers at their minimum alignment (tests/guarded.py)
and exactly the documented extent is written; inputs are snapshotted and
compared after the call; after every refusal all guard and payload bytes still
hold the fill and one good call follows."""
import ctypes
import zlib

import numpy as np
import pytest

from nakevaleng_amd import record
from tests.encode_ref import encode_many_ref
from tests.guarded import frozen, guarded
from tests.memtable_ref import flush_closed
from tests.test_memtable_ref import rec

pytestmark = pytest.mark.gpu

INVALID = 2  # NKV_ERR_INVALID
FILL = 0xA5
PLACES = (0, 1, 2, 3, 15, 16, 17, 63)  # blob residues modulo 64 past a 256-byte boundary
U64 = 2**64


def _torch():
    import torch
    return torch


def _dev(a, at=0):
    """A device copy of the array's bytes `at` bytes past a 256-byte boundary: (tensor, address)."""
    torch = _torch()
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    buf = np.zeros(at + max(raw.size, 16), np.uint8)
    buf[at:at + raw.size] = raw
    t = torch.from_numpy(buf).cuda()
    return t, t.data_ptr() + at


class Batch:
    """A batch of puts as the C struct describes it: two blobs with offset and
    length arrays (spans may overlap or repeat), and the header fields."""

    def __init__(self, kb, koff, klen, vb, voff, vlen, ts=None, ts_all=0, status=None, type_info=None):
        self.kb, self.vb = bytes(kb), bytes(vb)
        self.koff, self.klen = np.asarray(koff, np.uint64), np.asarray(klen, np.uint64)
        self.voff, self.vlen = np.asarray(voff, np.uint64), np.asarray(vlen, np.uint64)
        self.n = int(self.koff.size)
        self.ts = None if ts is None else np.asarray(ts, np.int64)
        self.ts_all = int(ts_all)
        self.status = None if status is None else np.asarray(status, np.uint8)
        self.type_info = None if type_info is None else np.asarray(type_info, np.uint8)

    @classmethod
    def packed(cls, keys, vals, **kw):
        p = record.pack_puts(keys, vals, timestamps=0)
        return cls(p["keys"].tobytes(), p["koff"], p["klen"], p["vals"].tobytes(), p["voff"], p["vlen"], **kw)

    def keys(self):
        return [self.kb[int(o):int(o) + int(l)] for o, l in zip(self.koff, self.klen)]

    def vals(self):
        return [self.vb[int(o):int(o) + int(l)] for o, l in zip(self.voff, self.vlen)]

    def reference(self):
        """(stream, offsets, checksums), computed once."""
        if not hasattr(self, "_ref"):
            self._ref = encode_many_ref(self.keys(), self.vals(), self.ts if self.ts is not None else self.ts_all,
                                        self.status, self.type_info)
        return self._ref


def encode_raw(nkv, b, out_at=0, key_at=0, val_at=0, want_crc=True, out_cap=None, query=False, room=None,
               keys_len=None, vals_len=None, n=None, one_blob=False):
    """nkv_encode_records_dev over Batch b.  The key blob lies key_at bytes past
    a 256-byte boundary, the value blob val_at (one_blob: keys and vals are the
    one key blob), d_out out_at bytes past one (any residue), d_out_off 8 and
    d_crc 4 bytes past one.  room: payload bytes of d_out (default: the
    reference length).  Returns (rc, stream, offsets, checksums, out_len) after
    checking that the inputs are intact, that no guard byte changed and that
    nothing but the documented extents was written."""
    torch = _torch()
    _lib, ctx = nkv
    nn = b.n if n is None else n
    if room is None:
        room = 30 * b.n + int(b.klen.sum()) + int(b.vlen.sum())
    t_k, p_k = _dev(np.frombuffer(b.kb, np.uint8), key_at)
    t_v, p_v = (t_k, p_k) if one_blob else _dev(np.frombuffer(b.vb, np.uint8), val_at)
    arrays = [_dev(x) for x in (b.koff, b.klen, b.voff, b.vlen)]
    opt = [None if x is None else _dev(x) for x in (b.ts, b.status, b.type_info)]
    held = [t_k, t_v] + [t for t, _ in arrays] + [x[0] for x in opt if x is not None]
    intact = [frozen(t) for t in held]
    p_out, out_check = guarded(room, out_at, fill=FILL)
    p_off, off_check = guarded(8 * b.n, 8, fill=FILL)
    p_crc, crc_check = guarded(4 * b.n, 4, fill=FILL)
    puts = _lib.NkvPuts(p_k, len(b.kb) if keys_len is None else keys_len, arrays[0][1], arrays[1][1],
                        p_v, (len(b.kb) if one_blob else len(b.vb)) if vals_len is None else vals_len,
                        arrays[2][1], arrays[3][1], opt[0][1] if opt[0] else None, b.ts_all,
                        opt[1][1] if opt[1] else None, opt[2][1] if opt[2] else None, nn)
    torch.cuda.synchronize()
    out_len = ctypes.c_uint64(7)
    rc = _lib.lib().nkv_encode_records_dev(ctx.h, ctypes.byref(puts), None if query else p_out,
                                           room if out_cap is None else out_cap, p_off,
                                           p_crc if want_crc else None, ctypes.byref(out_len))
    torch.cuda.synchronize()
    for f in intact:
        f()
    got_out, got_off, got_crc = out_check(), off_check(), crc_check()
    nb = out_len.value
    if rc != 0 or query:  # a refused call and a size query write nothing
        assert (got_out == FILL).all() and (got_off == FILL).all() and (got_crc == FILL).all()
        return rc, None, None, None, nb
    assert nb <= room and (got_out[nb:] == FILL).all()
    if not want_crc:
        assert (got_crc == FILL).all()
    return rc, got_out[:nb].tobytes(), got_off.view(np.uint64), got_crc.view(np.uint32) if want_crc else None, nb


def check_encode(nkv, b, **kw):
    want, want_off, want_crc = b.reference()
    rc, stream, off, crc, nb = encode_raw(nkv, b, **kw)
    assert rc == 0
    assert nb == len(want)
    assert np.array_equal(off, want_off)
    if crc is not None:
        assert np.array_equal(crc, want_crc)
    assert stream == want, f"first differing byte {next(i for i, (x, y) in enumerate(zip(stream, want)) if x != y)}"
    return stream


def random_batch(rng, n, kmax=33, vmax=70, empties=0.0, **kw):
    kl, vl = rng.integers(0, kmax + 1, n), rng.integers(0, vmax + 1, n)
    if empties:
        kl[rng.random(n) < empties] = 0
        vl[rng.random(n) < empties] = 0
    ts = rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64)
    return Batch.packed([rng.bytes(int(k)) for k in kl], [rng.bytes(int(v)) for v in vl], ts=ts,
                        status=rng.integers(0, 256, n).astype(np.uint8),
                        type_info=rng.integers(0, 256, n).astype(np.uint8), **kw)


def _good(nkv):
    check_encode(nkv, Batch.packed([b"k1", b"", b"key3"], [b"v", b"value two", b""], ts=[1, 2, 3]), out_at=3)


# ---------------------------------------------------------------------------
# counts

@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025])
def test_counts(nkv, n):
    rng = np.random.default_rng(0x656E + n)
    check_encode(nkv, random_batch(rng, n), out_at=n % 16)


# ---------------------------------------------------------------------------
# the tile list's bound: 16384 / 30 + 2 records in one tile

def test_header_only_records_fill_a_tile_list(nkv):
    b = Batch.packed([b""] * 1200, [b""] * 1200, ts=np.arange(1200) - 600)
    assert len(b.reference()[0]) == 30 * 1200
    check_encode(nkv, b, out_at=7)


def test_empty_records_alternating_with_one_byte_keys(nkv):
    keys = [b"" if i % 2 == 0 else bytes([i & 0xFF]) for i in range(1200)]
    check_encode(nkv, Batch.packed(keys, [b""] * 1200, ts=np.arange(1200)), out_at=9, key_at=1)


# ---------------------------------------------------------------------------
# piece boundaries at every residue of d_out

KLENS = (0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65)
VLENS = (0, 1, 3, 4, 5, 29, 30, 31, 63, 64, 65, 127, 128, 129, 200, 4050, 4096, 20000)
_pairs = {}


def all_pairs():
    """Every (key length, value length) pair in one batch, built once."""
    if "b" not in _pairs:
        rng = np.random.default_rng(0x7062)
        keys = [rng.bytes(k) for k in KLENS for _ in VLENS]
        vals = [rng.bytes(v) for _ in KLENS for v in VLENS]
        n = len(keys)
        _pairs["b"] = Batch.packed(keys, vals, ts=rng.integers(-2**40, 2**40, n), status=np.arange(n) & 0xFF,
                                   type_info=(np.arange(n) * 7) & 0xFF)
        _pairs["b"].reference()
    return _pairs["b"]


@pytest.mark.parametrize("s", range(16))
def test_piece_boundaries_at_every_residue(nkv, s):
    check_encode(nkv, all_pairs(), out_at=s, key_at=PLACES[s % 8], val_at=PLACES[(s + 3) % 8])


# ---------------------------------------------------------------------------
# a long record among short ones

@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_one_long_value_among_short_puts(nkv, where):
    rng = np.random.default_rng(0x6C67)
    kl, vl = rng.integers(0, 20, 3000), rng.integers(0, 40, 3000)
    keys, vals = [rng.bytes(int(k)) for k in kl], [rng.bytes(int(v)) for v in vl]
    vals[{"first": 0, "middle": 1500, "last": 2999}[where]] = rng.bytes(1 << 20)
    check_encode(nkv, Batch.packed(keys, vals, ts=rng.integers(0, 2**33, 3000)), out_at=5, key_at=3, val_at=17)


# ---------------------------------------------------------------------------
# shared and overlapping sources

def test_shared_and_overlapping_spans(nkv):
    """One blob for keys and values: every record uses the same key span, the
    value spans overlap and lie in descending offset order, and one value span
    is the key span itself."""
    rng = np.random.default_rng(0x6F76)
    blob = rng.bytes(5000)
    n = 400
    koff, klen = np.full(n, 37), np.full(n, 21)
    voff = np.asarray([4900 - 12 * i for i in range(n)])
    vlen = np.asarray([(i * 5) % 90 for i in range(n)])
    voff[200], vlen[200] = 37, 21
    b = Batch(blob, koff, klen, blob, voff, vlen, ts=np.arange(n))
    check_encode(nkv, b, out_at=11, key_at=2, one_blob=True)


# ---------------------------------------------------------------------------
# header fields

TS = (-2**63, -1, 0, 2**63 - 1)
STATUS = (0, 1, 0xFF)
TYPES = (0, 7, 0xFF)


def _fields():
    combos = [(t, s, y) for t in TS for s in STATUS for y in TYPES]
    rng = np.random.default_rng(0x6866)
    keys = [rng.bytes(i % 9) for i in range(len(combos))]
    vals = [rng.bytes(i % 23) for i in range(len(combos))]
    return keys, vals, [c[0] for c in combos], [c[1] for c in combos], [c[2] for c in combos]


@pytest.mark.parametrize("absent", ["none", "ts", "status", "type", "all"])
def test_header_fields(nkv, absent):
    keys, vals, ts, st, ty = _fields()
    kw = {"ts": ts, "status": st, "type_info": ty}
    if absent in ("ts", "all"):
        kw["ts"], kw["ts_all"] = None, -0x0102030405060708
    if absent in ("status", "all"):
        kw["status"] = None
    if absent in ("type", "all"):
        kw["type_info"] = None
    b = Batch.packed(keys, vals, **kw)
    with_crc = check_encode(nkv, b, out_at=13)
    assert check_encode(nkv, b, out_at=13, want_crc=False) == with_crc


# ---------------------------------------------------------------------------
# size query

def test_size_query(nkv):
    _lib, ctx = nkv
    rng = np.random.default_rng(0x7371)
    b = random_batch(rng, 700)
    want = len(b.reference()[0])
    rc, _, _, _, nb = encode_raw(nkv, b, query=True)  # d_out_off and d_crc given: their guards and payloads untouched
    assert (rc, nb) == (0, want)
    arrays = [_dev(x) for x in (b.koff, b.klen, b.voff, b.vlen)]
    t_k, p_k = _dev(np.frombuffer(b.kb, np.uint8))
    t_v, p_v = _dev(np.frombuffer(b.vb, np.uint8))
    puts = _lib.NkvPuts(p_k, len(b.kb), arrays[0][1], arrays[1][1], p_v, len(b.vb), arrays[2][1], arrays[3][1], None,
                        0, None, None, b.n)
    _torch().cuda.synchronize()
    out_len = ctypes.c_uint64(7)
    assert _lib.lib().nkv_encode_records_dev(ctx.h, ctypes.byref(puts), None, 0, None, None,
                                             ctypes.byref(out_len)) == 0
    assert out_len.value == want
    _good(nkv)


# ---------------------------------------------------------------------------
# refusals

def _refusal_batch():
    rng = np.random.default_rng(0x7266)
    return random_batch(rng, 130, kmax=12, vmax=20)


@pytest.mark.parametrize("at", ["first", "last", "second_wave"])
@pytest.mark.parametrize("kind", ["off_past_len", "len_one_too_long", "off_wraps"])
@pytest.mark.parametrize("side", ["key", "value"])
def test_bad_spans_are_refused(nkv, side, kind, at):
    b = _refusal_batch()
    i = {"first": 0, "last": b.n - 1, "second_wave": 70}[at]
    off, ln, blob = (b.koff, b.klen, len(b.kb)) if side == "key" else (b.voff, b.vlen, len(b.vb))
    off, ln = off.copy(), ln.copy()
    if kind == "off_past_len":
        off[i] = blob + 1
    elif kind == "len_one_too_long":
        ln[i] = blob - int(off[i]) + 1
    else:
        off[i], ln[i] = U64 - 1, 2
    bad = Batch(b.kb, off if side == "key" else b.koff, ln if side == "key" else b.klen,
                b.vb, off if side == "value" else b.voff, ln if side == "value" else b.vlen, ts=b.ts)
    rc, *_ = encode_raw(nkv, bad, room=len(b.reference()[0]) + 64)
    assert rc == INVALID
    _good(nkv)


def test_out_cap_one_short_reports_the_length(nkv):
    b = _refusal_batch()
    want = len(b.reference()[0])
    rc, _, _, _, nb = encode_raw(nkv, b, out_cap=want - 1)
    assert (rc, nb) == (INVALID, want)
    _good(nkv)


def test_blob_lengths_that_wrap_are_refused(nkv):
    b = Batch.packed([b"k"], [b"v"])
    rc, *_ = encode_raw(nkv, b, keys_len=2**63, vals_len=2**63)
    assert rc == INVALID
    _good(nkv)


def test_too_many_puts_are_refused_before_anything_is_read(nkv):
    b = Batch.packed([b"k", b"kk"], [b"v", b""])  # small dummy arrays: n = 2^31 may not read them
    rc, *_ = encode_raw(nkv, b, n=2**31)
    assert rc == INVALID
    _good(nkv)


def test_null_pointers_are_refused(nkv):
    _lib, ctx = nkv
    torch = _torch()
    L = _lib.lib()
    b = Batch.packed([b"a", b"bc"], [b"xyz", b""], ts=[4, 5])
    want, want_off, _ = b.reference()
    dev = {k: _dev(v) for k, v in (("keys", np.frombuffer(b.kb, np.uint8)), ("vals", np.frombuffer(b.vb, np.uint8)),
                                   ("koff", b.koff), ("klen", b.klen), ("voff", b.voff), ("vlen", b.vlen))}
    p_out, out_check = guarded(len(want), 1, fill=FILL)
    p_off, off_check = guarded(16, 8, fill=FILL)
    torch.cuda.synchronize()
    out_len = ctypes.c_uint64(7)
    ok = dict(ctx=ctx.h, out=p_out, oo=p_off, ol=ctypes.byref(out_len), puts=True,
              **{k: v[1] for k, v in dev.items()})

    def call(**kw):
        p = dict(ok, **kw)
        puts = _lib.NkvPuts(p["keys"], len(b.kb), p["koff"], p["klen"], p["vals"], len(b.vb), p["voff"], p["vlen"],
                            None, 9, None, None, 2)
        rc = L.nkv_encode_records_dev(p["ctx"], ctypes.byref(puts) if p["puts"] else None, p["out"], len(want),
                                      p["oo"], None, p["ol"])
        torch.cuda.synchronize()
        return rc

    for name in ("ctx", "puts", "ol", "koff", "klen", "voff", "vlen", "keys", "vals", "oo"):
        assert call(**{name: None}) == INVALID, name
        assert (out_check() == FILL).all() and (off_check() == FILL).all(), name
    assert call() == 0 and out_len.value == len(want)
    assert out_check().tobytes() == encode_many_ref(b.keys(), b.vals(), 9)[0]
    assert np.array_equal(off_check().view(np.uint64), want_off)
    _good(nkv)


def test_no_puts(nkv):
    _lib, ctx = nkv
    rc, stream, off, crc, nb = encode_raw(nkv, Batch.packed([], []))
    assert (rc, stream, nb) == (0, b"", 0) and off.size == 0 and crc.size == 0
    puts = _lib.NkvPuts()
    out_len = ctypes.c_uint64(7)
    assert _lib.lib().nkv_encode_records_dev(ctx.h, ctypes.byref(puts), None, 0, None, None,
                                             ctypes.byref(out_len)) == 0
    assert out_len.value == 0
    _good(nkv)


def test_timing_intervals(nkv):
    _lib, ctx = nkv
    rng = np.random.default_rng(0x7469)
    b = random_batch(rng, 3000)
    ctx.set_timing(True)
    try:
        check_encode(nkv, b)
        leaf, reduce_ = ctx.last_timing()
        assert leaf > 0 and reduce_ > 0
    finally:
        ctx.set_timing(False)


# ---------------------------------------------------------------------------
# round trips through the existing entries

def _encode_on_device(nkv, b, out_at=0):
    """The encoded log left on the device: (tensor, address, n bytes, offsets tensor, checksums tensor)."""
    torch = _torch()
    _lib, ctx = nkv
    want = b.reference()[0]
    held = [_dev(np.frombuffer(x, np.uint8)) for x in (b.kb, b.vb)] + [_dev(x) for x in (b.koff, b.klen, b.voff, b.vlen)]
    opt = [None if x is None else _dev(x) for x in (b.ts, b.status, b.type_info)]
    puts = _lib.NkvPuts(held[0][1], len(b.kb), held[2][1], held[3][1], held[1][1], len(b.vb), held[4][1], held[5][1],
                        opt[0][1] if opt[0] else None, b.ts_all, opt[1][1] if opt[1] else None,
                        opt[2][1] if opt[2] else None, b.n)
    d_log = torch.zeros(len(want) + 16, dtype=torch.uint8, device="cuda")
    d_off = torch.zeros(8 * b.n, dtype=torch.uint8, device="cuda")
    d_crc = torch.zeros(4 * b.n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    out_len = ctypes.c_uint64(0)
    _lib.check(_lib.lib().nkv_encode_records_dev(ctx.h, ctypes.byref(puts), d_log.data_ptr() + out_at, len(want),
                                                 d_off.data_ptr(), d_crc.data_ptr(), ctypes.byref(out_len)))
    assert out_len.value == len(want)
    ctx.sync()  # the inputs are released on return: the encode has to be through with them
    return d_log, d_log.data_ptr() + out_at, len(want), d_off, d_crc


def test_the_encoded_log_passes_the_record_checksum_check(nkv):
    torch = _torch()
    _lib, ctx = nkv
    rng = np.random.default_rng(0x7263)
    b = random_batch(rng, 2500, vmax=300, empties=0.1)
    d_log, p_log, nbytes, d_off, d_crc = _encode_on_device(nkv, b, out_at=1)
    d_crc2 = torch.zeros(4 * b.n, dtype=torch.uint8, device="cuda")
    d_stats = torch.zeros(24, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    _lib.check(_lib.lib().nkv_record_crc_dev(ctx.h, p_log, nbytes, d_off.data_ptr(), b.n, d_crc2.data_ptr(),
                                             d_stats.data_ptr()))
    ctx.sync()
    assert d_stats.cpu().numpy().view(np.uint64).tolist() == [0, U64 - 1, 0]
    assert np.array_equal(d_crc2.cpu().numpy(), d_crc.cpu().numpy())
    assert np.array_equal(d_crc.cpu().numpy().view(np.uint32), b.reference()[2])


def test_the_encoded_log_feeds_the_sort(nkv):
    """5,000 puts over 1,500 keys with tombstones: nkv_sort_records_dev over the
    encoded log equals the closed-form flush of the same records."""
    torch = _torch()
    _lib, ctx = nkv
    rng = np.random.default_rng(0x7374)
    pool = sorted({rng.bytes(int(rng.integers(0, 25))) for _ in range(1600)})[:1500]
    n = 5000
    keys = [pool[j] for j in rng.integers(0, len(pool), n)]
    tomb = rng.random(n) < 0.2
    vals = [b"" if t else rng.bytes(int(v)) for t, v in zip(tomb, rng.integers(0, 80, n))]
    ts = rng.integers(100, 110, n)
    b = Batch.packed(keys, vals, ts=ts, status=tomb.astype(np.uint8))
    d_log, p_log, nbytes, d_off, _ = _encode_on_device(nkv, b)
    d_out = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    d_oo = torch.zeros(8 * n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    n_out, out_len = ctypes.c_uint64(), ctypes.c_uint64()
    _lib.check(_lib.lib().nkv_sort_records_dev(ctx.h, p_log, nbytes, d_off.data_ptr(), n, d_out.data_ptr(), nbytes,
                                               d_oo.data_ptr(), None, ctypes.byref(n_out), ctypes.byref(out_len)))
    recs = [rec(k, int(t), v, tomb=bool(d)) for k, t, v, d in zip(keys, ts, vals, tomb)]
    want = b"".join(r.ToBytes() for r in flush_closed(recs)[0])
    assert (n_out.value, out_len.value) == (len(flush_closed(recs)[0]), len(want))
    assert d_out.cpu().numpy()[:out_len.value].tobytes() == want


# ---------------------------------------------------------------------------
# the host form and the Python layer

def test_encode_many(nkv):
    _lib, ctx = nkv
    rng = np.random.default_rng(0x656D)
    b = random_batch(rng, 2100, vmax=200, empties=0.1)
    want, want_off, want_crc = b.reference()
    stream, sizes = record.encode_many(b.keys(), b.vals(), b.ts, b.status, b.type_info, ctx=ctx)
    assert stream == want
    assert np.array_equal(sizes, np.diff(np.append(want_off, np.uint64(len(want)))))
    # one value for the batch, and record.New's defaults
    stream, _ = record.encode_many(b.keys(), b.vals(), 77, 1, 9, ctx=ctx)
    assert stream == encode_many_ref(b.keys(), b.vals(), 77, 1, 9)[0]
    stream, sizes = record.encode_many([b"k"], [b"v"], ctx=ctx)
    r, end = record.parse(stream)
    assert end == 32 and (r.Key, r.Value, r.Status, r.TypeInfo) == (b"k", b"v", 0, 0) and r.Timestamp > 1600000000
    assert record.encode_many([], [], ctx=ctx)[0] == b""
    with pytest.raises(ValueError):
        record.encode_many([b"a", b"b"], [b"x", b"y"], timestamps=[1, 2, 3], ctx=ctx)
    # the C entry itself: checksums, the size query, a capacity one short
    p = record.pack_puts(b.keys(), b.vals(), b.ts)
    puts = _lib.NkvPuts(p["keys"].ctypes.data, p["keys"].size, p["koff"].ctypes.data, p["klen"].ctypes.data,
                        p["vals"].ctypes.data, p["vals"].size, p["voff"].ctypes.data, p["vlen"].ctypes.data,
                        p["ts"].ctypes.data, 0, None, None, b.n)
    out, osz, crc = np.zeros(len(want), np.uint8), np.zeros(b.n, np.uint64), np.zeros(b.n, np.uint32)
    out_len = ctypes.c_uint64(7)

    def call(o, cap):
        return _lib.lib().nkv_encode_records(ctx.h, ctypes.byref(puts), o, cap, osz.ctypes.data, crc.ctypes.data,
                                             ctypes.byref(out_len))

    assert call(None, 0) == 0 and out_len.value == len(want)
    assert call(out.ctypes.data, len(want) - 1) == INVALID and out_len.value == len(want) and not out.any()
    assert call(out.ctypes.data, len(want)) == 0
    assert out.tobytes() == encode_many_ref(b.keys(), b.vals(), b.ts)[0] and np.array_equal(crc, want_crc)


@pytest.fixture(scope="module")
def put_world():
    """4,000 puts over 1,200 keys with tombstones, and the records they stand for."""
    rng = np.random.default_rng(0x7075)
    pool = sorted({rng.bytes(int(rng.integers(1, 20))) for _ in range(1300)})[:1200]
    n = 4000
    keys = [pool[j] for j in rng.integers(0, len(pool), n)]
    tomb = rng.random(n) < 0.15
    vals = [b"" if t else rng.bytes(int(v)) for t, v in zip(tomb, rng.integers(0, 150, n))]
    ts = np.sort(rng.integers(1000, 1400, n))
    recs = [rec(k, int(t), v, tomb=bool(d)) for k, t, v, d in zip(keys, ts, vals, tomb)]
    return keys, vals, ts, tomb.astype(np.uint8), recs


def test_flush_puts_equals_flush_log(nkv, put_world):
    from nakevaleng_amd import lsmtree
    keys, vals, ts, status, recs = put_world
    tab = record.data_table(recs)
    want = lsmtree.flush_log(tab, device=0, seed=99, summary_page_size=7)
    got = lsmtree.flush_puts(keys, vals, ts, status, device=0, seed=99, summary_page_size=7)
    assert sorted(got) == sorted(list(want) + ["log"])
    assert got["table"][0] == want["table"][0] and np.array_equal(got["table"][1], want["table"][1])
    for k in ("root", "image", "index", "summary"):
        assert got[k] == want[k], k
    assert np.array_equal(got["sources"], want["sources"])
    assert (got["filter"].M, got["filter"].K, got["filter"].HashSeeds) == \
        (want["filter"].M, want["filter"].K, want["filter"].HashSeeds)
    assert got["filter"].Contents == want["filter"].Contents
    assert got["log"][0] == tab[0] and np.array_equal(got["log"][1], tab[1])
    plain = lsmtree.flush_puts(keys, vals, ts, status, device=0)
    assert sorted(plain) == ["filter", "image", "log", "root", "sources", "table"] and plain["filter"] is None
    assert plain["root"] == want["root"]


def test_flush_puts_resident_answers_get_many(nkv, put_world):
    from nakevaleng_amd import lsmtree
    keys, vals, ts, status, recs = put_world
    out, handle = lsmtree.flush_puts(keys, vals, ts, status, device=0, seed=5, resident=True)
    state = {}
    for k, v, s in zip(keys, vals, status):
        state[k] = None if s else v
    queries = sorted(state) + [b"\xff" * 21, b""]
    want = [state.get(q) for q in queries]
    assert None in want[:len(state)] and sum(v is not None for v in want) > 500
    assert lsmtree.get_many([handle], queries) == want
    assert "log" in out


def test_flush_puts_of_no_puts_raises_the_reference_error(nkv):
    from nakevaleng_amd import lsmtree
    from nakevaleng_amd.merkletree import MerkleTreeError
    with pytest.raises(MerkleTreeError) as e:
        lsmtree.flush_puts([], [], device=0)
    assert str(e.value) == "cannot build Merkle Tree from 0 nodes"
    _good(nkv)


# ---------------------------------------------------------------------------
# fuzz

@pytest.mark.parametrize("round_", range(30))
def test_fuzz(nkv, round_):
    rng = np.random.default_rng(0x667A + round_)
    n = int(rng.integers(1, 3001))
    vmax = int(rng.choice([8, 70, 400]))
    b = random_batch(rng, n, kmax=int(rng.choice([4, 33, 90])), vmax=vmax, empties=0.1)
    if rng.random() < 0.5:
        b.ts, b.ts_all = None, int(rng.integers(-2**63, 2**63 - 1, dtype=np.int64))
    if rng.random() < 0.5:
        b.status = None
    if rng.random() < 0.5:
        b.type_info = None
    check_encode(nkv, b, out_at=int(rng.integers(0, 16)), key_at=int(rng.integers(0, 64)),
                 val_at=int(rng.integers(0, 64)), want_crc=bool(rng.random() < 0.7))
