"""core/record byte format -- the input side of the Merkle step (host code, no hashing).

Layout written by record.Serialize (core/record/record.go:191-199), little endian:
  Crc u32 | Timestamp i64 | Status u8 | TypeInfo u8 | KeySize u64 | ValueSize u64 | Key | Value
TotalSize = 30 + KeySize + ValueSize (record.go:44-46); Crc = CRC-32/IEEE over
Key || Value (record.go:51).  The Merkle leaf of a record is SHA-1(Value) only
(core/sstable/sstable.go:62, core/lsmtree/lsmtree.go:211).
"""
from __future__ import annotations

import struct
import time
import zlib
from dataclasses import dataclass
from typing import Iterable, List, Tuple

import numpy as np

HEADER_SIZE = 30  # 4 + 8 + 1 + 1 + 8 + 8
RECORD_STATUS_DEFAULT = 0
RECORD_TOMBSTONE_REMOVED = 1
_HDR = struct.Struct("<IqBBQQ")


@dataclass
class Record:  # record.go:26-35
    Crc: int
    Timestamp: int
    Status: int
    TypeInfo: int
    KeySize: int
    ValueSize: int
    Key: bytes
    Value: bytes

    def TotalSize(self) -> int:  # record.go:44-46
        return HEADER_SIZE + self.KeySize + self.ValueSize

    def ToBytes(self) -> bytes:  # record.go:175-187
        return _HDR.pack(self.Crc, self.Timestamp, self.Status, self.TypeInfo, self.KeySize,
                         self.ValueSize) + self.Key + self.Value

    def IsDeleted(self) -> bool:  # record.go:96-98
        return (self.Status & RECORD_TOMBSTONE_REMOVED) == RECORD_TOMBSTONE_REMOVED


def New(key: bytes, val: bytes, timestamp: int = None) -> Record:  # record.go:49-60
    key, val = bytes(key), bytes(val)
    return Record(zlib.crc32(key + val) & 0xFFFFFFFF,
                  int(time.time()) if timestamp is None else int(timestamp),
                  RECORD_STATUS_DEFAULT, 0, len(key), len(val), key, val)


def parse(buf: bytes, off: int = 0) -> Tuple[Record, int]:
    """record.Deserialize (record.go:119-172) on an in-memory buffer: returns
    (record, next offset); raises ValueError on a CRC mismatch (the reference panics)."""
    crc, ts, st, ti, ks, vs = _HDR.unpack_from(buf, off)
    k0 = off + HEADER_SIZE
    key = bytes(buf[k0:k0 + ks])
    val = bytes(buf[k0 + ks:k0 + ks + vs])
    if len(key) != ks or len(val) != vs:
        raise EOFError("truncated record")
    if zlib.crc32(key + val) & 0xFFFFFFFF != crc:
        raise ValueError(f"Bad Record checksum (got {zlib.crc32(key + val)}, expected {crc})")
    return Record(crc, ts, st, ti, ks, vs, key, val), k0 + ks + vs


def data_table(records: Iterable[Record]) -> Tuple[bytes, np.ndarray]:
    """The Data-table byte stream (sstable/datatable.go) and each record's
    TotalSize (KeyContext.RecSize, record.go:38-41)."""
    parts: List[bytes] = []
    sizes: List[int] = []
    for r in records:
        b = r.ToBytes()
        parts.append(b)
        sizes.append(len(b))
    return b"".join(parts), np.asarray(sizes, dtype=np.uint64)


def _per_record(what, x, n, dtype):
    """None, one int for the batch, or a sequence of n: (array or None, the one value)."""
    if x is None:
        return None, 0
    if np.ndim(x) == 0:
        return None, int(x)
    a = np.ascontiguousarray(x, dtype=dtype)
    if a.shape != (n,):
        raise ValueError(f"{what}: {a.size} entries for {n} records")
    return a, 0


def pack_puts(keys, values, timestamps=None, status=None, type_info=None):
    """A batch of puts as nkv_puts takes it: the keys and the values packed one
    behind the other, their offset and length arrays, and the per-record header
    fields.  Returns a dict of numpy arrays (ts / status / type None where one
    value serves the batch) with "ts_all" and "n".  timestamps None stamps one
    int(time.time()) for the batch, as record.New does per record."""
    keys, values = [bytes(k) for k in keys], [bytes(v) for v in values]
    n = len(keys)
    if len(values) != n:
        raise ValueError(f"encode: {n} keys and {len(values)} values")
    klen = np.fromiter((len(k) for k in keys), dtype=np.uint64, count=n)
    vlen = np.fromiter((len(v) for v in values), dtype=np.uint64, count=n)
    koff, voff = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    if n > 1:
        koff[1:], voff[1:] = np.cumsum(klen[:-1]), np.cumsum(vlen[:-1])
    ts, ts_all = _per_record("timestamps", int(time.time()) if timestamps is None else timestamps, n, np.int64)
    st, st_all = _per_record("status", status, n, np.uint8)
    ty, ty_all = _per_record("type_info", type_info, n, np.uint8)
    if st is None and st_all:
        st = np.full(n, st_all, np.uint8)
    if ty is None and ty_all:
        ty = np.full(n, ty_all, np.uint8)
    return {"keys": np.frombuffer(b"".join(keys), np.uint8), "koff": koff, "klen": klen,
            "vals": np.frombuffer(b"".join(values), np.uint8), "voff": voff, "vlen": vlen,
            "ts": ts, "ts_all": ts_all, "status": st, "type": ty, "n": n}


def encode_many(keys, values, timestamps=None, status=None, type_info=None, ctx=None) -> Tuple[bytes, np.ndarray]:
    """record.New(key, val).ToBytes() for a batch of puts on the device
    (nkv_encode_records; record.go:49-60, 175-187): the write log, which is what
    the WAL appends (wal.go:199-232), and each record's TotalSize.  timestamps:
    None = one int(time.time()) for the batch, an int = that value in every
    record, a sequence = one per record; status and type_info: None (0), an int
    or a sequence.  A length mismatch raises ValueError."""
    import ctypes
    from nakevaleng_amd import _lib
    ctx = ctx or _lib.default_context()
    p = pack_puts(keys, values, timestamps, status, type_info)
    n = p["n"]

    def ptr(a):
        return None if a is None or a.size == 0 else a.ctypes.data

    puts = _lib.NkvPuts(ptr(p["keys"]), p["keys"].size, ptr(p["koff"]), ptr(p["klen"]), ptr(p["vals"]),
                        p["vals"].size, ptr(p["voff"]), ptr(p["vlen"]), ptr(p["ts"]), p["ts_all"], ptr(p["status"]),
                        ptr(p["type"]), n)
    total = 30 * n + int(p["klen"].sum()) + int(p["vlen"].sum())
    out = np.zeros(total + 1, np.uint8)
    sizes = np.zeros(n + 1, np.uint64)
    out_len = ctypes.c_uint64(0)
    _lib.check(_lib.lib().nkv_encode_records(ctx.h, ctypes.byref(puts), out.ctypes.data, total, sizes.ctypes.data,
                                             None, ctypes.byref(out_len)), "record encode")
    return out[:out_len.value].tobytes(), sizes[:n].copy()


def value_spans(stream: bytes, rec_sizes: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """Host reference for the value locator: (offset, length) of each Value."""
    offs = np.zeros(len(rec_sizes), np.uint64)
    lens = np.zeros(len(rec_sizes), np.uint64)
    p = 0
    for i, rs in enumerate(rec_sizes):
        _, _, _, _, ks, vs = _HDR.unpack_from(stream, p)
        offs[i] = p + HEADER_SIZE + ks
        lens[i] = vs
        p += int(rs)
    return offs, lens


def checksums(stream, rec_sizes, ctx=None) -> Tuple[np.ndarray, int, int]:
    """Device CRC-32/IEEE of every record's Key || Value in a Data-table stream
    (nkv_record_crc; record.go:51 and :163-169).  Returns (checksums, number of
    records whose stored Crc differs, lowest such index or -1)."""
    import ctypes
    from nakevaleng_amd import _lib
    ctx = ctx or _lib.default_context()
    buf = np.frombuffer(bytes(stream), np.uint8) if not isinstance(stream, np.ndarray) else stream
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    sizes = np.ascontiguousarray(rec_sizes, dtype=np.uint64)
    n = sizes.size
    crc = np.zeros(max(n, 1), np.uint32)
    bad, first = ctypes.c_uint64(0), ctypes.c_uint64(0)
    _lib.check(_lib.lib().nkv_record_crc(ctx.h, _lib.p8(buf if buf.size else np.zeros(1, np.uint8)), buf.size,
                                         _lib.p64(sizes if n else np.zeros(1, np.uint64)), n,
                                         crc.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                         ctypes.byref(bad), ctypes.byref(first)))
    return crc[:n], int(bad.value), (-1 if first.value == 2**64 - 1 else int(first.value))


def verify(stream, rec_sizes, ctx=None) -> np.ndarray:
    """record.Deserialize's checksum check over a whole Data-table stream on the
    device: raises ValueError with the reference's message (record.go:166-167)
    for the first bad record, else returns the checksums."""
    crc, bad, first = checksums(stream, rec_sizes, ctx)
    if bad:
        off = int(np.sum(np.asarray(rec_sizes, dtype=np.uint64)[:first]))
        stored = _HDR.unpack_from(bytes(stream), off)[0]
        raise ValueError(f"Bad Record checksum (got {int(crc[first])}, expected {stored})")
    return crc


def frame(stream, segments=None, strict: bool = False, ctx=None):
    """The record boundaries of raw bytes on the device (nkv_frame_records): the
    loop of record.Deserialize (record.go:119-172) that the reference runs over
    a Data file (lsmtree.go:137-231) and over every WAL segment (wal.go:293-328).
    `segments` (optional) lists the segments' start offsets, non-decreasing;
    None is the one segment that is the whole stream.  A record never crosses a
    segment's end, and what is left of a segment behind its last whole record
    is its tail: dropped, as Deserialize's eof drops it, or with `strict`
    refused with a ValueError that names where the first tail starts.

    Returns (rec_sizes, seg_first, seg_len, stats): each record's TotalSize,
    the index of every segment's first record with n appended, the bytes of
    whole records in every segment, and stats = [n, sum of seg_len, segments
    with a tail, the lowest such segment or 2**64 - 1].  Checksums are not
    checked here (record.verify does that)."""
    import ctypes
    from nakevaleng_amd import _lib
    ctx = ctx or _lib.default_context()
    buf = np.frombuffer(bytes(stream), np.uint8) if not isinstance(stream, np.ndarray) else stream
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    L = buf.size
    seg = None if segments is None else np.ascontiguousarray(segments, dtype=np.uint64)
    S = 0 if seg is None else int(seg.size)
    if seg is not None and S == 0:
        raise ValueError("frame: an empty list of segments (None is the whole stream)")
    f = _lib.lib().nkv_frame_records
    n_out, stats = ctypes.c_uint64(0), (ctypes.c_uint64 * 4)()
    p_buf = buf.ctypes.data if L else None
    p_seg = seg.ctypes.data if S else None
    flags = _lib.NKV_FRAME_STRICT if strict else 0

    def refused():
        if strict and stats[2]:
            j = int(stats[3])
            at = int(stats[1]) if S == 0 else None
            where = f"at byte {at}" if at is not None else f"in segment {j}"
            return ValueError(f"frame: {int(stats[2])} segment(s) end in bytes that are no whole record, "
                              f"the first {where}")
        return _lib.NkvError(_lib.NKV_ERR_INVALID, "frame")

    cap = L // HEADER_SIZE  # a record spends at least its header
    sizes, first, seg_len = np.zeros(cap + 1, np.uint64), np.zeros(S + 2, np.uint64), np.zeros(S + 1, np.uint64)
    rc = f(ctx.h, p_buf, L, p_seg, S, flags, sizes.ctypes.data, cap, first.ctypes.data, seg_len.ctypes.data,
           ctypes.byref(n_out), stats)
    if rc == _lib.NKV_ERR_INVALID:
        raise refused()
    _lib.check(rc, "frame")
    n = int(n_out.value)
    if S == 0:  # the one segment, as a caller who listed it would get it
        first, seg_len = np.asarray([0, n], np.uint64), np.asarray([stats[1]], np.uint64)
    else:
        first, seg_len = first[:S + 1].copy(), seg_len[:S].copy()
    return sizes[:n].copy(), first, seg_len, [int(x) for x in stats]
