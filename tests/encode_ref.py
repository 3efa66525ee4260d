"""The byte layout of record.New(key, val).ToBytes() (core/record/record.go:49-60,
175-187), restated on its own: the reference the record encoder is held to.

    Crc u32 | Timestamp i64 | Status u8 | TypeInfo u8 | KeySize u64 | ValueSize u64 | Key | Value

little endian, Crc = CRC-32/IEEE of Key ++ Value.  A batch is its records one
behind the other in input order (what wal.flushPartialBufferToSegment appends).
"""
import struct
import zlib

import numpy as np


def encode_ref(key, val, ts=0, status=0, type_info=0) -> bytes:
    key, val = bytes(key), bytes(val)
    return struct.pack("<IqBBQQ", zlib.crc32(key + val), ts, status, type_info, len(key), len(val)) + key + val


def _field(x, i, default=0):
    if x is None:
        return default
    return int(x) if np.ndim(x) == 0 else int(x[i])


def encode_many_ref(keys, vals, ts=0, status=None, type_info=None):
    """(stream, offsets u64, checksums u32) of a batch; ts / status / type_info
    are one value for the batch or one per record."""
    parts = [encode_ref(k, v, _field(ts, i), _field(status, i), _field(type_info, i))
             for i, (k, v) in enumerate(zip(keys, vals))]
    off = np.zeros(len(parts), np.uint64)
    if len(parts) > 1:
        off[1:] = np.cumsum([len(p) for p in parts[:-1]])
    crc = np.asarray([zlib.crc32(bytes(k) + bytes(v)) for k, v in zip(keys, vals)], np.uint32)
    return b"".join(parts), off, crc
