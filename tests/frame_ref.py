"""Host references for nkv_frame_records[_dev]: the record boundaries of a raw
byte stream cut into segments.

deserialize_loop restates the reference literally: record.Deserialize
(core/record/record.go:119-172) over a byte reader, field by field, each read
ending the segment on io.EOF / io.ErrUnexpectedEOF, called until it reports eof
as wal.readEntireSegment (core/wal/wal.go:293-328) and lsmtree.merge
(core/lsmtree/lsmtree.go:137-231) call it.  Checksums are not looked at (the
library checks them in a pass of its own), and a size that Go's make would
panic on ends the segment like any other size that does not fit.

frame_closed is the closed form include/nkv_merkle.h states; tests/
test_frame_ref.py holds the two to each other, the GPU tests hold the device to
frame_closed.
"""
import struct

import numpy as np

HDR = 30
NONE = 2**64 - 1
_FIELDS = (4, 8, 1, 1, 8, 8)  # Crc, Timestamp, Status, TypeInfo, KeySize, ValueSize


class _Reader:
    """bytes.Reader behind binary.Read: read_full(n) is io.ReadFull."""

    def __init__(self, buf):
        self.buf, self.at = buf, 0

    def read_full(self, n):
        """The n bytes, or None for io.EOF (nothing left, n > 0) or
        io.ErrUnexpectedEOF (some, not n).  n = 0 reads nothing and succeeds."""
        got = self.buf[self.at:self.at + n]
        self.at += len(got)
        return got if len(got) == n else None


def _deserialize(reader):
    """One Deserialize: the record's TotalSize, or None for eof."""
    fields = []
    for width in _FIELDS:
        b = reader.read_full(width)
        if b is None:
            return None
        fields.append(int.from_bytes(b, "little"))
    ks, vs = fields[4], fields[5]
    # rec.Key = make([]byte, KeySize); rec.Value = make([]byte, ValueSize); then the two reads
    if reader.read_full(ks) is None:
        return None
    if reader.read_full(vs) is None:
        return None
    return HDR + ks + vs


def segments_of(stream_len, seg_off):
    """[(start, end)] of the segments; seg_off None = the one segment [0, stream_len)."""
    if seg_off is None:
        return [(0, stream_len)]
    off = [int(x) for x in seg_off]
    return [(a, b) for a, b in zip(off, off[1:] + [stream_len])]


def _result(offsets, seg_first, seg_len, segs):
    tails = [j for j, ((a, e), ln) in enumerate(zip(segs, seg_len)) if a + ln != e]
    stats = [len(offsets), sum(seg_len), len(tails), tails[0] if tails else NONE]
    return (np.asarray(offsets, np.uint64), np.asarray(seg_first + [len(offsets)], np.uint64),
            np.asarray(seg_len, np.uint64), stats)


def deserialize_loop(stream, seg_off=None):
    """(offsets, seg_first (one entry per segment and n), seg_len, stats) by
    running Deserialize over each segment's bytes until eof."""
    stream = bytes(stream)
    segs = segments_of(len(stream), seg_off)
    offsets, seg_first, seg_len = [], [], []
    for a, e in segs:
        seg_first.append(len(offsets))
        reader = _Reader(stream[a:e])
        done = 0
        while True:
            size = _deserialize(reader)
            if size is None:
                break
            offsets.append(a + done)
            done += size
        seg_len.append(done)
    return _result(offsets, seg_first, seg_len, segs)


def frame_closed(stream, seg_off=None):
    """The same by the closed form: the record at p is accepted iff 30 <= end -
    p, KeySize <= end - p - 30 and ValueSize <= end - p - 30 - KeySize."""
    stream = bytes(stream)
    segs = segments_of(len(stream), seg_off)
    offsets, seg_first, seg_len = [], [], []
    for a, e in segs:
        seg_first.append(len(offsets))
        p = a
        while e - p >= HDR:
            ks, vs = struct.unpack_from("<QQ", stream, p + 14)
            room = e - p - HDR
            if ks > room or vs > room - ks:
                break
            offsets.append(p)
            p += HDR + ks + vs
        seg_len.append(p - a)
    return _result(offsets, seg_first, seg_len, segs)


def sizes_of(stream, offsets):
    """TotalSize of the record at each offset (the host form's rec_size_out)."""
    stream = bytes(stream)
    out = np.zeros(len(offsets), np.uint64)
    for i, p in enumerate(offsets):
        ks, vs = struct.unpack_from("<QQ", stream, int(p) + 14)
        out[i] = HDR + ks + vs
    return out
