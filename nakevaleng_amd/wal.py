"""The read side of core/wal: records out of write-ahead-log segments that are
only bytes.

  read_segments    WAL.ReadAllSegments / ReadSegmentsInRange / ReadSegmentAt /
                   ReadLastSegment (wal.go:262-290): readEntireSegment
                   (wal.go:293-328) over each listed segment, the records
                   appended in segment order

readEntireSegment runs record.Deserialize until it reports eof, so a segment
whose last record was torn by a crash yields its whole records and drops the
rest.  Here the segments are concatenated, uploaded once and framed on the
device (record.frame, nkv_frame_records): one lane per segment follows its
length prefixes, which is the right shape for segments of five records
(wal_max_recs_in_seg).  Checksums are checked by record.verify, or by
lsmtree.recover, which goes on to the memtable flush.
"""
from __future__ import annotations

from typing import Sequence, Tuple

import numpy as np

Table = Tuple[bytes, np.ndarray]  # (record stream, RecSize per record)


def concat_segments(segments: Sequence[bytes]):
    """(the segments one behind the other, their start offsets)."""
    parts = [bytes(s) for s in segments]
    off = np.zeros(len(parts), np.uint64)
    if len(parts) > 1:
        off[1:] = np.cumsum([len(p) for p in parts[:-1]])
    return b"".join(parts), off


def close_gaps(stream: bytes, seg_off, seg_len) -> bytes:
    """The whole records of every segment one behind the other: the stream
    without the segments' tails."""
    return b"".join(stream[int(a):int(a) + int(n)] for a, n in zip(seg_off, seg_len))


def read_segments(segments: Sequence[bytes], ctx=None) -> Table:
    """The records of the listed WAL segments in order, as a Table: the write
    log (whole records only, torn tails dropped as the reference drops them)
    and each record's TotalSize.  No segments, or only empty ones, give an
    empty log."""
    from . import record
    if len(segments) == 0:
        return b"", np.zeros(0, np.uint64)
    stream, off = concat_segments(segments)
    sizes, _, seg_len, stats = record.frame(stream, segments=off, ctx=ctx)
    if stats[2]:
        stream = close_gaps(stream, off, seg_len)
    return stream, sizes
