"""Reference for the batched point lookup (nkv_lookup_dev /
nkv_lookup_values_dev), on the CPU.

get() is a statement-by-statement restatement of the disk part of the
reference's CoreEngine.get (engine/coreeng/coreeng.go:99-160) over byte strings
instead of files: per table, in the order given, Filter.Query, then
FindSummaryTableEntry, then FindIndexTableEntry (tests/sstable_ref.py's
restatements, as they are), then record.Deserialize at the Data offset; the
first table that holds the key answers, even with a tombstone.  The caller
lists the tables in the engine's order (levels ascending, runs descending).

closed_get() is the closed form the device code computes: with a table's keys
K_0 < ... < K_(n-1), the Summary step refuses exactly the keys outside
[K_0, K_(n-1)] and the Index step exactly the keys no record holds.
tests/test_lookup_ref.py holds the two to each other.
"""
import bisect
import struct
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from tests import sstable_ref

NOT_SEARCHED, FILTER, SUMMARY, INDEX, FOUND = 0, 1, 2, 3, 4  # NKV_STAGE_*
ABSENT, LIVE, TOMBSTONE = 0, 1, 2  # NKV_GET_*
HIT_NONE = 2**64 - 1
_HDR = struct.Struct("<IqBBQQ")  # record.go:191-199


@dataclass
class Filter:  # bloomfilter.go: M, K, HashSeeds t, t+1, .., Contents
    m: int
    k: int
    seed0: int
    contents: bytes  # (m + 7) / 8 bytes

    def words(self) -> np.ndarray:
        """Contents padded with zeros to whole 32-bit words, as the device holds them."""
        w = np.zeros(((self.m + 31) // 32) * 4, np.uint8)
        w[:len(self.contents)] = np.frombuffer(self.contents, np.uint8)
        return w


def _oracle():
    from oracle import oracle_c
    oracle_c.build()
    return oracle_c


def _pack(keys: Sequence[bytes]):
    lens = np.fromiter((len(k) for k in keys), dtype=np.uint64, count=len(keys))
    off = np.zeros(len(keys), np.uint64)
    if len(keys) > 1:
        off[1:] = np.cumsum(lens[:-1])
    return np.frombuffer(b"".join(keys) or b"\0", np.uint8).copy(), off, lens


def filter_of(keys: Sequence[bytes], m: int, k: int, seed0: int) -> Filter:
    """A filter of m bits and k hash functions seeded seed0, seed0 + 1, .. with `keys` inserted."""
    base, off, lens = _pack(keys)
    return Filter(m, k, seed0, _oracle().bloom_insert(base, off, lens, m, k, seed0).tobytes())


def filter_query(f: Optional[Filter], keys: Sequence[bytes]) -> List[bool]:
    """Filter.Query of every key (bloomfilter.go:93-111); no filter: every key passes."""
    if f is None or not keys:
        return [True] * len(keys)
    base, off, lens = _pack(keys)
    return _oracle().bloom_query(base, off, lens, f.m, f.k, f.seed0, np.frombuffer(f.contents, np.uint8)).tolist()


@dataclass
class Table:
    """One SSTable as the read path sees it: the four files' bytes."""
    data: bytes
    index: bytes
    summary: bytes
    filter: Optional[Filter]
    keys: List[bytes] = field(default_factory=list)  # of the records, in order (the closed form's view)
    offsets: List[int] = field(default_factory=list)  # Data offset of each record


def table_of(stream: bytes, rec_sizes, page: int, filter: Optional[Filter] = None) -> Table:
    """The files makeIndexAndSummary writes for a Data table, next to it."""
    index, summary = sstable_ref.from_table(stream, rec_sizes, page)
    kcs = sstable_ref.keyctx_of(stream, rec_sizes)
    offsets, p = [], 0
    for s in rec_sizes:
        offsets.append(p)
        p += int(s)
    return Table(bytes(stream), index, summary, filter, [kc.Key for kc in kcs], offsets)


def parse_record(data: bytes, off: int):
    """record.Deserialize's fields at `off` (the stored Crc is not checked here)."""
    crc, ts, status, typeinfo, ks, vs = _HDR.unpack_from(data, off)
    key = data[off + 30:off + 30 + ks]
    value = data[off + 30 + ks:off + 30 + ks + vs]
    assert len(key) == ks and len(value) == vs
    return status, key, value


@dataclass
class Result:
    table: int  # the table that answered, -1 if none
    offset: int  # the record's Data offset in it, -1 if none
    status: int  # ABSENT / LIVE / TOMBSTONE
    stages: Tuple[int, ...]  # per table
    value: bytes  # the Value of a LIVE hit, else b""

    def hit(self, tables: Sequence[Table]) -> int:
        """(table << 32) | record index, HIT_NONE if none."""
        if self.table < 0:
            return HIT_NONE
        return (self.table << 32) | tables[self.table].offsets.index(self.offset)


def _answer(tables, t, offset, stages) -> Result:
    status, _, value = parse_record(tables[t].data, offset)
    stages = tuple(stages) + (NOT_SEARCHED,) * (len(tables) - len(stages))
    if status & 1:  # rec.IsDeleted(): "not found", and the walk stops
        return Result(t, offset, TOMBSTONE, stages, b"")
    return Result(t, offset, LIVE, stages, value)


def get(tables: Sequence[Table], key: bytes) -> Result:
    """coreeng.go:99-160, the loops flattened into the given order."""
    stages = []
    for t, tab in enumerate(tables):
        q = filter_query(tab.filter, [key])[0]
        if not q:
            stages.append(FILTER)
            continue
        ste = sstable_ref.find_summary_table_entry(tab.summary, key)
        if ste.Offset == -1:
            stages.append(SUMMARY)
            continue
        ite = sstable_ref.find_index_table_entry(tab.index, key, ste.Offset)
        if ite.Offset == -1:
            stages.append(INDEX)
            continue
        stages.append(FOUND)
        return _answer(tables, t, ite.Offset, stages)
    return Result(-1, -1, ABSENT, tuple(stages), b"")


def closed_get(tables: Sequence[Table], key: bytes, passes: Optional[Sequence[bool]] = None) -> Result:
    """The closed form.  passes[t]: Filter.Query of table t, when the caller
    has it already (closed_get_many queries each filter once for all keys)."""
    stages = []
    for t, tab in enumerate(tables):
        if not (passes[t] if passes is not None else filter_query(tab.filter, [key])[0]):
            stages.append(FILTER)
            continue
        if key < tab.keys[0] or key > tab.keys[-1]:
            stages.append(SUMMARY)
            continue
        j = bisect.bisect_left(tab.keys, key)
        if tab.keys[j] != key:
            stages.append(INDEX)
            continue
        stages.append(FOUND)
        return _answer(tables, t, tab.offsets[j], stages)
    return Result(-1, -1, ABSENT, tuple(stages), b"")


def get_many(tables: Sequence[Table], keys: Sequence[bytes]) -> List[Result]:
    return [get(tables, k) for k in keys]


def closed_get_many(tables: Sequence[Table], keys: Sequence[bytes]) -> List[Result]:
    passes = [filter_query(tab.filter, keys) for tab in tables]
    return [closed_get(tables, k, [p[i] for p in passes]) for i, k in enumerate(keys)]
