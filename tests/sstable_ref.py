"""Reference for the Index and Summary tables of the SSTable writer, on the CPU.

make_index_and_summary is a statement-by-statement restatement of the
reference's makeIndexAndSummary (core/sstable/sstable.go:76-139) over byte
strings instead of files; find_summary_table_entry and find_index_table_entry
restate its readers (summarytable.go:129-178 with the goodSte lag,
indextable.go:64-92).  The closed forms below are what the device code
computes; tests/test_sstable_ref.py holds them to the restatement.
"""
import io
import struct
from dataclasses import dataclass
from typing import List, Sequence, Tuple


@dataclass
class KeyContext:  # record.go:38-41
    Key: bytes
    RecSize: int


@dataclass
class Entry:  # indexTableEntry / summaryTableEntry: KeySize u64 | Offset i64 | Key
    KeySize: int = 0
    Offset: int = 0
    Key: bytes = b""

    def CalcSize(self) -> int:
        return 8 + 8 + self.KeySize

    def Write(self, w) -> None:
        w.write(struct.pack("<Q", self.KeySize))
        w.write(struct.pack("<q", self.Offset))
        w.write(self.Key)

    def Read(self, r) -> bool:
        """True on EOF (io.EOF / io.ErrUnexpectedEOF in any of the three reads)."""
        b = r.read(8)
        if len(b) < 8:
            return True
        self.KeySize = struct.unpack("<Q", b)[0]
        b = r.read(8)
        if len(b) < 8:
            return True
        self.Offset = struct.unpack("<q", b)[0]
        self.Key = r.read(self.KeySize)
        if self.KeySize and len(self.Key) < self.KeySize:
            return True
        return False


def make_index_and_summary(keyctx: Sequence[KeyContext], summaryPageSize: int) -> Tuple[bytes, bytes]:
    """sstable.go:76-139.  Returns (Index file bytes, Summary file bytes).  Go
    panics on the integer division by zero; so does this (ZeroDivisionError)."""
    wIndex = io.BytesIO()
    wSummary = io.BytesIO()
    offsetIndex = 0
    offsetSummary = 0
    MinKey = b""
    MaxKey = b""
    Payload = 0
    summaryEntries: List[Entry] = []
    for i, kc in enumerate(keyctx):
        if i == 0:
            MinKey = kc.Key
        ite = Entry(KeySize=len(kc.Key), Key=kc.Key, Offset=offsetIndex)
        ite.Write(wIndex)
        offsetIndex += kc.RecSize
        if (i != 0 and i % summaryPageSize == 0) or i == len(keyctx) - 1 or i == 0:
            ste = Entry(KeySize=ite.KeySize, Offset=offsetSummary, Key=ite.Key)
            summaryEntries.append(ste)
            Payload += ste.CalcSize()
        offsetSummary += ite.CalcSize()
        if i == len(keyctx) - 1:
            MaxKey = kc.Key
    wSummary.write(struct.pack("<Q", len(MinKey)))
    wSummary.write(struct.pack("<Q", len(MaxKey)))
    wSummary.write(struct.pack("<Q", Payload))
    wSummary.write(MinKey)
    wSummary.write(MaxKey)
    for ste in summaryEntries:
        ste.Write(wSummary)
    return wIndex.getvalue(), wSummary.getvalue()


def find_summary_table_entry(summary: bytes, key: bytes) -> Entry:
    """summarytable.go:129-178: the entry BEFORE the first one whose key is >=
    `key` (goodSte lags one read behind), Offset -1 outside [MinKey, MaxKey]."""
    r = io.BytesIO(summary)
    MinKeySize, MaxKeySize, Payload = struct.unpack("<QQQ", r.read(24))
    MinKey = r.read(MinKeySize)
    MaxKey = r.read(MaxKeySize)
    if MinKey > key:
        return Entry(Offset=-1)
    if key > MaxKey:
        return Entry(Offset=-1)
    buf = r.read(Payload)
    assert len(buf) == Payload  # io.ReadFull
    r = io.BytesIO(buf)
    ste = Entry()
    while True:
        goodSte = Entry(ste.KeySize, ste.Offset, ste.Key)
        if ste.Read(r):
            ste.Offset = -1
            break
        if key <= ste.Key:
            break
    return goodSte


def find_index_table_entry(index: bytes, key: bytes, startOffset: int) -> Entry:
    """indextable.go:64-92: scan from startOffset; Offset -1 at EOF or at the
    first greater key."""
    r = io.BytesIO(index)
    r.seek(startOffset)
    ite = Entry()
    while True:
        if ite.Read(r):
            ite.Offset = -1
            break
        if key == ite.Key:
            break
        if key < ite.Key:
            ite.Offset = -1
            break
    return ite


def lookup(index: bytes, summary: bytes, key: bytes) -> int:
    """The read path's two steps (engine/coreeng/coreeng.go:118-136): the Data
    offset of `key`, or -1 where either table says it is absent."""
    ste = find_summary_table_entry(summary, key)
    if ste.Offset == -1:
        return -1
    return find_index_table_entry(index, key, ste.Offset).Offset


# ---------------------------------------------------------------------------
# closed forms

def summary_entries(n: int, page: int) -> int:
    """How many records the loop selects."""
    if n <= 1:
        return n
    return 1 + (n - 1) // page + (1 if (n - 1) % page else 0)


def selected(n: int, page: int) -> List[int]:
    """Entry e is record e * page, the last entry the last record."""
    m = summary_entries(n, page)
    return [n - 1 if e == m - 1 else e * page for e in range(m)]


def closed_index_and_summary(keys: Sequence[bytes], rec_sizes: Sequence[int], page: int) -> Tuple[bytes, bytes]:
    n = len(keys)
    off = ioff = 0
    rec_off, idx_off = [], []
    for k, s in zip(keys, rec_sizes):
        rec_off.append(off)
        idx_off.append(ioff)
        off += s
        ioff += 16 + len(k)
    index = b"".join(struct.pack("<Qq", len(k), o) + k for k, o in zip(keys, rec_off))
    if n == 0:
        return index, bytes(24)
    entries = b"".join(struct.pack("<Qq", len(keys[i]), idx_off[i]) + keys[i] for i in selected(n, page))
    header = struct.pack("<QQQ", len(keys[0]), len(keys[-1]), len(entries)) + keys[0] + keys[-1]
    return index, header + entries


def keyctx_of(stream: bytes, rec_sizes: Sequence[int]) -> List[KeyContext]:
    """The KeyContext list of a Data-table stream (record.go:191-199 headers)."""
    out, p = [], 0
    for s in rec_sizes:
        ks = struct.unpack_from("<Q", stream, p + 14)[0]
        out.append(KeyContext(bytes(stream[p + 30:p + 30 + ks]), int(s)))
        p += int(s)
    return out


def from_table(stream: bytes, rec_sizes: Sequence[int], page: int) -> Tuple[bytes, bytes]:
    return make_index_and_summary(keyctx_of(stream, rec_sizes), page)
