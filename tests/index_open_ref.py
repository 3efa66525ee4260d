"""Reference for nkv_index_open_dev / nkv_locate_dev, on the CPU.

open() checks the six conditions of a canonical Index/Summary pair
(include/nkv_merkle.h, "index lookup") in order, by sequential walks with
sstable_ref.Entry.Read, and returns the lowest failing bit.  closed_locate() is
the closed form the device computes over an opened table; tests/
test_index_open_ref.py holds it to the literal restatements of the reference's
two readers (tests/sstable_ref.py, as they are).

canonical() builds a canonical pair over any page partition; hand_made() is one
refused pair per way to fail, each at the smallest shape that trips it.
"""
import bisect
import io
import struct
from typing import Dict, List, Optional, Sequence, Tuple

from tests import sstable_ref
from tests.sstable_ref import Entry

BAD_HEADER, BAD_SUMMARY_CHAIN, BAD_INDEX_CHAIN, BAD_LINK, BAD_ORDER, BAD_RANGE = 1, 2, 4, 8, 16, 32
NOT_SEARCHED, FILTER, SUMMARY, INDEX, FOUND = 0, 1, 2, 3, 4  # NKV_STAGE_*
ABSENT, LOCATED = 0, 3  # NKV_GET_*
HIT_NONE = 2**64 - 1


def chain(buf: bytes) -> Optional[List[Tuple[int, Entry]]]:
    """(position, entry) of a whole chain that ends exactly at len(buf); None
    where a Read reports EOF on the way."""
    r = io.BytesIO(buf)
    out = []
    while r.tell() < len(buf):
        pos, e = r.tell(), Entry()
        try:
            eof = e.Read(r)
        except OverflowError:  # a KeySize no read can ask for: Go's Read ends in EOF
            eof = True
        if eof:
            return None
        out.append((pos, e))
    return out


def open(index: bytes, summary: bytes):  # noqa: A001 (the issue's name)
    """(ent_off, n, s, verdict); a refused pair reports no entries: ([], 0, 0, bit)."""
    def refuse(bit):
        return [], 0, 0, bit

    if len(summary) < 24:
        return refuse(BAD_HEADER)
    mn, mx, payload = struct.unpack_from("<QQQ", summary, 0)
    if 24 + mn + mx + payload > len(summary):
        return refuse(BAD_HEADER)
    MinKey, MaxKey = summary[24:24 + mn], summary[24 + mn:24 + mn + mx]
    ste = chain(summary[24 + mn + mx:24 + mn + mx + payload])
    if not ste:
        return refuse(BAD_SUMMARY_CHAIN)
    ite = chain(index)
    if not ite:
        return refuse(BAD_INDEX_CHAIN)
    at = {pos: j for j, (pos, _) in enumerate(ite)}
    named = []
    for _, e in ste:
        j = at.get(e.Offset)
        if j is None or ite[j][1].KeySize != e.KeySize or ite[j][1].Key != e.Key:
            return refuse(BAD_LINK)
        named.append(j)
    if named[0] != 0 or named[-1] != len(ite) - 1 or any(a >= b for a, b in zip(named, named[1:])):
        return refuse(BAD_LINK)
    keys = [e.Key for _, e in ite]
    if any(a >= b for a, b in zip(keys, keys[1:])):
        return refuse(BAD_ORDER)
    if MinKey != keys[0] or MaxKey != keys[-1]:
        return refuse(BAD_RANGE)
    return [pos for pos, _ in ite], len(ite), len(ste), 0


def entries(index: bytes, ent_off: Sequence[int]) -> Tuple[List[bytes], List[int]]:
    """The keys and stored Offsets of an opened Index."""
    keys, offs = [], []
    for o in ent_off:
        ks, off = struct.unpack_from("<Qq", index, o)
        keys.append(index[o + 16:o + 16 + ks])
        offs.append(off)
    return keys, offs


def closed_locate(keys: Sequence[bytes], offs: Sequence[int], key: bytes) -> Tuple[int, int, int]:
    """(stage, entry index, Data offset) of one key in one opened table."""
    if key < keys[0] or key > keys[-1]:
        return SUMMARY, -1, -1
    j = bisect.bisect_left(keys, key)
    if keys[j] != key or offs[j] == -1:
        return INDEX, -1, -1
    return FOUND, j, offs[j]


def closed_locate_many(tables, queries, passes=None, base=0):
    """tables: [(keys, offs)] in search order; passes[t][i]: table t's filter
    lets query i through (None: all).  Returns (hit, data_off, status, stage rows)."""
    hit, data, status, stages = [], [], [], []
    for i, key in enumerate(queries):
        row, h, d, st = [NOT_SEARCHED] * len(tables), HIT_NONE, -1, ABSENT
        for t, (keys, offs) in enumerate(tables):
            if passes is not None and not passes[t][i]:
                row[t] = FILTER
                continue
            row[t], j, off = closed_locate(keys, offs, key)
            if row[t] == FOUND:
                h, d, st = ((base + t) << 32) | j, off, LOCATED
                break
        hit.append(h)
        data.append(d)
        status.append(st)
        stages.append(row)
    return hit, data, status, stages


# ---------------------------------------------------------------------------
# builders

def ent(key: bytes, off: int) -> bytes:
    return struct.pack("<Qq", len(key), off) + key


def canonical(keys: Sequence[bytes], offs: Sequence[int], named: Sequence[int]) -> Tuple[bytes, bytes]:
    """The pair over `keys` with stored Offsets `offs` whose Summary names the
    Index entries `named` (ascending, 0 first, n - 1 last): canonical when the
    keys are sorted and distinct."""
    assert list(named) == sorted(set(named)) and named[0] == 0 and named[-1] == len(keys) - 1
    pos, p = [], 0
    for k in keys:
        pos.append(p)
        p += 16 + len(k)
    index = b"".join(ent(k, o) for k, o in zip(keys, offs))
    payload = b"".join(ent(keys[j], pos[j]) for j in named)
    return index, summary_of(keys[0], keys[-1], payload)


def summary_of(mn: bytes, mx: bytes, payload: bytes, payload_field: Optional[int] = None) -> bytes:
    return struct.pack("<QQQ", len(mn), len(mx), len(payload) if payload_field is None else payload_field) \
        + mn + mx + payload


def written(keys: Sequence[bytes], rec_sizes: Sequence[int], page: int) -> Tuple[bytes, bytes]:
    """What makeIndexAndSummary writes."""
    return sstable_ref.make_index_and_summary([sstable_ref.KeyContext(k, s) for k, s in zip(keys, rec_sizes)], page)


def hand_made() -> Dict[str, Tuple[bytes, bytes, int]]:
    """name -> (index, summary, the verdict's lowest bit)."""
    k = [b"a", b"b", b"c"]
    index, summary = canonical(k, [0, 40, 80], [0, 1, 2])  # entries of 17 bytes at 0, 17, 34
    one_i, _ = canonical([b"a"], [0], [0])
    hdr = 24 + 1 + 1
    out = {}
    out["header-23-bytes"] = (index, summary[:23], BAD_HEADER)
    long_i, long_s = canonical([b"abcd", b"b"], [0, 1], [0, 1])
    out["header-cut-in-minkey"] = (long_i, long_s[:26], BAD_HEADER)
    out["header-payload-one-short"] = (index, summary[:-1], BAD_HEADER)
    out["payload-ends-mid-entry"] = (index, summary_of(b"a", b"c", summary[hdr:-1]), BAD_SUMMARY_CHAIN)
    out["payload-keysize-past-end"] = (one_i, summary_of(b"a", b"a", struct.pack("<Qq", 2, 0) + b"a"),
                                       BAD_SUMMARY_CHAIN)
    out["no-summary-entry"] = (one_i, summary_of(b"a", b"a", b""), BAD_SUMMARY_CHAIN)
    out["index-ends-mid-entry"] = (index + b"\x01" * 15, summary, BAD_INDEX_CHAIN)
    out["index-last-key-cut"] = (index[:-1], summary, BAD_INDEX_CHAIN)
    out["index-keysize-past-end"] = (index[:34] + struct.pack("<Qq", 2, 80) + b"c", summary, BAD_INDEX_CHAIN)
    out["index-keysize-huge"] = (index[:34] + struct.pack("<Qq", 2**64 - 1, 80) + b"c", summary, BAD_INDEX_CHAIN)
    out["link-one-byte-off"] = (index, summary_of(b"a", b"c", ent(b"a", 0) + ent(b"b", 18) + ent(b"c", 34)), BAD_LINK)
    out["link-other-key"] = (index, summary_of(b"a", b"c", ent(b"a", 0) + ent(b"x", 17) + ent(b"c", 34)), BAD_LINK)
    out["link-other-keysize"] = (index, summary_of(b"a", b"c", ent(b"a", 0) + ent(b"bb", 17) + ent(b"c", 34)),
                                 BAD_LINK)
    out["link-negative"] = (index, summary_of(b"a", b"c", ent(b"a", 0) + ent(b"b", -17) + ent(b"c", 34)), BAD_LINK)
    out["first-not-entry-0"] = (index, summary_of(b"a", b"c", ent(b"b", 17) + ent(b"c", 34)), BAD_LINK)
    out["last-not-entry-n-1"] = (index, summary_of(b"a", b"c", ent(b"a", 0) + ent(b"b", 17)), BAD_LINK)
    out["links-descend"] = (index, summary_of(b"a", b"c", ent(b"a", 0) + ent(b"c", 34) + ent(b"b", 17) + ent(b"c", 34)),
                            BAD_LINK)
    out["links-repeat"] = (index, summary_of(b"a", b"c", ent(b"a", 0) + ent(b"a", 0) + ent(b"c", 34)), BAD_LINK)
    eq = [b"a", b"b", b"b"]
    out["equal-neighbours"] = canonical(eq, [0, 1, 2], [0, 2]) + (BAD_ORDER,)
    deep = [b"samehead-b", b"samehead-a"]
    out["descend-behind-prefix"] = canonical(deep, [0, 1], [0, 1]) + (BAD_ORDER,)
    out["prefix-behind-longer"] = canonical([b"ab", b"a"], [0, 1], [0, 1]) + (BAD_ORDER,)
    out["minkey-one-byte-off"] = (index, summary_of(b"`", b"c", summary[hdr:]), BAD_RANGE)
    out["maxkey-one-byte-off"] = (index, summary_of(b"a", b"d", summary[hdr:]), BAD_RANGE)
    out["maxkey-longer"] = (index, summary_of(b"a", b"c\0", summary[hdr:]), BAD_RANGE)
    # the lowest bit wins: a bad link over an Index whose chain is broken too
    out["broken-index-under-bad-link"] = (index + b"\x01" * 15,
                                          summary_of(b"a", b"c", ent(b"a", 0) + ent(b"b", 18) + ent(b"c", 34)),
                                          BAD_INDEX_CHAIN)
    return out

