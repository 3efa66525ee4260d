"""Plain-Python restatements of the memtable flush (core/memtable over
core/skiplist), the oracle of the device sort (nkv_sort_records_dev).

  flush_literal(records)  models skiplist.Write (skiplist.go:62-120) statement
                          by statement on level 0 and then the level-0 walk of
                          Memtable.NewIterator (memtable.go:103-116): an ordered
                          list of nodes; the search stops at the first node
                          whose key is not below the record's (the loop advances
                          while bytes.Compare(rec.Key, next.Key) == 1); on an
                          equal key that node's Data is replaced, otherwise a
                          node is linked in front of it.  The heights of the
                          nodes only shorten the search, they never change the
                          order, so the model is deterministic.
  flush_closed(records)   the closed form: sort the arrival indices by (key
                          ascending, arrival index ascending) and keep position
                          s iff it is the last or the key at s + 1 differs.

`records` is a list of nakevaleng_amd.record.Record in arrival order.  Both
return (output records, [arrival index, ...]).  Python's bytes ordering is
bytes.Compare's: unsigned lexicographic, a proper prefix first.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

from nakevaleng_amd.record import Record


def flush_literal(records: Sequence[Record]) -> Tuple[List[Record], List[int]]:
    nodes: list = []  # level 0 behind the header: [Data, arrival index]
    for arrival, rec in enumerate(records):
        at = 0  # `node.Next[0]` of the search: the first node whose key is not below rec.Key
        while at < len(nodes) and rec.Key > nodes[at][0].Key:
            at += 1
        if not (at == len(nodes) or rec.Key != nodes[at][0].Key):
            nodes[at][0] = rec  # node.Data = rec: the whole record is replaced
            nodes[at][1] = arrival
            continue
        nodes.insert(at, [rec, arrival])
    return [n[0] for n in nodes], [n[1] for n in nodes]


def flush_closed(records: Sequence[Record]) -> Tuple[List[Record], List[int]]:
    n = len(records)
    order = sorted(range(n), key=lambda i: (records[i].Key, i))
    keep = [order[s] for s in range(n) if s == n - 1 or records[order[s + 1]].Key != records[order[s]].Key]
    return [records[i] for i in keep], keep
