"""The batch forms of the engine's own entry points (engine/coreeng/coreeng.go):
CoreEngine.Put and Get for n requests in arrival order, admission included.

Both run the prologue the reference runs per request (coreeng.go:63-75,
184-199): IsLegal(key), getTokenBucket(user) -> HasEnoughTokens(), and for every
admitted request putTokenBucket before the request's own work.  The bucket
records go into the memtable like any other record (coreeng.go:201-219 skips
only the WAL for them), so they count towards Count, memusage and flush_at, and
the next batch reads them back.

put_many() looks the buckets up once (lsmtree.get_many over the tables and the
memtable), admits the batch on the device (tokenbucket.admit_many), builds the
interleaved batch the engine would have written -- for each allowed request the
bucket record (key start ++ user, Value the 32-byte image), then the user's
record -- and hands it to Memtable.put_many.  get_many() admits likewise, puts
the bucket records of the admitted and looks up the admitted keys.

The admission answers do not depend on where a bucket is stored: the one lookup
in front of the batch sees memtable and tables alike, and every later state of a
bucket within the batch follows from the closed form, not from a read.  The
flush is left to the caller, as Memtable.put_many leaves it: a batch whose
flush_at falls inside it is the caller's to split (flush records [0, flush_at],
clear, put the rest again), and the records behind flush_at were admitted
already.  Delete, the WAL and the LRU are not provided.
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import lsmtree, tokenbucket
from .tokenbucket import ALLOWED


def _admit_and_log(mt, tables, users, keys, now, start, max_tokens, reset_interval):
    """The shared prologue.  Returns (the Admission, the indices of the allowed
    requests, their bucket records' keys and Values, now per request)."""
    users, keys, start = [bytes(u) for u in users], [bytes(k) for k in keys], bytes(start)
    n = len(users)
    if len(keys) != n:
        raise ValueError(f"{n} users and {len(keys)} keys")
    ts = np.full(n, int(now), np.int64) if np.ndim(now) == 0 else np.ascontiguousarray(now, dtype=np.int64)
    if ts.shape != (n,):
        raise ValueError(f"{ts.size} times for {n} requests")
    stored = lsmtree.get_many(tables, [start + u for u in users], memtable=mt) if n else []
    adm = tokenbucket.admit_many(users, keys, ts if n else 0, start, max_tokens, reset_interval, stored=stored,
                                 device=mt.device)
    allowed = np.flatnonzero(adm.verdict == ALLOWED)
    bkeys = [start + users[i] for i in allowed]
    bvals = [adm.bucket[i].tobytes() for i in allowed]
    return adm, allowed, bkeys, bvals, ts


def put_many(mt, tables, users: Sequence[bytes], keys: Sequence[bytes], values: Sequence[bytes], now,
             type_info=None, start: bytes = b"$", max_tokens: int = 100, reset_interval: int = 1):
    """CoreEngine.Put (coreeng.go:184-199) for a batch: mt a memtable.Memtable,
    tables the resident tables below it in search order (may be empty), now one
    int or n non-decreasing ints, type_info None, one int or n.  Returns
    (verdicts, is_new, flush_at): the admission verdict per request, and what
    Memtable.put_many returns for the records written -- two per allowed
    request, the bucket record first."""
    n = len(users)
    adm, allowed, bkeys, bvals, ts = _admit_and_log(mt, tables, users, keys, now, start, max_tokens, reset_interval)
    ty = np.zeros(n, np.uint8) if type_info is None else np.broadcast_to(np.asarray(type_info, np.uint8), (n,))
    k2: List[bytes] = []
    v2: List[bytes] = []
    for j, i in enumerate(allowed):
        k2 += [bkeys[j], bytes(keys[i])]
        v2 += [bvals[j], bytes(values[i])]
    ts2 = np.repeat(ts[allowed], 2)
    ty2 = np.zeros(2 * allowed.size, np.uint8)
    ty2[1::2] = ty[allowed]  # the bucket record is record.New's: TypeInfo 0
    is_new, flush_at = mt.put_many(k2, v2, timestamps=ts2, type_info=ty2)
    return adm.verdict, is_new, flush_at


def get_many(mt, tables, users: Sequence[bytes], keys: Sequence[bytes], now, start: bytes = b"$",
             max_tokens: int = 100, reset_interval: int = 1) -> Tuple[np.ndarray, list, np.ndarray, Optional[int]]:
    """CoreEngine.Get (coreeng.go:63-75) for a batch.  Returns (verdicts, values,
    is_new, flush_at): per request the Value get() finds, None where there is
    none or the request was not admitted; is_new and flush_at are
    Memtable.put_many's for the bucket records of the admitted."""
    n = len(users)
    adm, allowed, bkeys, bvals, ts = _admit_and_log(mt, tables, users, keys, now, start, max_tokens, reset_interval)
    is_new, flush_at = mt.put_many(bkeys, bvals, timestamps=ts[allowed])
    values: list = [None] * n
    if allowed.size:
        found = lsmtree.get_many(tables, [bytes(keys[i]) for i in allowed], memtable=mt)
        for i, v in zip(allowed, found):
            values[i] = v
    return adm.verdict, values, is_new, flush_at
