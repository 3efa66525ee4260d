"""The live memtable on the device (core/memtable/memtable.go:40-90): Add, Find,
Count and ShouldFlush over a write log that stays resident.

Memtable owns the device log, its record offsets, the hash index
(nkv_memtable_add_dev / nkv_memtable_find_dev) and the four state words.
put_many() encodes a batch of puts straight behind the resident log
(nkv_encode_records_dev) and adds it; find_many() is Memtable.Find, tombstones
included; flush() hands the same bytes to the flush (lsmtree._flush_tail:
nkv_sort_records_dev and the flushed table's tree, filter, Index and Summary),
with no upload and no re-encode, and clears.  lsmtree.get_many(...,
memtable=mt) runs the engine's get in order: the memtable first, then the
resident tables.

What Add computes is the reference's, including where it surprises: an
overwrite leaves memusage where it was (include/nkv_merkle.h, "live memtable").
Memtable.Remove and the LRU step of get are not provided.
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib, record
from ._dev import pack_keys, up, up_opt

NONE = 2**64 - 1


class Memtable:
    """strategy, capacity and threshold default to the reference's configuration
    (coreconf.go:33-35: capacity 10, "2 KB" = 2 * 1024 bytes as
    MemtableThresholdBytes parses it, both rules).  The log holds at most
    `max_writes` records and `max_bytes` bytes between two clears."""

    def __init__(self, max_writes: int, max_bytes: int, strategy: int = 3, capacity: int = 10, threshold: int = 2048,
                 device=None):
        import torch
        from .lsmtree import rank_device
        if max_writes < 1 or max_writes > 2**31 - 1 or max_bytes < 30:
            raise ValueError("Memtable: max_writes in 1..2^31 - 1 and max_bytes >= 30")
        self.max_writes, self.max_bytes = int(max_writes), int(max_bytes)
        self.strategy, self.capacity, self.threshold = int(strategy), int(capacity), int(threshold)
        self.device = rank_device(device)
        self.slots = 2
        while self.slots < 2 * self.max_writes:
            self.slots *= 2
        self._ctx = _lib.default_context(self.device)
        self._dev = torch.device("cuda", self.device)
        self.d_log = torch.zeros(self.max_bytes, dtype=torch.uint8, device=self._dev)
        self.d_off = torch.zeros(8 * self.max_writes, dtype=torch.uint8, device=self._dev)
        self.d_index = torch.zeros(_lib.lib().nkv_memtable_index_bytes(self.slots), dtype=torch.uint8,
                                   device=self._dev)
        self.d_state = torch.zeros(8 * _lib.NKV_MEMTABLE_STATE_WORDS, dtype=torch.uint8, device=self._dev)
        self.clear()

    # -- helpers ---------------------------------------------------------

    def _stream(self):
        import torch
        return torch.cuda.current_stream(self._dev)

    def _state(self) -> List[int]:
        return self.d_state.cpu().numpy().view(np.uint64).tolist()

    def as_struct(self):
        """The resident log as a table of nkv_lookup_values_dev (no filter)."""
        return _lib.NkvLookupTable(self.d_log.data_ptr(), self.log_len, self.d_off.data_ptr(), self.n, None, 0, 0, 0)

    def clear(self) -> None:
        """skiplist.Clear + memusage = 0: the log is empty again."""
        stream = self._stream()
        with self._ctx.on_stream(stream.cuda_stream):
            _lib.check(_lib.lib().nkv_memtable_clear_dev(self._ctx.h, self.d_index.data_ptr(), self.slots,
                                                         self.d_state.data_ptr()), "memtable clear")
        self.n, self.log_len = 0, 0
        self._sizes = np.zeros(0, np.uint64)  # TotalSize of every record of the log
        self._host_log = None

    def _fits(self, m: int, nbytes: int) -> None:
        if self.n + m > self.max_writes or self.log_len + nbytes > self.max_bytes:
            raise ValueError(f"Memtable: {m} writes of {nbytes} bytes do not fit behind {self.n} writes of "
                             f"{self.log_len} bytes (max_writes {self.max_writes}, max_bytes {self.max_bytes})")

    def _add(self, m: int, nbytes: int, sizes) -> Tuple[np.ndarray, Optional[int]]:
        """Index the m records just placed behind the log (on the context's stream already)."""
        import torch
        n = self.n + m
        d_is_new = torch.zeros(max(m, 1), dtype=torch.uint8, device=self._dev)
        d_err = torch.zeros(4, dtype=torch.uint8, device=self._dev)
        _lib.check(_lib.lib().nkv_memtable_add_dev(
            self._ctx.h, self.d_log.data_ptr(), self.log_len + nbytes, self.d_off.data_ptr(), self.n, n,
            self.d_index.data_ptr(), self.slots, self.strategy, self.capacity, self.threshold,
            self.d_state.data_ptr(), d_is_new.data_ptr(), d_err.data_ptr()), "memtable add")
        self._stream().synchronize()
        err = int(d_err.cpu().numpy().view(np.uint32)[0])
        if err:
            raise _lib.NkvError(_lib.NKV_ERR_INVALID, f"memtable add refused (verdict {err})")
        self.n, self.log_len = n, self.log_len + nbytes
        self._sizes = np.concatenate([self._sizes, np.asarray(sizes, np.uint64)])
        self._host_log = None
        flush_at = self._state()[3]
        return d_is_new.cpu().numpy()[:m].astype(bool), (None if flush_at == NONE else flush_at)

    # -- the reference's interface -----------------------------------------

    def put_many(self, keys, values, timestamps=None, status=None, type_info=None):
        """Memtable.Add of record.New(key, value) for a batch of puts in order
        (timestamps, status and type_info as record.encode_many takes them).
        Returns (Add's return value per put, flush_at): flush_at is the arrival
        index in the log of the first put of this batch after which
        ShouldFlush() holds, or None.  The engine would flush there
        (coreeng.go:214-218): flush records [0, flush_at], clear, add the rest.
        Raises ValueError when the batch does not fit max_writes / max_bytes."""
        p = record.pack_puts(keys, values, timestamps, status, type_info)
        m = p["n"]
        sizes = 30 + p["klen"] + p["vlen"]
        nbytes = int(sizes.sum())
        self._fits(m, nbytes)
        if m == 0:
            return np.zeros(0, bool), None
        import torch
        L = _lib.lib()

        def ptr(t):
            return None if t is None else t.data_ptr()

        stream = self._stream()
        with self._ctx.on_stream(stream.cuda_stream):
            d = {k: up_opt(self._dev, p[k])
                 for k in ("keys", "koff", "klen", "vals", "voff", "vlen", "ts", "status", "type")}
            puts = _lib.NkvPuts(ptr(d["keys"]), p["keys"].size, ptr(d["koff"]), ptr(d["klen"]), ptr(d["vals"]),
                                p["vals"].size, ptr(d["voff"]), ptr(d["vlen"]), ptr(d["ts"]), p["ts_all"],
                                ptr(d["status"]), ptr(d["type"]), m)
            out_len = ctypes.c_uint64(0)
            # straight behind the resident log; the offsets come back relative to where the batch starts
            _lib.check(L.nkv_encode_records_dev(self._ctx.h, ctypes.byref(puts), self.d_log.data_ptr() + self.log_len,
                                                nbytes, self.d_off.data_ptr() + 8 * self.n, None,
                                                ctypes.byref(out_len)), "record encode")
            assert out_len.value == nbytes
            self.d_off.view(torch.int64)[self.n:self.n + m] += self.log_len
            return self._add(m, nbytes, sizes)

    def add_log(self, table):
        """The same for records already serialized (WAL replay): `table` is
        (stream, RecSize array) in arrival order."""
        import torch
        data, rec_sizes = table
        sizes = np.ascontiguousarray(rec_sizes, dtype=np.uint64)
        m, nbytes = int(sizes.size), len(data)
        if int(sizes.sum()) != nbytes:
            raise ValueError("Memtable.add_log: the record sizes do not add up to the stream")
        self._fits(m, nbytes)
        if m == 0:
            return np.zeros(0, bool), None
        off = np.uint64(self.log_len) + np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)
        stream = self._stream()
        with self._ctx.on_stream(stream.cuda_stream):
            self.d_log[self.log_len:self.log_len + nbytes] = torch.from_numpy(
                np.frombuffer(bytes(data), np.uint8).copy()).to(self._dev)
            self.d_off[8 * self.n:8 * (self.n + m)] = torch.from_numpy(off.view(np.uint8).copy()).to(self._dev)
            return self._add(m, nbytes, sizes)

    def find_dev(self, d_keys, d_koff, d_klen, q: int, d_hit, d_status, table_id: int = 0, overlay: bool = False):
        """nkv_memtable_find_dev over device arrays (torch tensors), on the
        context's current stream; raises if a slot or record is out of bounds."""
        import torch
        d_err = torch.zeros(4, dtype=torch.uint8, device=self._dev)
        _lib.check(_lib.lib().nkv_memtable_find_dev(
            self._ctx.h, self.d_log.data_ptr(), self.log_len, self.d_off.data_ptr(), self.n, self.d_index.data_ptr(),
            self.slots, d_keys.data_ptr(), d_koff.data_ptr(), d_klen.data_ptr(), q, table_id, 1 if overlay else 0,
            d_hit.data_ptr(), d_status.data_ptr(), d_err.data_ptr()), "memtable find")
        if int(d_err.cpu().numpy().view(np.uint32)[0]):
            raise _lib.NkvError(_lib.NKV_ERR_INVALID, "memtable find: a record reaches outside the log")

    def find_many(self, keys: Sequence[bytes]) -> list:
        """Memtable.Find per key: the Record of its latest write (a tombstone
        included), or None."""
        import torch
        q = len(keys)
        if q == 0:
            return []
        blob, koff, klen = pack_keys(keys)
        stream = self._stream()
        with self._ctx.on_stream(stream.cuda_stream):
            d_keys, d_koff, d_klen = (up(self._dev, a) for a in (np.frombuffer(blob, np.uint8), koff, klen))
            d_hit = torch.zeros(8 * q, dtype=torch.uint8, device=self._dev)
            d_status = torch.zeros(q, dtype=torch.uint8, device=self._dev)
            self.find_dev(d_keys, d_koff, d_klen, q, d_hit, d_status)
            stream.synchronize()
        hit = d_hit.cpu().numpy().view(np.uint64)
        if self._host_log is None:
            self._host_log = self.d_log[:self.log_len].cpu().numpy().tobytes()
        off = np.concatenate([[0], np.cumsum(self._sizes)]).astype(np.uint64)
        return [None if h == NONE else record.parse(self._host_log, int(off[int(h) & 0xFFFFFFFF]))[0] for h in hit]

    def count(self) -> Tuple[int, int]:
        """Memtable.Count: (number of elements, memusage)."""
        s = self._state()
        return s[0], s[1]

    def should_flush(self) -> bool:
        """Memtable.ShouldFlush (memtable.go:70-73) as the memtable stands."""
        count, memusage = self.count()
        return bool((self.strategy & _lib.NKV_FLUSH_BY_CAPACITY and count == self.capacity) or
                    (self.strategy & _lib.NKV_FLUSH_BY_THRESHOLD and memusage >= self.threshold))

    def flush(self, seed: Optional[int] = None, false_positive_rate: float = 0.01,
              summary_page_size: Optional[int] = None, resident: bool = False):
        """Memtable.Flush's MakeTable over the resident log where it lies, then
        the clear.  Returns what lsmtree.flush_log returns."""
        from . import lsmtree
        from .merkletree import MerkleTreeError
        if self.n == 0:
            raise MerkleTreeError("cannot build Merkle Tree from 0 nodes")
        stream = self._stream()
        with self._ctx.on_stream(stream.cuda_stream):
            got = lsmtree._flush_tail(self._ctx, self.device, stream, self.d_log, self.log_len, self.d_off, self.n,
                                      seed, false_positive_rate, summary_page_size, resident)
        self.clear()
        return got
