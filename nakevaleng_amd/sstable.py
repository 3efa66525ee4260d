"""The secondary files of the SSTable writer (core/sstable/sstable.go), on the MI355X.

  make_metadata              sstable.makeMetadata           sstable.go:58-74
  make_table_secondaries     Merkle part of MakeTableSecondaries   sstable.go:35-47
  make_metadata_from_records the same, hashing Values in place inside the
                             serialized Data table
  make_filter_contents       the bits of sstable.makeFilter  sstable.go:49-56 (8f row 4)
  make_filter_from_records   the same over the keys of a serialized Data table
  key_sketches_from_records  an HLL and / or a Count-Min Sketch over the same keys
                             (ds/hll, ds/cmsketch; nakevaleng_amd/sketch.py)
  index_and_summary          the bytes of sstable.makeIndexAndSummary  sstable.go:76-139
  make_index_and_summary_from_records   the same into the two files
  make_table_secondaries_from_records   MakeTableSecondaries over a serialized
                             Data table: Index, Summary and Metadata files
                             (and the filter's bits) from one upload
  open_index / open_index_files   the readers' first half: an Index/Summary pair
                             parsed and validated on the device (nkv_index_open_dev),
                             the Index kept resident for lsmtree.locate_many
  open_data_table            the Deserialize loop lsmtree.merge runs over a Data file
                             (lsmtree.go:137-231): the records' sizes from the bytes alone
  table_filename             util/filename.Table             filename.go:58-65, 300-309

What remains outside this path is the Data file itself and the Filter's gob
encoding.
"""
from __future__ import annotations

from typing import Iterable, List, Optional

import numpy as np

from . import _lib
from ._dev import u8, up
from .merkletree import MerkleNode, MerkleTree, MerkleTreeError, New, NewLeaf
from .record import Record

TYPE_METADATA = "metadata"
TYPE_INDEX = "index"      # filename.go: TypeIndex
TYPE_SUMMARY = "summary"  # filename.go: TypeSummary


def table_filename(path: str, dbname: str, level: int, run: int, filetype: str = TYPE_METADATA) -> str:
    if not path.endswith("/"):
        raise ValueError("Table() :: relativePath must end with '/'")
    if level <= 0:
        raise ValueError("Level must be a positive integer!")
    if run < 0:
        raise ValueError("Run must be a non-negative integer!")
    return f"{path}{dbname}-{level}-{run}-{filetype}.db"


def open_data_table(data, device: Optional[int] = None):
    """A Data table that is only bytes (a Data file read back from disk) as the
    Table = (stream, RecSize array) every records entry takes: the record
    boundaries are found on the device (record.frame, strict).  A Data file
    holds whole records and nothing else, so bytes behind the last whole record
    raise ValueError naming the offset at which they start."""
    from . import record
    data = bytes(data)
    sizes, _, _, _ = record.frame(data, strict=True, ctx=_lib.default_context(device))
    return data, sizes


def make_metadata(path: str, dbname: str, level: int, run: int, records: Iterable[Record]) -> MerkleTree:
    """sstable.go:58-74: NewLeaf(rec.Value) per record, New, Serialize."""
    leaves = [NewLeaf(r.Value) for r in records]
    tree = New(leaves)  # raises MerkleTreeError("cannot build Merkle Tree from 0 nodes") like the panic
    tree.Serialize(table_filename(path, dbname, level, run))
    return tree


def make_table_secondaries(path: str, dbname: str, level: int, run: int,
                           merkleleaves: List[MerkleNode]) -> MerkleTree:
    """Merkle part of sstable.go:35-47 (leaves collected by lsmtree.merge, lsmtree.go:211)."""
    tree = New(merkleleaves)
    tree.Serialize(table_filename(path, dbname, level, run))
    return tree


def make_metadata_from_records(path: str, dbname: str, level: int, run: int, stream: bytes,
                               rec_sizes: np.ndarray, device: Optional[int] = None) -> bytes:
    """Same output file as make_metadata, straight from the Data-table bytes and
    KeyContext.RecSize list: values are located and hashed on the device
    (nkv_tree_from_records) on `device` (None: the process's device).  Returns the
    root digest."""
    n = len(rec_sizes)
    if n == 0:
        raise MerkleTreeError("cannot build Merkle Tree from 0 nodes")
    L = _lib.lib()
    ctx = _lib.default_context(device)
    buf = np.frombuffer(bytes(stream) + b"\0", dtype=np.uint8)
    rs = np.ascontiguousarray(rec_sizes, dtype=np.uint64)
    img = np.zeros(L.nkv_bfs_size(n), np.uint8)
    root = np.zeros(20, np.uint8)
    _lib.check(L.nkv_tree_from_records(ctx.h, _lib.p8(buf), buf.size - 1, _lib.p64(rs), n,
                                       _lib.p8(root), None, _lib.p8(img)), "MakeTable")
    fname = table_filename(path, dbname, level, run)
    _lib.check(L.nkv_write_file(fname.encode(), _lib.p8(img), img.size), f"Serialize({fname})")
    return root.tobytes()


def make_filter_contents(keys, seed: int, false_positive_rate: float = 0.01, ctx=None):
    """sstable.makeFilter (sstable.go:49-56) minus the gob file: bloomfilter.New(
    len(keys), 0.01), Insert(key) for every key, on the device.  Returns the
    filter (M, K, HashSeeds, Contents).  The reference's seed is the clock."""
    from . import bloomfilter
    bf = bloomfilter.New(len(keys), false_positive_rate, seed=seed, ctx=ctx)
    bf.InsertMany(keys)
    bf.Contents  # noqa: B018 -- one device batch
    return bf


def make_filter_from_records(stream, rec_sizes, seed: int, false_positive_rate: float = 0.01, ctx=None):
    """makeFilter over the keys of a serialized Data table (KeyContext.Key is the
    record's Key), hashed in place on the device (nkv_bloom_from_records)."""
    import ctypes
    from . import bloomfilter
    sizes = np.ascontiguousarray(rec_sizes, dtype=np.uint64)
    bf = bloomfilter.New(int(sizes.size), false_positive_rate, seed=seed, ctx=ctx)
    buf = np.frombuffer(bytes(stream), np.uint8) if not isinstance(stream, np.ndarray) else stream
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    bits = np.zeros((bf.M + 7) // 8, np.uint8)
    ctx = ctx or _lib.default_context()
    _lib.check(_lib.lib().nkv_bloom_from_records(ctx.h, _lib.p8(buf if buf.size else np.zeros(1, np.uint8)),
                                                 buf.size, _lib.p64(sizes if sizes.size else np.zeros(1, np.uint64)),
                                                 sizes.size, bf.M, bf.K, bf.HashSeeds[0] if bf.K else 0,
                                                 _lib.p8(bits)))
    bf._contents = bytearray(bits.tobytes())
    return bf


def key_sketches_from_records(stream, rec_sizes, precision: Optional[int] = None, cms=None,
                              seed: Optional[int] = None, ctx=None):
    """The sketches of a serialized Data table's keys, hashed in place on the
    device: (HLL or None, CountMinSketch or None).  `precision` asks for an HLL
    (sketch.New(precision) with every key Added: its EstimateStandard() is the
    number of distinct keys, the expected_elements of the table's filter);
    `cms` = (epsilon, delta) asks for a Count-Min Sketch (sketch.NewCMS(epsilon,
    delta, seed) with every key Inserted: writes per key)."""
    from . import sketch
    sizes = np.ascontiguousarray(rec_sizes, dtype=np.uint64)
    buf = np.frombuffer(bytes(stream), np.uint8) if not isinstance(stream, np.ndarray) else stream
    buf = np.ascontiguousarray(buf, dtype=np.uint8)
    p_buf = (buf if buf.size else np.zeros(1, np.uint8)).ctypes.data
    p_sizes = (sizes if sizes.size else np.zeros(1, np.uint64)).ctypes.data
    hll = sketch.New(precision, ctx=ctx) if precision is not None else None
    cm = sketch.NewCMS(cms[0], cms[1], seed=seed, ctx=ctx) if cms is not None else None
    ctx = ctx or _lib.default_context()
    L = _lib.lib()
    if hll is not None:
        _lib.check(L.nkv_hll_add_records(ctx.h, p_buf, buf.size, p_sizes, sizes.size, hll.P, hll._reg.ctypes.data),
                   "key sketches: HLL")
    if cm is not None:
        _lib.check(L.nkv_cms_insert_records(ctx.h, p_buf, buf.size, p_sizes, sizes.size, cm.M, cm.K, cm.HashSeeds[0],
                                            cm._table.ctypes.data), "key sketches: CMS")
    return hll, cm


# ---------------------------------------------------------------------------
# Index and Summary tables (nkv_index_summary_dev / nkv_index_summary_from_records)

def index_and_summary(stream, rec_sizes, summary_page_size: int, device: Optional[int] = None):
    """The bytes sstable.makeIndexAndSummary (sstable.go:76-139) writes for the
    Data table `stream` with KeyContext.RecSize list `rec_sizes`, built on
    `device` (None: the process's device): (Index file bytes, Summary file
    bytes).  A summary_page_size of 0 with two or more records raises, where
    the reference panics on its division."""
    import ctypes
    L = _lib.lib()
    ctx = _lib.default_context(device)
    buf = np.frombuffer(bytes(stream) + b"\0", dtype=np.uint8)
    rs = np.ascontiguousarray(rec_sizes, dtype=np.uint64)
    n, nbytes = int(rs.size), buf.size - 1
    rs_p = rs if n else np.zeros(1, np.uint64)
    # enough for a well-formed table (include/nkv_merkle.h); a table whose
    # KeySize fields reach into later records reports what it needs instead
    icap = max(nbytes - 14 * n, 0)
    scap = 24 + 2 * max(nbytes - 30 * n, 0) + icap  # header: two keys; entries: a subset of the Index's
    ilen, slen = ctypes.c_uint64(0), ctypes.c_uint64(0)
    for _ in range(2):
        index, summary = np.empty(icap + 1, np.uint8), np.empty(scap + 1, np.uint8)
        rc = L.nkv_index_summary_from_records(ctx.h, buf.ctypes.data, nbytes, rs_p.ctypes.data, n,
                                              int(summary_page_size), index.ctypes.data, icap, summary.ctypes.data,
                                              scap, ctypes.byref(ilen), ctypes.byref(slen))
        if rc != _lib.NKV_ERR_INVALID or (ilen.value <= icap and slen.value <= scap):
            break
        icap, scap = ilen.value, slen.value
    _lib.check(rc, "makeIndexAndSummary")
    return index[:ilen.value].tobytes(), summary[:slen.value].tobytes()


def _create(fname: str, data: bytes) -> None:
    """os.Create + write (sstable.go:80-83): unlike Serialize's metadata file,
    these two are truncated."""
    with open(fname, "wb") as f:
        f.write(data)


def make_index_and_summary_from_records(path: str, dbname: str, summary_page_size: int, level: int, run: int,
                                        stream, rec_sizes, device: Optional[int] = None) -> None:
    """makeIndexAndSummary's two files, <dbname>-<level>-<run>-index.db and
    -summary.db, from the Data-table bytes."""
    f_index = table_filename(path, dbname, level, run, TYPE_INDEX)
    f_summary = table_filename(path, dbname, level, run, TYPE_SUMMARY)
    index, summary = index_and_summary(stream, rec_sizes, summary_page_size, device)
    _create(f_index, index)
    _create(f_summary, summary)


def index_summary_dev(ctx, dev, d_stream: int, nbytes: int, d_rec_off: int, n: int, summary_page_size: int):
    """nkv_index_summary_dev over a device-resident Data table (addresses as
    ints): a size query, then the images into two torch tensors of exactly
    those lengths on `dev`.  Returns (index tensor, summary tensor); they are
    complete in the order of the context's stream."""
    import ctypes
    import torch
    L = _lib.lib()
    ilen, slen = ctypes.c_uint64(0), ctypes.c_uint64(0)
    _lib.check(L.nkv_index_summary_dev(ctx.h, d_stream, nbytes, d_rec_off, n, int(summary_page_size), None, 0, None,
                                       0, ctypes.byref(ilen), ctypes.byref(slen)), "makeIndexAndSummary")
    d_index = torch.empty(max(ilen.value, 16), dtype=torch.uint8, device=dev)
    d_summary = torch.empty(max(slen.value, 16), dtype=torch.uint8, device=dev)
    _lib.check(L.nkv_index_summary_dev(ctx.h, d_stream, nbytes, d_rec_off, n, int(summary_page_size),
                                       d_index.data_ptr(), ilen.value, d_summary.data_ptr(), slen.value,
                                       ctypes.byref(ilen), ctypes.byref(slen)), "makeIndexAndSummary")
    return d_index[:ilen.value], d_summary[:slen.value]


def make_table_secondaries_from_records(path: str, dbname: str, summary_page_size: int, level: int, run: int,
                                        stream, rec_sizes, device: Optional[int] = None,
                                        seed: Optional[int] = None, false_positive_rate: float = 0.01):
    """sstable.MakeTableSecondaries (sstable.go:35-47) over a serialized Data
    table, uploaded once: the Index and Summary files (truncated, os.Create),
    the filter's bits when `seed` is given (the gob file is the caller's), and
    the Metadata file (no O_TRUNC, as Serialize).  Returns (root digest, filter
    or None).  As in the reference, a table of no records leaves an empty Index
    and a 24-byte Summary behind before New's error is raised."""
    import torch
    from . import bloomfilter, lsmtree
    L = _lib.lib()
    dev_index = lsmtree.rank_device(device)
    ctx = _lib.default_context(dev_index)
    dev = torch.device("cuda", dev_index)
    f_index = table_filename(path, dbname, level, run, TYPE_INDEX)
    f_summary = table_filename(path, dbname, level, run, TYPE_SUMMARY)
    f_meta = table_filename(path, dbname, level, run)
    sizes = np.ascontiguousarray(rec_sizes, dtype=np.uint64)
    data = np.frombuffer(bytes(stream), np.uint8)
    n, nbytes = int(sizes.size), int(data.size)
    if n == 0:
        index, summary = index_and_summary(stream, sizes, summary_page_size, dev_index)
        _create(f_index, index)
        _create(f_summary, summary)
        raise MerkleTreeError("cannot build Merkle Tree from 0 nodes")

    ts = torch.cuda.current_stream(dev)
    with ctx.on_stream(ts.cuda_stream):
        d_data, d_size = up(dev, data), up(dev, sizes)
        d_off = u8(dev, 8 * n)
        _lib.check(L.nkv_record_offsets_dev(ctx.h, d_size.data_ptr(), n, d_off.data_ptr()))
        d_index, d_summary = index_summary_dev(ctx, dev, d_data.data_ptr(), nbytes, d_off.data_ptr(), n,
                                               summary_page_size)
        bf = d_bits = None
        if seed is not None:
            bf = bloomfilter.New(n, false_positive_rate, seed=seed, ctx=ctx)
            d_bits = u8(dev, ((bf.M + 31) // 32) * 4)
            _lib.check(L.nkv_bloom_insert_records_dev(ctx.h, d_data.data_ptr(), nbytes, d_off.data_ptr(), n, bf.M,
                                                      bf.K, bf.HashSeeds[0] if bf.K else 0, d_bits.data_ptr()),
                       "makeFilter")
        d_nodes, d_img, d_err = u8(dev, L.nkv_total_nodes(n) * 20), u8(dev, L.nkv_bfs_size(n)), u8(dev, 4)
        _lib.check(L.nkv_tree_from_records_dev(ctx.h, d_data.data_ptr(), nbytes, d_off.data_ptr(), n,
                                               d_nodes.data_ptr(), d_err.data_ptr()), "MakeTable")
        _lib.check(L.nkv_bfs_image_dev(ctx.h, d_nodes.data_ptr(), n, d_img.data_ptr()), "Serialize image")
        ts.synchronize()
    if int(d_err.cpu().numpy().view(np.uint32)[0]):
        raise _lib.NkvError(_lib.NKV_ERR_INVALID, "MakeTable")
    _create(f_index, d_index.cpu().numpy().tobytes())
    _create(f_summary, d_summary.cpu().numpy().tobytes())
    if bf is not None:
        bf._contents = bytearray(d_bits.cpu().numpy()[:(bf.M + 7) // 8].tobytes())
    img = np.ascontiguousarray(d_img.cpu().numpy()[:L.nkv_bfs_size(n)])
    _lib.check(L.nkv_write_file(f_meta.encode(), _lib.p8(img), img.size), f"Serialize({f_meta})")
    root_at = (L.nkv_total_nodes(n) - 1) * 20
    return d_nodes.cpu().numpy()[root_at:root_at + 20].tobytes(), bf


# ---------------------------------------------------------------------------
# Index tables opened on the device (nkv_index_open_dev): the key directory of
# lsmtree.locate_many / get_many_on_disk

class IndexedTable:
    """One table whose Index (and, optionally, filter words) stays on a device
    while its Data file stays on disk: the Index bytes, the n entry offsets
    nkv_index_open_dev found, and the filter.  The handle keeps the torch
    tensors alive; drop it to free them."""

    def __init__(self, device: int, index, index_len: int, ent_off, n: int, s: int, bits=None, m: int = 0,
                 k: int = 0, seed0: int = 0):
        self.device, self.index, self.index_len, self.ent_off = device, index, int(index_len), ent_off
        self.n, self.s = int(n), int(s)
        self.bits, self.m, self.k, self.seed0 = bits, int(m), int(k), int(seed0)

    def as_struct(self):
        return _lib.NkvIndexTable(self.index.data_ptr(), self.index_len, self.ent_off.data_ptr(), self.n,
                                  self.bits.data_ptr() if self.bits is not None else None, self.m, self.k,
                                  self.seed0)


def open_index(index_bytes, summary_bytes, filter=None, device: Optional[int] = None) -> IndexedTable:
    """Upload an Index/Summary pair, parse and validate it on the device
    (nkv_index_open_dev) and keep the Index with its entry offsets; the Summary
    is dropped, the search does not need it.  `filter` (a BloomFilter) adds the
    filter's words.  A pair that is not canonical (include/nkv_merkle.h, "index
    lookup") raises ValueError naming the verdict bit: the reference's one-key
    reader remains the way to serve it."""
    import ctypes
    import torch
    from . import lsmtree
    index_bytes, summary_bytes = bytes(index_bytes), bytes(summary_bytes)
    if not index_bytes or not summary_bytes:
        raise ValueError("open_index: an empty Index or Summary holds no chain")
    dev_index = lsmtree.rank_device(device)
    ctx = _lib.default_context(dev_index)
    dev = torch.device("cuda", dev_index)

    d_index, d_summary = up(dev, np.frombuffer(index_bytes, np.uint8)), up(dev, np.frombuffer(summary_bytes, np.uint8))
    cap = len(index_bytes) // 16
    d_ent = torch.empty(8 * max(cap, 1), dtype=torch.uint8, device=dev)
    n, s, verdict = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint32(0)
    stream = torch.cuda.current_stream(dev)
    with ctx.on_stream(stream.cuda_stream):
        _lib.check(_lib.lib().nkv_index_open_dev(ctx.h, d_index.data_ptr(), len(index_bytes), d_summary.data_ptr(),
                                                 len(summary_bytes), d_ent.data_ptr(), cap, ctypes.byref(n),
                                                 ctypes.byref(s), ctypes.byref(verdict)), "index open")
    if verdict.value:
        bit = verdict.value & -verdict.value
        raise ValueError(f"open_index: the pair is not canonical: NKV_INDEX_{_lib.INDEX_VERDICTS[bit]} ({bit})")
    d_ent = d_ent[:8 * n.value].clone()
    d_bits, m, k, seed0 = None, 0, 0, 0
    if filter is not None:
        m, k, seed0 = filter.M, filter.K, filter._seed0
        words = np.zeros(((m + 31) // 32) * 4, np.uint8)
        contents = np.frombuffer(bytes(filter.Contents), np.uint8)
        words[:contents.size] = contents
        d_bits = up(dev, words)
    return IndexedTable(dev_index, d_index, len(index_bytes), d_ent, n.value, s.value, d_bits, m, k, seed0)


def open_index_files(path: str, dbname: str, level: int, run: int, filter=None,
                     device: Optional[int] = None) -> IndexedTable:
    """open_index over <dbname>-<level>-<run>-index.db and -summary.db."""
    with open(table_filename(path, dbname, level, run, TYPE_INDEX), "rb") as f:
        index = f.read()
    with open(table_filename(path, dbname, level, run, TYPE_SUMMARY), "rb") as f:
        summary = f.read()
    return open_index(index, summary, filter, device)
