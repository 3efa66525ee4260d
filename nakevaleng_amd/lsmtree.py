"""Per-run Merkle rebuild of core/lsmtree compaction, sharded over GPUs.

In the reference, compaction merges a level's runs (lsmtree.go:71-128), collects
NewLeaf(head.Rec.Value) for every output record (lsmtree.go:211) and builds the
output table's tree in MakeTableSecondaries (sstable.go:41-46).  Independent
table builds are independent trees, so they shard with no data-path exchange:
one process per GPU builds its tables, then the 20-byte roots are all-gathered
(RCCL over xGMI when the process group is "nccl"; gloo in CPU tests) so every
rank holds every table's root.

The k-way merge itself (lsmtree.go:137-231) runs on the device too: merge() is
its host-memory form, compact() uploads the runs once and chains the checksum
check, the merge, the output table's tree and its filter with no re-upload.

The step in front of compaction runs there as well: sort_log() is the memtable
flush of a write log in arrival order in its host-memory form, and flush_log()
uploads the log once and chains the checksum check, the sort
(nkv_sort_records_dev) and the flushed table's tree, filter, Index and Summary.
flush_puts() starts one step earlier, from the keys and values themselves: it
encodes the write log on the device (nkv_encode_records_dev, record.New /
ToBytes) and goes on as flush_log does, with no host serialization.

recover() starts from WAL segments that are only bytes: one upload, the record
boundaries found on the device (nkv_frame_records_dev), then flush_log's steps.

The read side: upload_table() keeps a Data table (and its filter) resident, and
get_many() answers a batch of keys over resident tables in search order
(nkv_lookup_dev, nkv_lookup_values_dev), the disk part of the engine's get.
With a memtable.Memtable it asks the live memtable first, as get does
(nkv_memtable_find_dev laid over the tables' answers).

Tables whose Data file stays on disk keep only their Index and filter on the
device (sstable.open_index): locate_many() names, per key, the answering table
and the record's Data-file offset (nkv_locate_dev), and get_many_on_disk() lays
those tables under the memtable's and the resident tables' answers and reads
one record per hit from the Data files.
"""
from __future__ import annotations

from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from ._dev import pack_keys, u8, up, up_opt

Table = Tuple[bytes, np.ndarray]  # (Data-table stream, RecSize per record)


def shard(num_tables: int, world: int, rank: int) -> List[int]:
    """Tables owned by `rank`: round-robin, one run per GPU when num_tables == world."""
    return list(range(rank, num_tables, world))


def rank_device(device=None) -> int:
    """The GPU this rank hashes on: `device` when given (an int or torch.device),
    else _lib.current_device() -- the same rule the mirrors' default contexts
    use (LOCAL_RANK modulo the visible devices, else torch's device if torch
    already set one up, else 0)."""
    if device is not None:
        return device.index if hasattr(device, "index") else int(device)
    from . import _lib
    return _lib.current_device()


def _call_build(build, table, dev):
    """build(table, device), or build(table) for a one-argument builder (the
    form compact_roots took before round 2)."""
    import inspect
    try:
        params = [p for p in inspect.signature(build).parameters.values()
                  if p.kind in (p.POSITIONAL_ONLY, p.POSITIONAL_OR_KEYWORD)]
        takes_device = len(params) >= 2 or any(p.kind == p.VAR_POSITIONAL
                                               for p in inspect.signature(build).parameters.values())
    except (TypeError, ValueError):  # builtins without a signature: try the two-argument form
        takes_device = True
    return build(table, dev) if takes_device else build(table)


def gpu_table_root(table: Table, device: Optional[int] = None) -> bytes:
    """Root of one table's Merkle tree, values hashed in place on `device`
    (None: rank_device())."""
    from . import _lib
    stream, rec_sizes = table
    n = len(rec_sizes)
    L = _lib.lib()
    ctx = _lib.default_context(rank_device(device))
    buf = np.frombuffer(bytes(stream) + b"\0", dtype=np.uint8)
    rs = np.ascontiguousarray(rec_sizes, dtype=np.uint64)
    root = np.zeros(20, np.uint8)
    _lib.check(L.nkv_tree_from_records(ctx.h, _lib.p8(buf), buf.size - 1, _lib.p64(rs), n,
                                       _lib.p8(root), None, None), "compaction Merkle step")
    return root.tobytes()


def gather_roots(local: Dict[int, bytes], num_tables: int, device=None) -> List[bytes]:
    """All-gather {table index: 20-byte root} from every rank; returns roots by table index."""
    import torch
    import torch.distributed as dist

    world = dist.get_world_size()
    per = (num_tables + world - 1) // world
    rec = 4 + 20  # table index (int32 LE, -1 = empty slot) + root
    mine = np.zeros((per, rec), np.uint8)
    mine[:, :4] = np.frombuffer(np.int32(-1).tobytes(), np.uint8)
    for slot, (idx, root) in enumerate(sorted(local.items())):
        mine[slot, :4] = np.frombuffer(np.int32(idx).tobytes(), np.uint8)
        mine[slot, 4:] = np.frombuffer(root, np.uint8)
    t = torch.from_numpy(mine.reshape(-1))
    if dist.get_backend() == "nccl":
        t = t.to(device if device is not None else torch.device("cuda", torch.cuda.current_device()))
    out = torch.empty(world * t.numel(), dtype=torch.uint8, device=t.device)
    dist.all_gather_into_tensor(out, t)
    allrec = out.cpu().numpy().reshape(-1, rec)
    roots: List[Optional[bytes]] = [None] * num_tables
    for r in allrec:
        idx = int(np.frombuffer(r[:4].tobytes(), np.int32)[0])
        if idx >= 0:
            roots[idx] = r[4:].tobytes()
    if any(x is None for x in roots):
        raise RuntimeError("gather_roots: a table root is missing")
    return roots  # type: ignore[return-value]


def compact_roots(tables: Sequence[Table], build: Callable[[Table, int], bytes] = None,
                  device=None) -> List[bytes]:
    """Build the Merkle tree of every table this rank owns and all-gather the roots.

    `build(table, device)` (or `build(table)`) maps one table to its root; the
    default hashes on this rank's GPU (rank_device(device): LOCAL_RANK under one
    process per GPU), and the roots are gathered from that same device over RCCL.
    """
    import torch.distributed as dist

    world = dist.get_world_size() if dist.is_initialized() else 1
    rank = dist.get_rank() if dist.is_initialized() else 0
    dev = rank_device(device)
    if build is None:
        build = gpu_table_root
    local = {i: _call_build(build, tables[i], dev) for i in shard(len(tables), world, rank)}
    if world == 1:
        return [local[i] for i in range(len(tables))]
    import torch
    return gather_roots(local, len(tables), torch.device("cuda", dev))


# ---------------------------------------------------------------------------
# the merge itself (nkv_merge_records / nkv_merge_records_dev)

def _check_runs(tables) -> None:
    from . import _lib
    if not 1 <= len(tables) <= _lib.NKV_MERGE_MAX_RUNS:
        raise ValueError(f"merge takes 1..{_lib.NKV_MERGE_MAX_RUNS} runs, got {len(tables)}")


def merge(tables: Sequence[Table], device=None) -> Table:
    """lsmtree.merge (lsmtree.go:137-231) of k sorted runs held in host memory:
    one record per distinct key in ascending key order, the newest Timestamp
    winning (ties as include/nkv_merkle.h states), tombstones kept, every
    record copied byte for byte.  Returns the merged (stream, RecSize array)."""
    import ctypes
    from . import _lib
    _check_runs(tables)
    k = len(tables)
    ctx = _lib.default_context(rank_device(device))
    bufs = [np.frombuffer(bytes(t[0]) + b"\0", dtype=np.uint8) for t in tables]
    sizes = [np.ascontiguousarray(t[1], dtype=np.uint64) for t in tables]
    sizes_p = [s if s.size else np.zeros(1, np.uint64) for s in sizes]
    lens = np.asarray([b.size - 1 for b in bufs], dtype=np.uint64)
    ns = np.asarray([s.size for s in sizes], dtype=np.uint64)
    streams = (ctypes.c_void_p * k)(*[b.ctypes.data for b in bufs])
    rec_size = (ctypes.c_void_p * k)(*[s.ctypes.data for s in sizes_p])
    out = np.zeros(int(lens.sum()) + 1, np.uint8)
    out_sizes = np.zeros(int(ns.sum()) + 1, np.uint64)
    n_out, out_len = ctypes.c_uint64(0), ctypes.c_uint64(0)
    _lib.check(_lib.lib().nkv_merge_records(ctx.h, streams, _lib.p64(lens), rec_size, _lib.p64(ns), k,
                                            out.ctypes.data, out.size - 1, out_sizes.ctypes.data,
                                            ctypes.byref(n_out), ctypes.byref(out_len)), "compaction merge")
    return out[:out_len.value].tobytes(), out_sizes[:n_out.value].copy()


def compact(tables: Sequence[Table], device=None, seed: Optional[int] = None,
            false_positive_rate: float = 0.01, summary_page_size: Optional[int] = None, resident: bool = False):
    """One compaction on the device, the runs uploaded once: every input
    record's Crc checked (nkv_tree_verify_records_dev; a bad one raises
    record.verify's "Bad Record checksum" ValueError before any merge is
    launched), the k-way merge (nkv_merge_records_dev), the merged table's
    Merkle tree and Serialize image (nkv_tree_from_records_dev,
    nkv_bfs_image_dev) and, when `seed` is given, its filter
    (nkv_bloom_insert_records_dev; bloomfilter.New(n, false_positive_rate)).

    Returns {"table": (stream, RecSize array), "root": 20 bytes, "image":
    bytes, "filter": BloomFilter or None, "sources": (run << 32) | index of
    every output record}.  With `summary_page_size` the dict also holds "index"
    and "summary": the merged table's Index and Summary files
    (nkv_index_summary_dev over the merged table where it lies).  With
    `resident` the return is (that dict, a ResidentTable over the merged table
    and its filter where they lie on the device), ready for get_many with no
    re-upload.  A merge of no records raises MerkleTreeError, as New does on
    zero leaves."""
    import ctypes
    import torch
    from . import _lib
    _check_runs(tables)
    k = len(tables)
    dev_index = rank_device(device)
    ctx = _lib.default_context(dev_index)
    L = _lib.lib()
    dev = torch.device("cuda", dev_index)

    stream = torch.cuda.current_stream(dev)
    with ctx.on_stream(stream.cuda_stream):
        runs = (_lib.NkvRun * k)()
        keep = []
        total = n_all = 0
        for r, (data, rec_sizes) in enumerate(tables):
            sizes = np.ascontiguousarray(rec_sizes, dtype=np.uint64)
            n, nbytes = int(sizes.size), len(data)
            if n == 0:
                runs[r] = _lib.NkvRun(None, nbytes, None, 0)
                continue
            d_data, d_off = _checked_upload(ctx, dev, data, sizes, "compaction read", r)
            runs[r] = _lib.NkvRun(d_data.data_ptr(), nbytes, d_off.data_ptr(), n)
            keep += [d_data, d_off]
            total += nbytes
            n_all += n
        d_out, d_out_off, d_out_src = u8(dev, total), u8(dev, 8 * n_all), u8(dev, 8 * n_all)
        n_out, out_len = ctypes.c_uint64(0), ctypes.c_uint64(0)
        _lib.check(L.nkv_merge_records_dev(ctx.h, runs, k, d_out.data_ptr(), total, d_out_off.data_ptr(),
                                           d_out_src.data_ptr(), ctypes.byref(n_out), ctypes.byref(out_len)),
                   "compaction merge")
        return _table_secondaries(ctx, dev_index, stream, d_out, d_out_off, d_out_src, n_out.value, out_len.value,
                                  "compaction", seed, false_positive_rate, summary_page_size, resident)


def _checked_upload(ctx, dev, data, sizes, label, run=None):
    """The read in front of compact's merge and flush_log's sort, on the
    context's stream: one run's bytes and RecSize array to the device, its
    record offsets (nkv_record_offsets_dev) and every record's Crc checked
    (nkv_tree_verify_records_dev).  `label` (and `run`, for compact) name the
    step in the error text.  Returns (stream tensor, offsets tensor)."""
    from . import _lib
    L = _lib.lib()
    n, nbytes = int(sizes.size), len(data)
    d_data = up(dev, np.frombuffer(bytes(data), np.uint8))
    d_size, d_off = up(dev, sizes), u8(dev, 8 * n)
    _lib.check(L.nkv_record_offsets_dev(ctx.h, d_size.data_ptr(), n, d_off.data_ptr()))
    d_nodes, d_crc, d_stats = u8(dev, L.nkv_total_nodes(n) * 20), u8(dev, 4 * n), u8(dev, 24)
    _lib.check(L.nkv_tree_verify_records_dev(ctx.h, d_data.data_ptr(), nbytes, d_off.data_ptr(), n,
                                             d_nodes.data_ptr(), d_crc.data_ptr(), d_stats.data_ptr()), label)
    bad, first, hdr = d_stats.cpu().numpy().view(np.uint64).tolist()
    if hdr:
        raise _lib.NkvError(_lib.NKV_ERR_INVALID, label if run is None else f"{label} of run {run}")
    if bad:
        got = int(d_crc.cpu().numpy().view(np.uint32)[first])
        stored = int(np.frombuffer(bytes(data), "<u4", 1, int(sizes[:first].sum()))[0])
        raise ValueError(f"Bad Record checksum (got {got}, expected {stored})")
    return d_data, d_off


def _table_secondaries(ctx, dev_index, stream, d_out, d_out_off, d_out_src, n, nbytes, what, seed,
                       false_positive_rate, summary_page_size, resident):
    """What compact and flush_log do with the Data table their first step left
    on the device (d_out, d_out_off, d_out_src: n records, nbytes bytes), on
    `stream` with the context already on it: the tree and its Serialize image,
    the filter when `seed` is given, the Index and Summary when
    `summary_page_size` is, then the downloads into the result dict (and the
    ResidentTable when `resident`)."""
    import torch
    from . import _lib, bloomfilter, sstable
    from .merkletree import MerkleTreeError
    L = _lib.lib()
    dev = torch.device("cuda", dev_index)

    if n == 0:
        raise MerkleTreeError("cannot build Merkle Tree from 0 nodes")
    d_nodes, d_img = u8(dev, L.nkv_total_nodes(n) * 20), u8(dev, L.nkv_bfs_size(n))
    d_err = u8(dev, 4)
    _lib.check(L.nkv_tree_from_records_dev(ctx.h, d_out.data_ptr(), nbytes, d_out_off.data_ptr(), n,
                                           d_nodes.data_ptr(), d_err.data_ptr()), f"{what} Merkle step")
    _lib.check(L.nkv_bfs_image_dev(ctx.h, d_nodes.data_ptr(), n, d_img.data_ptr()), "Serialize image")
    bf = d_bits = None
    if seed is not None:
        bf = bloomfilter.New(n, false_positive_rate, seed=seed, ctx=ctx)
        d_bits = u8(dev, ((bf.M + 31) // 32) * 4)
        _lib.check(L.nkv_bloom_insert_records_dev(ctx.h, d_out.data_ptr(), nbytes, d_out_off.data_ptr(), n,
                                                  bf.M, bf.K, bf.HashSeeds[0] if bf.K else 0,
                                                  d_bits.data_ptr()), f"{what} filter")
    d_index = d_summary = None
    if summary_page_size is not None:
        d_index, d_summary = sstable.index_summary_dev(ctx, dev, d_out.data_ptr(), nbytes, d_out_off.data_ptr(),
                                                       n, summary_page_size)
    stream.synchronize()
    if int(d_err.cpu().numpy().view(np.uint32)[0]):
        raise _lib.NkvError(_lib.NKV_ERR_INVALID, f"{what} Merkle step")
    off = d_out_off.cpu().numpy().view(np.uint64)[:n]
    sizes = np.diff(np.append(off, np.uint64(nbytes))).astype(np.uint64)
    nodes = d_nodes.cpu().numpy()
    root_at = (L.nkv_total_nodes(n) - 1) * 20
    if bf is not None:
        bf._contents = bytearray(d_bits.cpu().numpy()[:(bf.M + 7) // 8].tobytes())
    out = {"table": (d_out.cpu().numpy()[:nbytes].tobytes(), sizes),
           "root": nodes[root_at:root_at + 20].tobytes(),
           "image": d_img.cpu().numpy()[:L.nkv_bfs_size(n)].tobytes(),
           "filter": bf,
           "sources": d_out_src.cpu().numpy().view(np.uint64)[:n].copy()}
    if d_index is not None:
        out["index"] = d_index.cpu().numpy().tobytes()
        out["summary"] = d_summary.cpu().numpy().tobytes()
    if resident:
        return out, ResidentTable(dev_index, d_out, nbytes, d_out_off, n, d_bits, bf.M if bf else 0,
                                  bf.K if bf else 0, bf._seed0 if bf else 0)
    return out


# ---------------------------------------------------------------------------
# the memtable flush (nkv_sort_records / nkv_sort_records_dev)

def sort_log(log: Table, device=None) -> Table:
    """Memtable.Flush's Data table (memtable.go:93-116 over skiplist.go:62-120)
    of a write log held in host memory: `log` is (stream, RecSize array) with
    the records in arrival order, any key order.  One record per distinct key
    in ascending key order, the last arrival of each key kept whatever its
    Timestamp or Status, every record copied byte for byte.  Returns the
    flushed (stream, RecSize array)."""
    import ctypes
    from . import _lib
    data, rec_sizes = log
    ctx = _lib.default_context(rank_device(device))
    buf = np.frombuffer(bytes(data) + b"\0", dtype=np.uint8)
    sizes = np.ascontiguousarray(rec_sizes, dtype=np.uint64)
    n = int(sizes.size)
    sizes_p = sizes if n else np.zeros(1, np.uint64)
    out = np.zeros(buf.size, np.uint8)
    out_sizes = np.zeros(n + 1, np.uint64)
    n_out, out_len = ctypes.c_uint64(0), ctypes.c_uint64(0)
    _lib.check(_lib.lib().nkv_sort_records(ctx.h, buf.ctypes.data, buf.size - 1, sizes_p.ctypes.data, n,
                                           out.ctypes.data, out.size - 1, out_sizes.ctypes.data,
                                           ctypes.byref(n_out), ctypes.byref(out_len)), "memtable flush")
    return out[:out_len.value].tobytes(), out_sizes[:n_out.value].copy()


def flush_log(log: Table, device=None, seed: Optional[int] = None, false_positive_rate: float = 0.01,
              summary_page_size: Optional[int] = None, resident: bool = False):
    """Memtable.Flush's MakeTable on the device from one upload of a write log
    (stream, RecSize array) in arrival order: every record's Crc checked
    (nkv_tree_verify_records_dev; a bad one raises record.verify's "Bad Record
    checksum" ValueError before any sort is launched, where WAL replay's
    Deserialize panics), the flush itself (nkv_sort_records_dev), then what
    compact does with its merged table: the tree and Serialize image, the
    filter when `seed` is given, the Index and Summary when
    `summary_page_size` is.

    Returns compact's dict: "table", "root", "image", "filter", "sources" (the
    arrival index of every output record) and, with `summary_page_size`,
    "index" and "summary"; with `resident` (that dict, a ResidentTable over the
    flushed table and its filter where they lie on the device).  An empty log
    raises MerkleTreeError, as New does on zero leaves."""
    import torch
    from . import _lib
    from .merkletree import MerkleTreeError
    data, rec_sizes = log
    sizes = np.ascontiguousarray(rec_sizes, dtype=np.uint64)
    n, nbytes = int(sizes.size), len(data)
    if n == 0:
        if nbytes:
            raise _lib.NkvError(_lib.NKV_ERR_INVALID, "memtable flush: bytes and no records")
        raise MerkleTreeError("cannot build Merkle Tree from 0 nodes")
    dev_index = rank_device(device)
    ctx = _lib.default_context(dev_index)
    dev = torch.device("cuda", dev_index)
    stream = torch.cuda.current_stream(dev)
    with ctx.on_stream(stream.cuda_stream):
        d_data, d_off = _checked_upload(ctx, dev, data, sizes, "flush read")
        return _flush_tail(ctx, dev_index, stream, d_data, nbytes, d_off, n, seed, false_positive_rate,
                           summary_page_size, resident)


def _flush_tail(ctx, dev_index, stream, d_log, nbytes, d_off, n, seed, false_positive_rate, summary_page_size,
                resident):
    """What flush_log and flush_puts do with the write log their first step
    left on the device (d_log of nbytes bytes, d_off its n record offsets), on
    `stream` with the context already on it: the flush itself
    (nkv_sort_records_dev), then _table_secondaries over the flushed table."""
    import ctypes
    import torch
    from . import _lib
    dev = torch.device("cuda", dev_index)
    d_out, d_out_off, d_out_src = u8(dev, nbytes), u8(dev, 8 * n), u8(dev, 8 * n)
    n_out, out_len = ctypes.c_uint64(0), ctypes.c_uint64(0)
    _lib.check(_lib.lib().nkv_sort_records_dev(ctx.h, d_log.data_ptr(), nbytes, d_off.data_ptr(), n,
                                               d_out.data_ptr(), nbytes, d_out_off.data_ptr(), d_out_src.data_ptr(),
                                               ctypes.byref(n_out), ctypes.byref(out_len)), "memtable flush")
    return _table_secondaries(ctx, dev_index, stream, d_out, d_out_off, d_out_src, n_out.value, out_len.value,
                              "flush", seed, false_positive_rate, summary_page_size, resident)


def recover(segments, device=None, **flush_kwargs):
    """WAL replay into the memtable flush from one upload of the segments' bytes:
    what the engine does at start with WAL.ReadAllSegments (wal.go:262-290)
    and Memtable.Add / Flush, with no host pass over the records.  The listed
    segments are concatenated and uploaded once; their records are framed on
    the device (nkv_frame_records_dev: whole records only, a torn tail dropped
    as readEntireSegment's Deserialize loop drops it); every record's Crc is
    checked (nkv_record_crc_dev; a bad one raises record.verify's "Bad Record
    checksum" ValueError, where Deserialize panics); then flush_log's tail: the
    flush (nkv_sort_records_dev) and the flushed table's tree, filter, Index
    and Summary.  `flush_kwargs` are flush_log's seed, false_positive_rate,
    summary_page_size and resident, and so is the return value.

    The flush refuses a log with gaps.  A tail behind the last record costs
    nothing: the framed length is passed instead of the uploaded one.  A tail
    with records behind it (a torn segment in the middle, which the WAL itself
    never writes) is the rare path: the segment lengths come back to the host,
    the gaps are closed there and the log is uploaded a second time.  No
    records at all raise MerkleTreeError, as flush_log does."""
    import ctypes
    import torch
    from . import _lib, wal
    from .merkletree import MerkleTreeError
    data, seg_off = wal.concat_segments(segments)
    S, nbytes = int(seg_off.size), len(data)
    if S == 0 or nbytes == 0:
        raise MerkleTreeError("cannot build Merkle Tree from 0 nodes")
    dev_index = rank_device(device)
    ctx = _lib.default_context(dev_index)
    L = _lib.lib()
    dev = torch.device("cuda", dev_index)

    def u64(t, count):
        return t.cpu().numpy().view(np.uint64)[:count].copy()

    stream = torch.cuda.current_stream(dev)
    with ctx.on_stream(stream.cuda_stream):
        d_data, d_seg = up(dev, np.frombuffer(data, np.uint8)), up(dev, seg_off)
        cap = nbytes // 30
        d_off, d_first, d_len = u8(dev, 8 * cap), u8(dev, 8 * (S + 1)), u8(dev, 8 * S)
        n_out, stats = ctypes.c_uint64(0), (ctypes.c_uint64 * 4)()
        _lib.check(L.nkv_frame_records_dev(ctx.h, d_data.data_ptr(), nbytes, d_seg.data_ptr(), S, 0,
                                           d_off.data_ptr(), cap, d_first.data_ptr(), d_len.data_ptr(),
                                           ctypes.byref(n_out), stats), "WAL replay: frame")
        n, framed, tails, lowest = int(n_out.value), int(stats[1]), int(stats[2]), int(stats[3])
        if n == 0:
            raise MerkleTreeError("cannot build Merkle Tree from 0 nodes")
        log_len = nbytes
        if tails:
            first = u64(d_first, S + 1)
            if tails == 1 and int(first[lowest + 1]) == n:
                log_len = framed  # the one tail lies behind the last record
            else:  # rare: records behind a tail
                seg_len, off = u64(d_len, S), u64(d_off, n)
                ends = np.append(seg_off[1:], np.uint64(nbytes))
                gap = (ends - seg_off) - seg_len  # every segment's tail
                shift = np.cumsum(gap) - gap      # the tails in front of each segment
                off -= np.repeat(shift, np.diff(first).astype(np.int64)).astype(np.uint64)
                data = wal.close_gaps(data, seg_off, seg_len)
                log_len = len(data)
                assert log_len == framed
                d_data = up(dev, np.frombuffer(data, np.uint8))
                d_off = up(dev, off)
        d_crc, d_stats = u8(dev, 4 * n), u8(dev, 24)
        _lib.check(L.nkv_record_crc_dev(ctx.h, d_data.data_ptr(), log_len, d_off.data_ptr(), n, d_crc.data_ptr(),
                                        d_stats.data_ptr()), "WAL replay: checksums")
        bad, bad_first, hdr = d_stats.cpu().numpy().view(np.uint64)[:3].tolist()
        if hdr:
            raise _lib.NkvError(_lib.NKV_ERR_INVALID, "WAL replay: checksums")
        if bad:
            got = int(d_crc.cpu().numpy().view(np.uint32)[bad_first])
            at = int(u64(d_off, n)[bad_first])
            stored = int(np.frombuffer(data, "<u4", 1, at)[0])
            raise ValueError(f"Bad Record checksum (got {got}, expected {stored})")
        return _flush_tail(ctx, dev_index, stream, d_data, log_len, d_off, n,
                           flush_kwargs.pop("seed", None), flush_kwargs.pop("false_positive_rate", 0.01),
                           flush_kwargs.pop("summary_page_size", None), flush_kwargs.pop("resident", False),
                           **flush_kwargs)


def flush_puts(keys, values, timestamps=None, status=None, type_info=None, device=None, seed: Optional[int] = None,
               false_positive_rate: float = 0.01, summary_page_size: Optional[int] = None, resident: bool = False):
    """The reference's whole write path on the device from one upload of a batch
    of puts: record.New / ToBytes for every (key, value) (nkv_encode_records_dev;
    timestamps, status and type_info as record.encode_many takes them), then
    what flush_log does behind its upload: the flush (nkv_sort_records_dev) and
    the flushed table's tree, filter, Index and Summary.  No checksum pass is
    made: the checksums were just computed.

    Returns flush_log's dict (with `resident`: that dict and the ResidentTable)
    plus "log": the encoded (stream, RecSize array) in arrival order, the bytes
    the WAL would append.  Zero puts raise MerkleTreeError, as flush_log does."""
    import ctypes
    import torch
    from . import _lib, record
    from .merkletree import MerkleTreeError
    p = record.pack_puts(keys, values, timestamps, status, type_info)
    n = p["n"]
    if n == 0:
        raise MerkleTreeError("cannot build Merkle Tree from 0 nodes")
    dev_index = rank_device(device)
    ctx = _lib.default_context(dev_index)
    L = _lib.lib()
    dev = torch.device("cuda", dev_index)

    def ptr(t):
        return None if t is None else t.data_ptr()

    stream = torch.cuda.current_stream(dev)
    with ctx.on_stream(stream.cuda_stream):
        d = {k: up_opt(dev, p[k]) for k in ("keys", "koff", "klen", "vals", "voff", "vlen", "ts", "status", "type")}
        puts = _lib.NkvPuts(ptr(d["keys"]), p["keys"].size, ptr(d["koff"]), ptr(d["klen"]), ptr(d["vals"]),
                            p["vals"].size, ptr(d["voff"]), ptr(d["vlen"]), ptr(d["ts"]), p["ts_all"],
                            ptr(d["status"]), ptr(d["type"]), n)
        nbytes = 30 * n + int(p["klen"].sum()) + int(p["vlen"].sum())
        d_log = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        d_off = torch.zeros(8 * n, dtype=torch.uint8, device=dev)
        out_len = ctypes.c_uint64(0)
        _lib.check(L.nkv_encode_records_dev(ctx.h, ctypes.byref(puts), d_log.data_ptr(), nbytes, d_off.data_ptr(),
                                            None, ctypes.byref(out_len)), "record encode")
        assert out_len.value == nbytes
        got = _flush_tail(ctx, dev_index, stream, d_log, nbytes, d_off, n, seed, false_positive_rate,
                          summary_page_size, resident)
        off = d_off.cpu().numpy().view(np.uint64)
        sizes = np.diff(np.append(off, np.uint64(nbytes))).astype(np.uint64)
        (got[0] if resident else got)["log"] = (d_log.cpu().numpy().tobytes(), sizes)
        return got


# ---------------------------------------------------------------------------
# point lookup over resident tables (nkv_lookup_dev / nkv_lookup_values_dev)

class ResidentTable:
    """One Data table kept on a device for get_many: the stream, its record
    offsets and, optionally, its filter words.  The handle keeps the torch
    tensors alive; drop it to free them."""

    def __init__(self, device: int, stream, nbytes: int, rec_off, n: int, bits=None, m: int = 0, k: int = 0,
                 seed0: int = 0):
        self.device, self.stream, self.nbytes, self.rec_off, self.n = device, stream, int(nbytes), rec_off, int(n)
        self.bits, self.m, self.k, self.seed0 = bits, int(m), int(k), int(seed0)

    def as_struct(self):
        from . import _lib
        return _lib.NkvLookupTable(self.stream.data_ptr(), self.nbytes, self.rec_off.data_ptr(), self.n,
                                   self.bits.data_ptr() if self.bits is not None else None, self.m, self.k,
                                   self.seed0)


def upload_table(table: Table, filter=None, device=None) -> ResidentTable:
    """Put one Data table (stream, RecSize array) on the device, with its record
    offsets (nkv_record_offsets_dev) and, when `filter` (a BloomFilter) is
    given, the filter's words with its M, K and first seed.  A table of no
    records raises ValueError: the reference cannot write one."""
    import torch
    from . import _lib
    data, rec_sizes = table
    sizes = np.ascontiguousarray(rec_sizes, dtype=np.uint64)
    n, nbytes = int(sizes.size), len(data)
    if n == 0:
        raise ValueError("upload_table: a table holds at least one record")
    dev_index = rank_device(device)
    ctx = _lib.default_context(dev_index)
    dev = torch.device("cuda", dev_index)

    d_data, d_size = up(dev, np.frombuffer(bytes(data) or b"\0", np.uint8)), up(dev, sizes)
    d_off = torch.zeros(8 * n, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev)
    with ctx.on_stream(stream.cuda_stream):
        _lib.check(_lib.lib().nkv_record_offsets_dev(ctx.h, d_size.data_ptr(), n, d_off.data_ptr()))
        stream.synchronize()
    d_bits, m, k, seed0 = None, 0, 0, 0
    if filter is not None:
        m, k, seed0 = filter.M, filter.K, filter._seed0
        words = np.zeros(((m + 31) // 32) * 4, np.uint8)
        contents = np.frombuffer(filter.Contents, np.uint8)
        words[:contents.size] = contents
        d_bits = up(dev, words)
    return ResidentTable(dev_index, d_data, nbytes, d_off, n, d_bits, m, k, seed0)


def get_many(tables: Sequence[ResidentTable], keys: Sequence[bytes], device=None, stages: bool = False,
             memtable=None, _indexed=(), _data_files=()):
    """The disk part of the engine's get (coreeng.go:99-160) for a batch of
    keys over resident tables listed in search order (levels ascending, runs
    descending): per key the Value bytes of the first table that holds it, or
    None where no table does or that table holds a tombstone.  With `stages`
    the return is (values, the q x T array of NKV_STAGE codes, the q hits
    (table << 32) | record index, NKV_HIT_NONE where absent).

    With `memtable` (a memtable.Memtable) the steps of get run in order
    (coreeng.go:79-160, without the LRU step): the table lookup as above
    (skipped when `tables` is empty), the memtable's answers laid over it
    (nkv_memtable_find_dev: a key the memtable holds is answered by its latest
    write, a tombstone reading as not found), and one nkv_lookup_values_dev
    over the tables plus the resident log, which a hit names as table
    len(tables).  At most 31 tables then.

    _indexed / _data_files are get_many_on_disk's: Index-only tables searched
    behind everything resident, and their Data files."""
    import ctypes
    import torch
    from . import _lib
    T, q = len(tables), len(keys)
    if _indexed:
        if T + (memtable is not None) > _lib.NKV_LOOKUP_MAX_TABLES:
            raise ValueError(f"get_many_on_disk takes at most {_lib.NKV_LOOKUP_MAX_TABLES} resident tables, "
                             f"the memtable included, got {T + (memtable is not None)}")
    elif memtable is None:
        if not 1 <= T <= _lib.NKV_LOOKUP_MAX_TABLES:
            raise ValueError(f"get_many takes 1..{_lib.NKV_LOOKUP_MAX_TABLES} tables, got {T}")
    elif T > _lib.NKV_LOOKUP_MAX_TABLES - 1:
        raise ValueError(f"get_many takes at most {_lib.NKV_LOOKUP_MAX_TABLES - 1} tables beside a memtable, got {T}")
    first = tables[0] if T else (memtable if memtable is not None else _indexed[0])
    dev_index = rank_device(device if device is not None else first.device)
    if any(t.device != dev_index for t in list(tables) + list(_indexed)) or \
            (memtable is not None and memtable.device != dev_index):
        raise ValueError(f"get_many: every table must be resident on device {dev_index}")
    if q == 0:
        return ([], np.zeros((0, T), np.uint8), np.zeros(0, np.uint64)) if stages else []
    ctx = _lib.default_context(dev_index)
    L = _lib.lib()
    dev = torch.device("cuda", dev_index)

    blob, koff, klen = pack_keys(keys)
    d_keys, d_koff, d_klen = up(dev, np.frombuffer(blob, np.uint8)), up(dev, koff), up(dev, klen)
    d_hit, d_status, d_stage, d_err = u8(dev, 8 * q), u8(dev, q), u8(dev, q * T), u8(dev, 4)
    d_out_off = u8(dev, 8 * (q + 1))
    structs = [t.as_struct() for t in tables]
    tabs = (_lib.NkvLookupTable * max(T, 1))(*structs)
    with_mem = memtable is not None and memtable.n > 0  # an empty memtable holds no key
    TV = T + 1 if with_mem else T  # the tables nkv_lookup_values_dev reads: the log is the last
    vtabs = (_lib.NkvLookupTable * TV)(*(structs + [memtable.as_struct()])) if with_mem else tabs
    out_len = ctypes.c_uint64(0)
    stream = torch.cuda.current_stream(dev)
    with ctx.on_stream(stream.cuda_stream):
        if T:
            _lib.check(L.nkv_lookup_dev(ctx.h, tabs, T, d_keys.data_ptr(), d_koff.data_ptr(), d_klen.data_ptr(), q,
                                        d_hit.data_ptr(), d_status.data_ptr(), d_stage.data_ptr(), d_err.data_ptr()),
                       "point lookup")
        else:
            d_hit.fill_(0xFF)  # no table: every key absent until the memtable answers
        if with_mem:
            memtable.find_dev(d_keys, d_koff, d_klen, q, d_hit, d_status, table_id=T, overlay=True)
        if _indexed:  # the disk tables under every resident answer, named TV, TV + 1, ..
            located = _locate_under(ctx, L, dev, _indexed, TV, d_keys, d_koff, d_klen, q, d_hit, d_status)
        if TV == 0:
            if _indexed:
                stream.synchronize()
                return read_located(_data_files, _located_of(located, d_hit, d_status, q, 0), keys)
            return ([None] * q, np.zeros((q, 0), np.uint8), np.full(q, _lib.NKV_HIT_NONE, np.uint64)) if stages \
                else [None] * q
        tabs, T_stage, T = vtabs, T, TV
        _lib.check(L.nkv_lookup_values_dev(ctx.h, tabs, T, d_hit.data_ptr(), d_status.data_ptr(), q, None, 0, None,
                                           ctypes.byref(out_len)), "point lookup, Value sizes")
        if int(d_err.cpu().numpy().view(np.uint32)[0]):
            raise _lib.NkvError(_lib.NKV_ERR_INVALID, "point lookup: a record reaches outside its table")
        d_out = u8(dev, out_len.value)
        _lib.check(L.nkv_lookup_values_dev(ctx.h, tabs, T, d_hit.data_ptr(), d_status.data_ptr(), q,
                                           d_out.data_ptr(), out_len.value, d_out_off.data_ptr(),
                                           ctypes.byref(out_len)), "point lookup, Values")
        stream.synchronize()
    status = d_status.cpu().numpy()[:q]
    off = d_out_off.cpu().numpy().view(np.uint64)[:q + 1].tolist()
    packed = d_out.cpu().numpy()[:out_len.value].tobytes()
    values = [packed[off[i]:off[i + 1]] if status[i] == _lib.NKV_GET_LIVE else None for i in range(q)]
    if _indexed:
        on_disk = read_located(_data_files, _located_of(located, d_hit, d_status, q, T), keys)
        return [v if status[i] != _lib.NKV_GET_LOCATED else on_disk[i] for i, v in enumerate(values)]
    if not stages:
        return values
    return (values, d_stage.cpu().numpy()[:q * T_stage].reshape(q, T_stage).copy(),
            d_hit.cpu().numpy().view(np.uint64)[:q].copy())


# ---------------------------------------------------------------------------
# tables whose Data file stays on disk (nkv_locate_dev over sstable.IndexedTable)

def _locate_under(ctx, L, dev, indexed, base, d_keys, d_koff, d_klen, q, d_hit, d_status):
    """nkv_locate_dev with overlay over the answers in d_hit / d_status, the
    Index-only tables named base, base + 1, ..; in chunks of
    NKV_LOOKUP_MAX_TABLES, each laid under the ones before.  Returns the
    d_data_off tensor."""
    from . import _lib
    d_data_off = u8(dev, 8 * q)
    for t0 in range(0, len(indexed), _lib.NKV_LOOKUP_MAX_TABLES):
        part = indexed[t0:t0 + _lib.NKV_LOOKUP_MAX_TABLES]
        tabs = (_lib.NkvIndexTable * len(part))(*[t.as_struct() for t in part])
        _lib.check(L.nkv_locate_dev(ctx.h, tabs, len(part), base + t0, d_keys.data_ptr(), d_koff.data_ptr(),
                                    d_klen.data_ptr(), q, 1, d_hit.data_ptr(), d_data_off.data_ptr(),
                                    d_status.data_ptr(), None, None), "index lookup")
    return d_data_off


def _located_of(d_data_off, d_hit, d_status, q, base):
    """Per query (Index-only table, Data offset) of a LOCATED answer, else None."""
    from . import _lib
    status = d_status.cpu().numpy()[:q]
    hit = d_hit.cpu().numpy().view(np.uint64)[:q]
    off = d_data_off.cpu().numpy().view(np.int64)[:q]
    return [(int(hit[i] >> np.uint64(32)) - base, int(off[i])) if status[i] == _lib.NKV_GET_LOCATED else None
            for i in range(q)]


def locate_many(tables, keys: Sequence[bytes], stages: bool = False, base: int = 0):
    """FindSummaryTableEntry and FindIndexTableEntry for a batch of keys over
    Index-only tables (sstable.IndexedTable, at most 32) in search order: per
    key (table, Data-file offset) of the first table whose Index holds it with a
    stored Offset other than -1, or None.  `base` is added to the table numbers.
    With `stages` the return is (that list, the q x T array of NKV_STAGE codes,
    the q hits ((base + table) << 32) | entry index, NKV_HIT_NONE where absent)."""
    import torch
    from . import _lib
    T, q = len(tables), len(keys)
    if not 1 <= T <= _lib.NKV_LOOKUP_MAX_TABLES:
        raise ValueError(f"locate_many takes 1..{_lib.NKV_LOOKUP_MAX_TABLES} tables, got {T}")
    dev_index = tables[0].device
    if any(t.device != dev_index for t in tables):
        raise ValueError(f"locate_many: every table must be open on device {dev_index}")
    if q == 0:
        return ([], np.zeros((0, T), np.uint8), np.zeros(0, np.uint64)) if stages else []
    ctx = _lib.default_context(dev_index)
    dev = torch.device("cuda", dev_index)

    blob, koff, klen = pack_keys(keys)
    d_keys, d_koff, d_klen = up(dev, np.frombuffer(blob, np.uint8)), up(dev, koff), up(dev, klen)
    d_hit, d_off, d_status, d_stage, d_err = u8(dev, 8 * q), u8(dev, 8 * q), u8(dev, q), u8(dev, q * T), u8(dev, 4)
    tabs = (_lib.NkvIndexTable * T)(*[t.as_struct() for t in tables])
    stream = torch.cuda.current_stream(dev)
    with ctx.on_stream(stream.cuda_stream):
        _lib.check(_lib.lib().nkv_locate_dev(ctx.h, tabs, T, base, d_keys.data_ptr(), d_koff.data_ptr(),
                                             d_klen.data_ptr(), q, 0, d_hit.data_ptr(), d_off.data_ptr(),
                                             d_status.data_ptr(), d_stage.data_ptr(), d_err.data_ptr()),
                   "index lookup")
        stream.synchronize()
    if int(d_err.cpu().numpy().view(np.uint32)[0]):
        raise _lib.NkvError(_lib.NKV_ERR_INVALID, "index lookup: an entry reaches outside its Index")
    out = _located_of(d_off, d_hit, d_status, q, 0)
    if not stages:
        return out
    return out, d_stage.cpu().numpy()[:q * T].reshape(q, T).copy(), d_hit.cpu().numpy().view(np.uint64)[:q].copy()


def read_located(data_files, located, keys=None, read_hint: int = 8192):
    """The host half of get_many_on_disk.  located[i] is (table, Data offset)
    or None; data_files[table] is that table's Data file (a path or an open
    file descriptor).  Per hit: one os.pread of read_hint bytes at the offset
    (a second one for the rest of a longer record), then record.Deserialize's
    work (record.go:119-172): the 30-byte header, Key and Value, and the stored
    Crc checked -- a mismatch raises ValueError where the reference panics.
    Returns the Value, or None for a miss or a tombstone.  With `keys` a record
    whose Key is not the query's raises ValueError: the Index named another
    record than the Data file holds there."""
    import os
    from . import record
    fds, opened = {}, []
    try:
        out = []
        for i, loc in enumerate(located):
            if loc is None:
                out.append(None)
                continue
            t, off = loc
            if t not in fds:
                f = data_files[t]
                if isinstance(f, int):
                    fds[t] = f
                else:
                    fds[t] = os.open(f, os.O_RDONLY)
                    opened.append(fds[t])
            if off < 0:
                raise ValueError(f"Data offset {off} of table {t} is negative")
            buf = os.pread(fds[t], read_hint, off)
            if len(buf) >= record.HEADER_SIZE:
                _, _, _, _, ks, vs = record._HDR.unpack_from(buf, 0)
                total = record.HEADER_SIZE + ks + vs
                if total > len(buf):
                    buf += os.pread(fds[t], total - len(buf), off + len(buf))
            if len(buf) < record.HEADER_SIZE:
                raise EOFError(f"truncated record at offset {off} of table {t}")
            rec, _ = record.parse(buf, 0)
            if keys is not None and rec.Key != bytes(keys[i]):
                raise ValueError(f"the record at offset {off} of table {t} holds another key")
            out.append(None if rec.IsDeleted() else rec.Value)
        return out
    finally:
        for fd in opened:
            os.close(fd)


def get_many_on_disk(indexed_tables, data_files, keys: Sequence[bytes], resident: Sequence[ResidentTable] = (),
                     memtable=None):
    """The engine's get (coreeng.go:79-160, without the LRU step) for a batch
    of keys over a store whose cold tables keep only their Index and filter on
    the device: the memtable and the `resident` tables answer first, as
    get_many has them; the keys they leave ABSENT are searched in
    `indexed_tables` (sstable.IndexedTable, in search order: every resident
    table is ahead of every Index-only one) by nkv_locate_dev with overlay; and
    each LOCATED key costs one pread of its record from data_files[table]
    (read_located).  Returns per key the Value bytes, or None where no table
    holds the key or the answer is a tombstone."""
    if len(data_files) != len(indexed_tables):
        raise ValueError("get_many_on_disk: one Data file per Index-only table")
    if not indexed_tables:
        return get_many(resident, keys, memtable=memtable)
    if len(keys) == 0:
        return []
    return get_many(resident, keys, memtable=memtable, _indexed=list(indexed_tables), _data_files=list(data_files))


# ---------------------------------------------------------------------------
# sketches over a table's keys (nkv_hll_add_records_dev / nkv_cms_insert_records_dev)

def key_sketches(table, precision: Optional[int] = None, cms=None, seed: Optional[int] = None, device=None):
    """An HLL and / or a Count-Min Sketch over the keys of one Data table:
    (sketch.HLL or None, sketch.CountMinSketch or None).  `table` is a Table
    (stream, RecSize array), uploaded once with upload_table, or a
    ResidentTable, whose resident stream and offsets are used as they are, with
    no upload.  `precision` asks for the HLL -- its EstimateStandard() says how
    many distinct keys a flush of this log will keep, the expected_elements of
    the flushed table's filter -- and `cms` = (epsilon, delta) for the Count-Min
    Sketch (writes per key), seeded with `seed` as sketch.NewCMS takes it."""
    import torch
    from . import _lib, sketch
    if not isinstance(table, ResidentTable):
        table = upload_table(table, device=device)
    dev_index = rank_device(device if device is not None else table.device)
    if table.device != dev_index:
        raise ValueError(f"key_sketches: the table is resident on device {table.device}, not {dev_index}")
    ctx = _lib.default_context(dev_index)
    L = _lib.lib()
    dev = torch.device("cuda", dev_index)
    hll = sketch.New(precision, ctx=ctx) if precision is not None else None
    cm = sketch.NewCMS(cms[0], cms[1], seed=seed, ctx=ctx) if cms is not None else None
    stream = torch.cuda.current_stream(dev)
    d_reg = d_tab = None
    with ctx.on_stream(stream.cuda_stream):
        if hll is not None:
            d_reg = torch.zeros(hll.M, dtype=torch.uint8, device=dev)
            _lib.check(L.nkv_hll_add_records_dev(ctx.h, table.stream.data_ptr(), table.nbytes,
                                                 table.rec_off.data_ptr(), table.n, hll.P, d_reg.data_ptr()),
                       "key sketches: HLL")
        if cm is not None:
            d_tab = torch.zeros(4 * cm.M * cm.K, dtype=torch.uint8, device=dev)
            _lib.check(L.nkv_cms_insert_records_dev(ctx.h, table.stream.data_ptr(), table.nbytes,
                                                    table.rec_off.data_ptr(), table.n, cm.M, cm.K, cm.HashSeeds[0],
                                                    d_tab.data_ptr()), "key sketches: CMS")
        stream.synchronize()
    if hll is not None:
        hll._reg = d_reg.cpu().numpy().copy()
    if cm is not None:
        cm._table = d_tab.cpu().numpy().view(np.uint32).reshape(cm.K, cm.M).copy()
    return hll, cm
