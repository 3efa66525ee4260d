/*
 * nkv_merkle.h -- C-ABI of libnkvmerkle.so, the MI355X (gfx950) Merkle step of
 * nakevaleng's SSTable build.
 *
 * This is the drop-in boundary for the reference's ds/merkletree package
 * (magley/nakevaleng, Go).  A Go cgo shim keeps the exact Go
 * API -- NewLeaf / New / (*MerkleTree).Serialize / Deserialize / Validate --
 * and calls the entry points below; the C++ header nkv_merkletree.hpp is the
 * same shim for C++ hosts.  Paths in the citations are relative to the
 * reference root.
 *
 *   reference symbol                                   replaced by
 *   ------------------------------------------------   -------------------------------
 *   merkletree.NewLeaf      ds/merkletree/merklenode.go:27-34   nkv_leaf_hash (batched)
 *   merkletree.New / build  ds/merkletree/merkletree.go:18-64   nkv_tree_build, nkv_tree_generic
 *   NewLeaf loop + New      core/sstable/sstable.go:58-71       nkv_tree_from_values
 *   (*MerkleTree).Serialize ds/merkletree/merkletree.go:67-92   image from the calls above +
 *                           ds/merkletree/merklenode.go:37-63   nkv_write_file
 *   MakeTableSecondaries    core/sstable/sstable.go:35-47       nkv_tree_from_values /
 *     (Merkle part) + lsmtree.merge leaf collection               nkv_tree_from_records[_dev]
 *                           core/lsmtree/lsmtree.go:146,211
 *   (*MerkleTree).Validate  ds/merkletree/merkletree.go:162-171 nkv_tree_validate (device rebuild
 *                           ds/merkletree/merklenode.go:99-108    + 20-byte root compare)
 *   compaction over GPUs    core/lsmtree/lsmtree.go:71-128,211  nkv_group_* (one process, one
 *                core/sstable/sstable.go:35-47       context per GPU, RCCL)
 *   record value location   core/record/record.go:191-199       nkv_locate_values_dev
 *   bloomfilter.New sizing  ds/bloomfilter/bloomfilter.go:18-24 nkv_bloom_params
 *   makeFilter / Insert     core/sstable/sstable.go:49-56,      nkv_bloom_build /
 *                           ds/bloomfilter/bloomfilter.go:76-91 nkv_bloom_from_records /
 *                                                               nkv_bloom_insert[_records]_dev
 *   (*BloomFilter).Query    ds/bloomfilter/bloomfilter.go:93-111 nkv_bloom_query_dev
 *   record checksum         core/record/record.go:51 (New),     nkv_record_crc /
 *     crc32.ChecksumIEEE    :163-169 (Deserialize check)        nkv_record_crc_dev /
 *     over Key ++ Value                                         nkv_crc32_dev
 *   makeIndexAndSummary     core/sstable/sstable.go:76-139      nkv_index_summary_dev /
 *                                                               nkv_index_summary_from_records
 *   CoreEngine.get, disk    engine/coreeng/coreeng.go:99-160    nkv_lookup_dev /
 *     path (Filter.Query, FindSummaryTableEntry,                  nkv_lookup_values_dev
 *     FindIndexTableEntry, record.Deserialize per table)
 *   Memtable.Flush over     core/memtable/memtable.go:93-116    nkv_sort_records_dev /
 *     skiplist.Write        core/skiplist/skiplist.go:62-120    nkv_sort_records
 *   Memtable.Add / Find /   core/memtable/memtable.go:40-90     nkv_memtable_add_dev /
 *     Count / ShouldFlush   core/skiplist/skiplist.go:52-120    nkv_memtable_find_dev /
 *     (skiplist.Clear)                                            nkv_memtable_clear_dev
 *   CoreEngine.get, memtable engine/coreeng/coreeng.go:79-86    nkv_memtable_find_dev (overlay)
 *     step                                                        + nkv_lookup_values_dev
 *   record.New / ToBytes    core/record/record.go:49-60,175-187 nkv_encode_records_dev /
 *   wal.flushPartialBufferToSegment  core/wal/wal.go:199-232    nkv_encode_records
 *   (*HLL).Add / Estimate   ds/hll/hll.go:43-62, 75-92          nkv_hll_add[_records][_dev] /
 *                                                               nkv_hll_estimate
 *   cmsketch.New sizing     ds/cmsketch/cmsketch.go:18-24       nkv_cms_params
 *   (*CountMinSketch).Insert / Query  cmsketch.go:76-111        nkv_cms_insert[_records][_dev] /
 *                                                               nkv_cms_query[_dev]
 *   record.Deserialize loop core/record/record.go:119-172,      nkv_frame_records_dev /
 *     over a Data file      core/lsmtree/lsmtree.go:137-231     nkv_frame_records
 *   wal.readEntireSegment   core/wal/wal.go:293-328             nkv_frame_records[_dev] with
 *     (ReadAllSegments, ReadSegmentsInRange, ...)                 segment offsets
 *   CoreEngine.IsLegal,     engine/coreeng/coreeng.go:47-59,    nkv_admit_dev
 *     getTokenBucket,         63-75, 165-199, 223-234
 *     HasEnoughTokens,      ds/tokenbucket/tokenbucket.go:51-83
 *     ToBytes / FromBytes
 *
 * Conventions
 *   - Every function returns an nkv_status (0 = NKV_OK) unless noted; nothing
 *     aborts.  nkv_strerror() gives the message; NKV_ERR_EMPTY's message is
 *     the reference's exact error text (merkletree.go:20).
 *   - Digests are 20 bytes in Go's byte order (sha1.Sum output).
 *   - "nodes" buffers hold every tree level bottom-up, level-major: level L
 *     has nkv_level_count(n, L) digests starting at digest index
 *     nkv_level_start(n, L); level 0 is the leaves, the root is the last
 *     digest (index nkv_total_nodes(n) - 1).  Pads are not stored.
 *   - "img" buffers receive the exact byte image Serialize() writes
 *     (nkv_bfs_size(n) bytes for 20-byte leaves).
 *   - Host-pointer functions are synchronous: outputs are written before
 *     return, and no caller pointer is retained (cgo rule).  Inputs are
 *     staged through library-owned pinned memory: a pool of host threads
 *     gathers chunk k+1 while chunk k is copied to the device.
 *   - *_dev functions take device pointers and are asynchronous on the
 *     context's stream (nkv_ctx_set_stream); nkv_ctx_sync() waits.
 *   - Device outputs: an output buffer needs only the natural alignment of
 *     what it holds, and a call writes exactly the documented extent of each
 *     output, not a byte before or past it (callers pack nodes, images and
 *     offset arrays next to each other in one allocation).
 *       byte strings, at any address: d_img, nkv_bloom_query_dev's d_out, the
 *         buffer of nkv_fill_splitmix64_dev, the merge's and the sort's d_out, d_index and
 *         d_summary of nkv_index_summary_dev, d_status and d_stage of
 *         nkv_lookup_dev and nkv_locate_dev, d_out of nkv_lookup_values_dev, d_out of
 *         nkv_encode_records_dev, d_is_new of nkv_memtable_add_dev, d_status of
 *         nkv_memtable_find_dev, d_verdict and d_last of nkv_admit_dev;
 *       digest arrays (d_nodes, nkv_table.nodes, d_roots and d_out entries of
 *         the group calls), 4-byte aligned: level starts inside a nodes buffer
 *         are multiples of 20 bytes, no more;
 *       uint32_t arrays and filter words (d_crc, the encode's d_crc included,
 *         d_err, d_bits, the sketches' d_reg and d_table, nkv_cms_query_dev's
 *         d_out), 4-byte aligned;
 *       uint64_t arrays (d_rec_off, the frame's included, d_voff, d_vlen, d_stats,
 *         d_out_off, the encode's d_out_off included, d_out_src, d_hit,
 *         d_seg_first, d_seg_len, the memtable's d_state and d_index, d_ent_off,
 *         d_data_off, and d_bucket, d_wait and d_group of nkv_admit_dev), 8-byte
 *         aligned.
 *     nkv_leaf_hash*_dev write level 0 only (20 n bytes); nkv_tree_reduce_dev
 *     leaves level 0 as given; d_bits is ((m + 31) / 32) * 4 bytes; the merge
 *     and the sort write out_len bytes and n_out entries; nkv_index_summary_dev writes
 *     *index_len and *summary_len bytes; nkv_lookup_dev writes q entries of
 *     d_hit and d_status and q T bytes of d_stage; nkv_lookup_values_dev
 *     writes *out_len bytes and q + 1 entries of d_out_off;
 *     nkv_encode_records_dev writes *out_len bytes and n entries of d_out_off
 *     and of d_crc; d_reg is 2^p bytes and d_table 4 K M bytes, both updated
 *     in place and never touched outside those extents; nkv_cms_query_dev
 *     writes n entries of d_out; nkv_frame_records_dev writes *n_out entries
 *     of d_rec_off, S + 1 of d_seg_first and S of d_seg_len;
 *     nkv_memtable_add_dev writes n - n_done bytes of d_is_new, the four words
 *     of d_state and, in place, the 8 slots bytes of d_index;
 *     nkv_memtable_find_dev writes q entries of d_hit and d_status (with
 *     overlay only those of the keys the memtable holds); nkv_index_open_dev
 *     writes *n_out entries of d_ent_off, and none for a refused pair;
 *     nkv_locate_dev writes q entries of d_hit, d_data_off and d_status (with
 *     overlay only those whose status was ABSENT) and q T bytes of d_stage;
 *     nkv_admit_dev writes n bytes of d_verdict and of d_last, 32 n bytes of
 *     d_bucket and n entries of d_wait and d_group, and none of them when its
 *     verdict word is nonzero.
 *     Inputs are never
 *     written: values, record streams, offset and length arrays, segment offsets, the merge's
 *     runs, the sort's log, the lookup's tables, filters and query keys, the
 *     Index and Summary images of nkv_index_open_dev and nkv_locate_dev, and the
 *     sketches' keys and the queried d_table are read in place
 *     (at any alignment where they are bytes).
 *   - Offsets, strides and stream lengths are full 64-bit quantities: the
 *     values, spans or records of one call may lie any distance apart inside
 *     mapped device memory.
 *   - Thread safety: distinct contexts may be used concurrently; one context
 *     must not be used by two threads at once.  Every call re-binds the
 *     context's device (cgo calls may land on any OS thread).
 */
#ifndef NKV_MERKLE_H
#define NKV_MERKLE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NKV_DIGEST_SIZE 20
#define NKV_MERKLE_NODE_EMPTY 1 /* merklenode.go:11 */

typedef enum nkv_status {
    NKV_OK = 0,
    NKV_ERR_EMPTY = 1,   /* "cannot build Merkle Tree from 0 nodes" (merkletree.go:20) */
    NKV_ERR_INVALID = 2, /* bad argument (null pointer, size overflow, bad record,
                            more than 2^31 - 1 values in one batch) */
    NKV_ERR_DEVICE = 3,  /* HIP runtime / kernel launch failure, or no such device */
    NKV_ERR_NOMEM = 4,   /* device, pinned-host or host allocation failed */
    NKV_ERR_IO = 5       /* file open/write failed (nkv_write_file) */
} nkv_status;

typedef struct nkv_ctx nkv_ctx;

/* ---- ABI version ----
 * NKV_ABI_VERSION is the version this header describes; nkv_abi_version()
 * the one the loaded library implements.  A caller built against version V
 * checks nkv_abi_version() == V at start (the Go shim does).
 * The version goes up whenever an existing entry point changes its meaning or
 * signature; adding entry points or option values does not change it.
 *   1: nkv_group_tree_dev takes d_roots as an array of g device pointers
 *      (void *const *; before: one device pointer), and the options
 *      NKV_OPT_DEEP_PREFETCH / NKV_OPT_QUEUE_RING accept only their one
 *      remaining value (and, since round 6, NKV_OPT_QUEUE_PAIR only 0: the
 *      opt-in pair kernel it selected never passed a GPU run). */
#define NKV_ABI_VERSION 1
int nkv_abi_version(void);

/* ---- errors, devices, contexts ---- */
const char *nkv_strerror(int status);
/* "nkv-src-sha256:<64 hex>": SHA-256 of the sources and build flags this
 * library was compiled from (nakevaleng_amd/build.py checks it before use). */
const char *nkv_build_id(void);
int nkv_device_count(int *count);
int nkv_ctx_create(int device, nkv_ctx **out);
void nkv_ctx_destroy(nkv_ctx *ctx);
/* Work is issued on the context's own (non-blocking) stream until
 * nkv_ctx_set_stream() selects a hipStream_t of the context's device; NULL
 * selects the device's null stream.  nkv_ctx_use_own_stream() switches back. */
int nkv_ctx_set_stream(nkv_ctx *ctx, void *hip_stream);
int nkv_ctx_use_own_stream(nkv_ctx *ctx);
int nkv_ctx_sync(nkv_ctx *ctx);
/* Tuning knobs (defaults are the measured-best settings). */
#define NKV_OPT_LEAF_LOAD 1 /* leaf-kernel load path: 4 (default) = 16-byte aligned values in
                               128-byte runs straight into registers, others as 11; 11 =
                               every value through the staged paths: the segment stage
                               when a wave's values share their offset mod 64, the
                               80-byte window stage when their full-block counts are
                               equal, else the value-relative LDS-DMA stream.  (The
                               load paths that lost their A/Bs in rounds 1-2 are gone.) */
#define NKV_OPT_BUCKET 2    /* ragged values (nkv_tree_from_values*, nkv_tree_from_records*):
                               1 = hash in length-sorted order (work queue); 0 = in input
                               order; 2 (default) = auto: input order when the full-block
                               counts of a batch of >= 4096 values lie within max(1, min/16)
                               of each other, else sorted (decided on the device, no
                               read-back) */
#define NKV_OPT_DEEP_PREFETCH 3 /* retired (ABI version 1): 3 is the only value accepted */
#define NKV_OPT_QUEUE_RING 9    /* retired (ABI version 1): 13 is the only value accepted */
#define NKV_OPT_QUEUE_SPLIT 4 /* work-queue kernel: groups whose longest value has at most
                                 this many 64-B blocks may go to the non-priority waves
                                 when the longest value bounds the batch (default 32) */
#define NKV_OPT_QUEUE_WAVES 5 /* work-queue kernel: waves per SIMD, 1..3 (default 3: its
                                 3-slot, 12 KiB LDS ring per wave) */
#define NKV_OPT_CRC_LOAD 6    /* record checksums: 0 (default) = one lane per span, slicing-by-4
                                 from lane-private LDS table columns (no bank conflicts),
                                 whole 128-byte lines into registers; 8 = 16 lanes per span,
                                 chunk states combined by CRC advance tables (a few long
                                 spans) */
#define NKV_OPT_HOST_THREADS 7 /* host-buffer API: threads that gather caller bytes into the
                                  pinned staging chunks (0 = default: min(16, cores), or
                                  the NKV_HOST_THREADS environment variable) */
#define NKV_OPT_STAGE_CHUNK 8  /* host-buffer API: bytes per pinned staging chunk (multiple of
                                  4096, default 32 MiB; three chunks are in flight) */
#define NKV_OPT_BLOOM_PATH 10  /* filter inserts: 2 (default) = group the bit updates by 32768-bit
                                  range from one hash pass (each tile counting-sorted in LDS and
                                  staged), then set them in LDS, one workgroup per range; 1 = the
                                  same grouping by a global counting sort (hashes twice); 0 = one
                                  device atomicOr per bit */
#define NKV_OPT_RECORDS_FUSED 11 /* records form (nkv_tree_from_records*): 1 (default) = one
                                    launch locates each value from its header and hashes it
                                    (k_leaf_records); 0 = a separate locate pass first */
#define NKV_OPT_TABLE_LANES 12 /* nkv_trees_dev: streams the tables of one call are spread
                                  over (1..8, default 2), so one table's leaf kernel runs
                                  while the previous one finishes and reduces */
#define NKV_OPT_TIMING_EVERY 13 /* NKV_TIMING_EVENTS on every k-th tree call only (1..10^6,
                                   default 1; counted from nkv_ctx_set_timing): each event
                                   record is a packet on the stream between two kernels,
                                   so a timed loop samples its kernel times instead of
                                   carrying three records per call */
#define NKV_OPT_SMALL_PATH 14 /* host-buffer tree calls (nkv_tree_from_values, nkv_tree_from_records)
                                 of at most NKV_OPT_SMALL_MAX_N values and NKV_OPT_SMALL_MAX_BYTES
                                 of payload: the whole tree and its image in ONE launch, one
                                 synchronize.  1 (default) = the kernel reads the packed values
                                 and writes its results across PCIe (host-coherent pinned
                                 buffers, no DMA); 2 = one copy to HBM, the launch, one copy
                                 back; 3 = the resident service: one workgroup stays on the GPU
                                 and serves each call of at most 256 values from a mailbox
                                 (NKV_OPT_SERVICE_MAILBOX) as path 1 does, without a launch or the runtime's
                                 completion (larger calls take path 1; the service leaves
                                 20 ms after its last request, or at nkv_ctx_destroy, and the
                                 next call starts it again; while it runs, a device-wide
                                 synchronize waits for it to leave); 0 = off (the grid path
                                 for every size) */
#define NKV_OPT_SMALL_MAX_N 15     /* 0..1024 (default 1024) */
#define NKV_OPT_SMALL_MAX_BYTES 16 /* payload bound of the small path (default 1 MiB; the values
                                      16-byte aligned; for records the whole stream) */
#define NKV_OPT_ARENA_COHERENT 17   /* nkv_host_alloc blocks: 1 (default) = host-coherent pinned memory
                                       (copies read it as any pinned block, and the small path's kernel
                                       reads NewLeaf values in place); 0 = default pinned memory */
#define NKV_OPT_SIDE_GATE 18 /* device-length batches on the gated plan (NKV_OPT_BUCKET 2): 1 (default) =
                                the input-order leaf kernel runs on a second stream of the context,
                                beside the length sort and the work queue (whichever of the two the
                                device-side range opens does the work; the other exits), joined
                                before the levels; 0 = all of them in turn on the context's stream */
#define NKV_OPT_QUEUE_PAIR 19 /* retired (ABI version 1): 0 is the only value accepted (one wave per
                                 work-queue group; the two-wave pair kernel of round 5 was removed
                                 after failing its first GPU parity run) */
#define NKV_OPT_SERVICE_MAILBOX 20 /* where small-tree calls put their input: 0 (default) = in
                                      fine-grained device memory the host stores to directly,
                                      when the GPU has a large BAR and the packed input fits
                                      16 KiB (the kernel stages local memory instead of reading
                                      across PCIe; for the resident service, NKV_OPT_SMALL_PATH 3,
                                      its doorbell and request line too, so it polls local
                                      memory; else as 1); 1 = in host-coherent memory.  Answers
                                      always land in host memory.  A change stops a running
                                      service; the next call starts it in the new form */
#define NKV_OPT_SKETCH_PATH 21 /* HLL adds and CMS inserts: 0 (default) = auto (by n and the table
                                  size); 1 = one lane per key straight onto
                                  the caller's buffer (a compare-and-swap on the register's dword
                                  only when the value rises, one atomicAdd per counter); 2 = a
                                  persistent grid whose workgroups keep private copies in LDS and
                                  merge them once at the end (a CMS table of more than 16384
                                  counters does not fit and takes 1).  Every value gives the same
                                  bytes */
#define NKV_OPT_FRAME_PATH 22 /* nkv_frame_records[_dev]: 0 (default) = auto: the walk when the mean
                                 segment (stream_len / segments) is shorter than 96 KiB, else
                                 speculative; 1 = walk: one lane per segment follows its chain of
                                 length prefixes; 2 = speculative: every byte position is tested as
                                 a record start, the survivors' successor links are doubled from
                                 the segment starts.  A speculative call
                                 whose candidates do not fit NKV_OPT_FRAME_BUDGET (or number more
                                 than 2^31 - 1, or none) takes the walk.  Every value gives the
                                 same bytes */
#define NKV_OPT_FRAME_BUDGET 23 /* bytes of device scratch a speculative frame call may use: 24 bytes
                                   per 64 stream bytes for the marks plus about 17 per candidate
                                   start; 0 (default) = auto: min(2 * stream_len, a quarter of the
                                   free device memory) */
#define NKV_OPT_INDEX_OPEN_PATH 24 /* nkv_index_open_dev, the Summary chain: 0 (default) = auto: the
                                      one-lane walk for a payload below 16 KiB, else chunked; 1 = one
                                      lane follows the payload; 2 = chunked: one lane per
                                      NKV_OPT_INDEX_OPEN_CHUNK payload bytes starts at the first
                                      position of its chunk that passes the link test, the host
                                      stitches the lanes, and any mismatch takes the walk.  Every
                                      value gives the same bytes */
#define NKV_OPT_INDEX_OPEN_CHUNK 25 /* payload bytes per lane of the chunked Summary walk: a multiple
                                       of 16 in 16..2^24; 0 (default) = 4096 */
int nkv_ctx_set_option(nkv_ctx *ctx, int key, int64_t value);
/* Which path the latest host-buffer tree call, or the latest frame call, of the context took */
#define NKV_PATH_GRID 0  /* copies + leaf kernel + per-level reduce launches */
#define NKV_PATH_SMALL 1 /* the one-launch small tree (NKV_OPT_SMALL_PATH) */
#define NKV_PATH_FRAME_WALK 2        /* nkv_frame_records[_dev]: one lane per segment */
#define NKV_PATH_FRAME_SPECULATIVE 3 /* nkv_frame_records[_dev]: mark, successor, doubling */
int nkv_ctx_last_path(nkv_ctx *ctx, int *path);
/* The resident small-tree service of the context (NKV_OPT_SMALL_PATH 3), for
 * diagnostics: out[0] doorbell (latest request), out[1] served (the latest the
 * service took), out[2] done (the latest it answered), out[3] launches so far,
 * out[4] 1 while a launch may still run, out[5] 1 if its stream still has work,
 * out[6] 1 if its requests go through device memory (NKV_OPT_SERVICE_MAILBOX),
 * out[7] where its latest launch landed: XCC_ID << 32 | HW_ID (the hardware's
 * wave/SIMD/CU/SE word).  All zero before the first request. */
int nkv_ctx_small_service_state(nkv_ctx *ctx, uint64_t out[8]);
/* Diagnostics of the same service: enable = 1 makes it stamp the phases of
 * each following request; out (nullable) receives the latest traced request's
 * stamps, seven (s_memrealtime at 100 MHz, s_memtime in shader clocks) pairs:
 * doorbell seen, input staged, leaves hashed, levels + image written,
 * completion stored, then levels done and first image segment built. */
int nkv_ctx_small_service_trace(nkv_ctx *ctx, int enable, uint64_t out[14]);
/* Timing (nkv_ctx_set_timing flags).  NKV_TIMING_EVENTS: the tree calls record
 * HIP events around the leaf kernel and the tree reduce on the context's
 * stream (and, for nkv_tree_from_values, around the upload and the download).
 * NKV_TIMING_CLOCK: every wave of the leaf kernels on the context's device
 * adds its lifetime in shader-clock cycles and in 100 MHz ticks to a
 * counter the context owns (nkv_ctx_clock); one context per device at a
 * time.  0 switches both off. */
#define NKV_TIMING_EVENTS 1
#define NKV_TIMING_CLOCK 2
int nkv_ctx_set_timing(nkv_ctx *ctx, int flags);
/* the latest tree call that recorded events (every call, or every k-th under
 * NKV_OPT_TIMING_EVERY) */
int nkv_ctx_last_timing(nkv_ctx *ctx, float *leaf_ms, float *reduce_ms);
/* the latest nkv_tree_from_values under NKV_TIMING_EVENTS: upload (host values ->
 * HBM), kernels (leaf + tree), download (outputs -> host); NKV_ERR_INVALID when
 * that call was not sampled (NKV_OPT_TIMING_EVERY) */
int nkv_ctx_last_host_timing(nkv_ctx *ctx, float *upload_ms, float *kernels_ms, float *download_ms);
/* NKV_TIMING_CLOCK: the lifetime-weighted mean shader clock of the leaf-kernel
 * waves since the flag was set, and how many waves reported (synchronizes). */
int nkv_ctx_clock(nkv_ctx *ctx, double *mhz, uint64_t *waves);
/* Sum over every tree call since timing was (re-)enabled: synchronizes on the
 * last call's events only, so a timed loop is not perturbed. */
int nkv_ctx_timing_summary(nkv_ctx *ctx, int *calls, float *leaf_ms_total, float *reduce_ms_total);

/* ---- tree shape (pure, no device) ---- */
int nkv_num_levels(uint64_t n); /* incl. the leaf level; 0 for n == 0 */
uint64_t nkv_level_count(uint64_t n, int level);
uint64_t nkv_level_start(uint64_t n, int level);
uint64_t nkv_total_nodes(uint64_t n);
uint64_t nkv_bfs_size(uint64_t n); /* Serialize() bytes for 20-byte leaves */

/* ---- pinned host arena (for the deferred-NewLeaf shim) ----
 * A block from nkv_host_alloc belongs to the context.  Host-buffer calls on the
 * same context whose values all lie inside one block copy them to the device
 * in one DMA straight from the block (no staging gather), values keeping their
 * places (16-byte aligned places take the aligned kernel path).
 * nkv_host_stream(block, upto): bytes [0, upto) of the block are final for the
 * current batch; their copy to the device starts now, asynchronously, so it
 * overlaps the caller's NewLeaf loop; the next call over the block moves only
 * the rest.  Those bytes must not change until that call returns.  A call over
 * the block ends the batch; an upto below the previous one starts a new batch.
 * nkv_host_free waits for copies from the block.  For a block of at least
 * 64 MiB nkv_host_alloc also allocates its device mirror (as many bytes of
 * HBM), so a block reserved once (e.g. at engine start, from the memtable's
 * capacity) costs the flushes that use it no allocation; smaller blocks, or a
 * mirror that does not fit the free HBM at that moment, get it on first use
 * (values that take the small path never need it). */
int nkv_host_alloc(nkv_ctx *ctx, uint64_t bytes, void **out);
int nkv_host_free(nkv_ctx *ctx, void *p);
int nkv_host_stream(nkv_ctx *ctx, const void *block, uint64_t upto);

/* ---- host-buffer API (synchronous) ---- */

/* NewLeaf over n values: value i = base[off[i] .. off[i]+len[i]).
 * out20: n * 20 bytes. */
int nkv_leaf_hash(nkv_ctx *ctx, const uint8_t *base, const uint64_t *off, const uint64_t *len,
                  uint64_t n, uint8_t *out20);

/* New() over n NewLeaf digests (leaf20: n * 20 bytes).  Outputs are
 * optional (NULL to skip): root20 (20 B), nodes_out (nkv_total_nodes(n) * 20 B),
 * img_out (nkv_bfs_size(n) B). */
int nkv_tree_build(nkv_ctx *ctx, const uint8_t *leaf20, uint64_t n, uint8_t *root20,
                   uint8_t *nodes_out, uint8_t *img_out);

/* makeMetadata: NewLeaf(value_i) for all i, then New, then the Serialize
 * image -- in one call. */
int nkv_tree_from_values(nkv_ctx *ctx, const uint8_t *base, const uint64_t *off,
                         const uint64_t *len, uint64_t n, uint8_t *root20, uint8_t *nodes_out,
                         uint8_t *img_out);

/* New() over leaves with arbitrary Data (leaf i = data[off[i] .. +len[i]),
 * README example ds/merkletree/README.md:44-57).  upper_out receives levels
 * 1..top ((nkv_total_nodes(n) - n) * 20 B).  img_out receives the Serialize
 * image (length nkv_generic_bfs_size()). */
uint64_t nkv_generic_bfs_size(const uint64_t *len, uint64_t n);
int nkv_tree_generic(nkv_ctx *ctx, const uint8_t *data, const uint64_t *off, const uint64_t *len,
                     uint64_t n, uint8_t *root20, uint8_t *upper_out, uint8_t *img_out);

/* (*MerkleTree).Validate (merkletree.go:162-171) of a tree New built from n
 * leaves: rehash (merklenode.go:99-108) recomputes every internal node from
 * the leaves' Data -- leaf i = leaf_data[off[i] .. off[i]+len[i]), a NewLeaf
 * leaf is its 20-byte digest, any other length is a generic leaf (README
 * example); pads contribute no bytes -- on the device, and compares the 20
 * bytes with root20 (the tree's Root.Data).  *ok = 1 if they match, else 0. */
int nkv_tree_validate(nkv_ctx *ctx, const uint8_t *leaf_data, const uint64_t *off, const uint64_t *len,
                      uint64_t n, const uint8_t *root20, int *ok);

/* Merkle step straight from a serialized Data-table stream (the records
 * written by record.Serialize, record.go:191-199) and the RecSize of each
 * record (record.KeyContext, record.go:38-41).  Leaves are the record Values
 * (sstable.go:62, lsmtree.go:211), hashed in place on the device. */
int nkv_tree_from_records(nkv_ctx *ctx, const uint8_t *stream, uint64_t stream_len,
                          const uint64_t *rec_size, uint64_t n, uint8_t *root20,
                          uint8_t *nodes_out, uint8_t *img_out);

/* Record checksums: CRC-32/IEEE of Key ++ Value of each
 * serialized record (stream and rec_size as for nkv_tree_from_records).
 * crc_out (nullable): n checksums, what record.New stores (record.go:51).
 * *n_bad: records whose stored Crc differs from the recomputed one, the check
 * record.Deserialize panics on (record.go:163-169); *first_bad: the lowest such
 * index, UINT64_MAX if none.  NKV_ERR_INVALID if a header points outside the
 * stream. */
int nkv_record_crc(nkv_ctx *ctx, const uint8_t *stream, uint64_t stream_len,
                   const uint64_t *rec_size, uint64_t n, uint32_t *crc_out, uint64_t *n_bad,
                   uint64_t *first_bad);

/* SSTable filter.  bloomfilter.New(n, p)'s sizing: m bits,
 * k hash functions (bloomfilter.go:18-24; n > 0, 0 < p < 1).  Hash j of a key is
 * MurmurHash3_x86_32(key, seed0 + j) % m (spaolacci/murmur3 Sum32; the reference
 * draws seed0 = uint32(time.Now().UnixNano()), bloomfilter.go:31 -- here it is
 * an argument).  Bit idx is Contents[idx / 8] & (1 << (idx % 8)). */
int nkv_bloom_params(uint64_t n, double p, uint32_t *m, uint32_t *k);
/* makeFilter over n keys (key i = keys + off[i], len[i]): bits_out receives
 * Contents, ceil(m / 8) bytes (bloomfilter.go:67). */
int nkv_bloom_build(nkv_ctx *ctx, const uint8_t *keys, const uint64_t *off, const uint64_t *len,
                    uint64_t n, uint32_t m, uint32_t k, uint32_t seed0, uint8_t *bits_out);
/* makeFilter over the keys of serialized records (stream and rec_size as for
 * nkv_tree_from_records; sstable.go:51-53 inserts KeyContext.Key). */
int nkv_bloom_from_records(nkv_ctx *ctx, const uint8_t *stream, uint64_t stream_len,
                           const uint64_t *rec_size, uint64_t n, uint32_t m, uint32_t k,
                           uint32_t seed0, uint8_t *bits_out);

/* Serialize()'s file semantics: open O_WRONLY|O_CREAT (mode 0666) WITHOUT
 * O_TRUNC (merkletree.go:68), write len bytes at offset 0, close. */
int nkv_write_file(const char *fname, const uint8_t *data, uint64_t len);

/* ---- device-resident API (asynchronous on the context stream) ---- */

/* level 0 of d_nodes from n values at d_base + d_off[i], d_len[i] (any alignment) */
int nkv_leaf_hash_dev(nkv_ctx *ctx, const void *d_base, const uint64_t *d_off,
                      const uint64_t *d_len, uint64_t n, void *d_nodes);
/* level 0 of d_nodes from n values of len bytes at d_base + i * stride */
int nkv_leaf_hash_strided_dev(nkv_ctx *ctx, const void *d_base, uint64_t stride, uint64_t len,
                              uint64_t n, void *d_nodes);
/* levels 1..top of d_nodes from its level 0 */
int nkv_tree_reduce_dev(nkv_ctx *ctx, void *d_nodes, uint64_t n);
/* leaf hash (order per NKV_OPT_BUCKET), then the tree levels */
int nkv_tree_from_values_dev(nkv_ctx *ctx, const void *d_base, const uint64_t *d_off,
                             const uint64_t *d_len, uint64_t n, void *d_nodes);
int nkv_tree_from_strided_dev(nkv_ctx *ctx, const void *d_base, uint64_t stride, uint64_t len,
                              uint64_t n, void *d_nodes);
/* Serialize() image of a 20-byte-leaf tree (nkv_bfs_size(n) bytes) */
int nkv_bfs_image_dev(nkv_ctx *ctx, const void *d_nodes, uint64_t n, void *d_img);
/* d_rec_off[i] = sum of d_rec_size[0..i) (exclusive scan of KeyContext.RecSize) */
int nkv_record_offsets_dev(nkv_ctx *ctx, const uint64_t *d_rec_size, uint64_t n,
                           uint64_t *d_rec_off);
/* value offset/length of each record; NKV_ERR_INVALID (after a sync) if a
 * header points outside the stream */
int nkv_locate_values_dev(nkv_ctx *ctx, const void *d_stream, uint64_t stream_len,
                          const uint64_t *d_rec_off, uint64_t n, uint64_t *d_voff,
                          uint64_t *d_vlen);
/* Merkle step of a device-resident Data table (compaction, lsmtree.go:211 /
 * sstable.go:41-46), asynchronous: the Value of each record at d_stream +
 * d_rec_off[i] (record.go:191-199) is located and hashed in place, and the full
 * tree goes to d_nodes.  d_err (nullable, 4 bytes on the device) receives 1 if
 * a header points outside the stream (that leaf hashes the empty value); with
 * d_err NULL the call synchronizes and returns NKV_ERR_INVALID instead. */
int nkv_tree_from_records_dev(nkv_ctx *ctx, const void *d_stream, uint64_t stream_len,
                              const uint64_t *d_rec_off, uint64_t n, void *d_nodes, uint32_t *d_err);
/* CRC-32/IEEE (Go crc32.ChecksumIEEE) of n byte spans d_base + d_off[i],
 * d_len[i] (any alignment) into d_crc[i] */
int nkv_crc32_dev(nkv_ctx *ctx, const void *d_base, const uint64_t *d_off, const uint64_t *d_len,
                  uint64_t n, uint32_t *d_crc);
/* Record checksums over Key ++ Value of the records at d_stream + d_rec_off[i].
 * d_crc (nullable): n checksums.  d_stats (nullable, 3 x u64 on the device,
 * overwritten): [0] records whose stored Crc differs, [1] the lowest such index
 * (UINT64_MAX if none), [2] 1 if a header points outside the stream. */
int nkv_record_crc_dev(nkv_ctx *ctx, const void *d_stream, uint64_t stream_len,
                       const uint64_t *d_rec_off, uint64_t n, uint32_t *d_crc, uint64_t *d_stats);
/* Compaction read of a device-resident Data table in one call, asynchronous:
 * the Merkle tree of the records' Values into d_nodes (as
 * nkv_tree_from_records_dev) and record.Deserialize's checksum check
 * (record.go:163-169) of every record, d_crc / d_stats as nkv_record_crc_dev
 * (a header outside the stream sets d_stats[2]; that leaf hashes the empty
 * value).  Records of similar sizes are read once for both (k_leaf_verify). */
int nkv_tree_verify_records_dev(nkv_ctx *ctx, const void *d_stream, uint64_t stream_len,
                                const uint64_t *d_rec_off, uint64_t n, void *d_nodes, uint32_t *d_crc,
                                uint64_t *d_stats);
/* Bloom filter bits on the device: d_bits holds ((m + 31) / 32) * 4 bytes
 * (Contents padded to whole 32-bit words, zero the padding); bits are OR-ed in,
 * so several calls build one filter. */
int nkv_bloom_insert_dev(nkv_ctx *ctx, const void *d_keys, const uint64_t *d_off,
                         const uint64_t *d_len, uint64_t n, uint32_t m, uint32_t k, uint32_t seed0,
                         void *d_bits);
/* keys of the records at d_stream + d_rec_off[i]; NKV_ERR_INVALID (after a
 * sync) if a header points outside the stream */
int nkv_bloom_insert_records_dev(nkv_ctx *ctx, const void *d_stream, uint64_t stream_len,
                                 const uint64_t *d_rec_off, uint64_t n, uint32_t m, uint32_t k,
                                 uint32_t seed0, void *d_bits);
/* d_out[i] = 1 if key i may be in the filter (every bit set), else 0 */
int nkv_bloom_query_dev(nkv_ctx *ctx, const void *d_keys, const uint64_t *d_off,
                        const uint64_t *d_len, uint64_t n, uint32_t m, uint32_t k, uint32_t seed0,
                        const void *d_bits, uint8_t *d_out);
/* synthetic input: byte j = byte (j % 8) of splitmix64(seed, j / 8) */
int nkv_fill_splitmix64_dev(nkv_ctx *ctx, void *d_buf, uint64_t nbytes, uint64_t seed);

/* ---- compaction merge (core/lsmtree/lsmtree.go:137-231) ----
 * k sorted runs of one level in, one Data table out.  A run is a Data-table
 * stream of whole serialized records (record.go:191-199) whose keys increase
 * strictly under bytes.Compare (unsigned lexicographic; a proper prefix sorts
 * first, the empty key is smallest).  The output holds one record per distinct
 * key in ascending key order, each copied byte for byte from its input (header,
 * stored Crc, Status and TypeInfo untouched).  Tombstones are kept: merge never
 * looks at Status.
 *
 * Among the records of one key the greatest Timestamp wins, compared as signed
 * int64.  Timestamps are whole seconds, so ties across runs are ordinary; the
 * reference settles them by the order in which the records entered its queue
 * (its sort of at most 6 elements is a stable insertion sort), which has this
 * closed form: the winner is the minimum under (Timestamp descending, then the
 * key of the record's predecessor in its own run ascending with "no
 * predecessor" smallest, then run index ascending).  For k > 6 the reference's
 * own result on a tie depends on the internals of its Go release's sort and is
 * not pinned; the library applies the closed form for every k.
 *
 * Errors: NKV_ERR_INVALID for k outside 1..NKV_MERGE_MAX_RUNS, a null pointer,
 * more than 2^31 - 1 records in all, out_cap below the sum of stream_len, and
 * for a run whose keys are not strictly increasing, whose header sizes reach
 * outside its stream, or whose records do not each end where the next one
 * starts (the first at 0, the last at stream_len).  The runs are validated by
 * a kernel of their own before any kernel follows a key or copies a record;
 * when it refuses, nothing further is launched and the context stays usable.
 * Empty runs (n = 0, stream_len = 0) are allowed; when every run is empty the
 * call returns NKV_OK with *n_out = 0 (the zero-leaf error belongs to the tree
 * call that would follow). */
#define NKV_MERGE_MAX_RUNS 16
typedef struct nkv_run { /* all pointers on the context's device */
    const void *stream;
    uint64_t stream_len;
    const uint64_t *rec_off; /* n record offsets, as nkv_record_offsets_dev writes them */
    uint64_t n;
} nkv_run;
/* Device-resident form.  d_out (out_cap >= sum of stream_len bytes, any
 * alignment) receives the merged stream, d_out_off (sum of n entries) the
 * offset of each output record, d_out_src (nullable, sum of n entries)
 * (run << 32) | index of the input record each output record was copied from.
 * *n_out / *out_len (host): records and bytes written; the call synchronizes.
 * d_out / d_out_off feed nkv_tree_from_records_dev, nkv_record_crc_dev and
 * nkv_bloom_insert_records_dev as they are.  Under NKV_TIMING_EVENTS the "leaf"
 * interval is rank + scans + scatter and the "reduce" interval the copy kernel. */
int nkv_merge_records_dev(nkv_ctx *ctx, const nkv_run *runs, int k, void *d_out, uint64_t out_cap,
                          uint64_t *d_out_off, uint64_t *d_out_src, uint64_t *n_out, uint64_t *out_len);
/* Host-memory form: run r is streams[r] (stream_len[r] bytes) with the RecSize
 * of each of its n[r] records in rec_size[r] (they must add up to stream_len[r]);
 * out (out_cap >= sum of stream_len) and out_rec_size (sum of n entries)
 * receive the merged table. */
int nkv_merge_records(nkv_ctx *ctx, const uint8_t *const *streams, const uint64_t *stream_len,
                      const uint64_t *const *rec_size, const uint64_t *n, int k, uint8_t *out,
                      uint64_t out_cap, uint64_t *out_rec_size, uint64_t *n_out, uint64_t *out_len);

/* ---- memtable flush (core/memtable/memtable.go:93-116) ----
 * A write log in, the Data table the memtable would flush out.  The log holds n
 * whole serialized records (record.go:191-199) in arrival order, one behind the
 * other: what CoreEngine.put hands to Memtable.Add, or a WAL segment's records.
 * No key order is required.  skiplist.Write (skiplist.go:62-120) compares keys
 * with bytes.Compare and replaces the whole record of a key that is already
 * there, so the flushed table holds one record per distinct key in ascending
 * key order (unsigned lexicographic; a proper prefix sorts first, the empty key
 * is smallest), and the record kept for a key is the one that arrived last,
 * copied byte for byte: Timestamp, Status and TypeInfo come along, a later
 * tombstone shadows a live record, and a later write with an older Timestamp
 * still wins (unlike the merge's rule).  In closed form: sort by (key
 * ascending, arrival index ascending) and keep position s iff it is the last
 * or the key at s + 1 differs.  That order is total, so there is no tie rule.
 * Memtable.Remove (the tombstone bit set in place) has no serialized form and
 * is not covered; the engine deletes through put.
 *
 * Errors: NKV_ERR_INVALID for a null context or a null pointer with n > 0,
 * n > 2^31 - 1, out_cap < log_len, log_len / 30 < n (n = 0 takes log_len = 0),
 * d_rec_off[0] != 0, a header outside the log, a KeySize or ValueSize that
 * reaches outside the log, and a record that does not end where the next one
 * starts (the last at log_len).  The log is validated by a kernel of its own
 * before any kernel follows an offset or copies a record; when it refuses,
 * nothing further is launched and the context stays usable.  n = 0 returns
 * NKV_OK with *n_out = 0.  Record checksums are not checked here
 * (nkv_record_crc_dev / nkv_tree_verify_records_dev in front do that). */
/* Device-resident form.  d_log (log_len bytes, any alignment) with d_rec_off (n
 * offsets, as nkv_record_offsets_dev writes them).  d_out (out_cap >= log_len
 * bytes, any alignment) receives the flushed stream, d_out_off (n entries) the
 * offset of each output record, d_out_src (nullable, n entries) the arrival
 * index of the input record each output record was copied from.  *n_out /
 * *out_len (host): records and bytes written; the call synchronizes.  d_out /
 * d_out_off feed nkv_tree_from_records_dev, nkv_bloom_insert_records_dev,
 * nkv_index_summary_dev, nkv_record_crc_dev and nkv_lookup_dev as they are.
 * Under NKV_TIMING_EVENTS the "leaf" interval is sort + survive + scans +
 * scatter and the "reduce" interval the copy kernel. */
int nkv_sort_records_dev(nkv_ctx *ctx, const void *d_log, uint64_t log_len, const uint64_t *d_rec_off, uint64_t n,
                         void *d_out, uint64_t out_cap, uint64_t *d_out_off, uint64_t *d_out_src,
                         uint64_t *n_out, uint64_t *out_len);
/* Host-memory form: log (log_len bytes) with the RecSize of each of its n
 * records in rec_size (they must add up to log_len); out (out_cap >= log_len)
 * and out_rec_size (n entries) receive the flushed table. */
int nkv_sort_records(nkv_ctx *ctx, const uint8_t *log, uint64_t log_len, const uint64_t *rec_size, uint64_t n,
                     uint8_t *out, uint64_t out_cap, uint64_t *out_rec_size, uint64_t *n_out, uint64_t *out_len);

/* ---- record encode (core/record/record.go:49-60,175-187) ----
 * The first step of the write path: CoreEngine.put calls record.New(key, val),
 * Record.ToBytes lays the record out, and the WAL appends those bytes
 * (wal.flushPartialBufferToSegment, core/wal/wal.go:199-232).  Here a batch of
 * n puts goes in and the write log comes out: record i is, little endian,
 *   Crc u32 | Timestamp i64 | Status u8 | TypeInfo u8 | KeySize u64 |
 *   ValueSize u64 | Key | Value
 * with Crc = crc32.ChecksumIEEE(Key ++ Value) (record.go:51; Timestamp, Status
 * and TypeInfo do not enter it) and TotalSize = 30 + KeySize + ValueSize, the
 * records one behind the other in input order.  record.New stamps
 * time.Now().Unix(), Status 0 and TypeInfo 0; NewTyped sets TypeInfo and
 * CoreEngine.Delete re-puts with Status |= 1, so the three are inputs: one
 * Timestamp for the batch or one per record, Status and TypeInfo 0 or one per
 * record.  The output feeds nkv_sort_records_dev and every other records
 * entry as it is. */
typedef struct nkv_puts {  /* pointers on the context's device (_dev form) or in host memory (host form) */
    const void *keys;      uint64_t keys_len;  /* key i   = keys[koff[i] .. koff[i] + klen[i]) */
    const uint64_t *koff;  const uint64_t *klen;
    const void *vals;      uint64_t vals_len;  /* value i = vals[voff[i] .. voff[i] + vlen[i]) */
    const uint64_t *voff;  const uint64_t *vlen;
    const int64_t *ts;     /* n Timestamps, or NULL: ts_all in every record */
    int64_t ts_all;
    const uint8_t *status; /* n Status bytes, or NULL: 0 */
    const uint8_t *type;   /* n TypeInfo bytes, or NULL: 0 */
    uint64_t n;
} nkv_puts;
/* Device form.  d_out (any byte alignment) receives the log: exactly *out_len
 * = 30 n + sum of klen + sum of vlen bytes are written; d_out_off (8-byte
 * aligned) the n record offsets; d_crc (nullable, 4-byte aligned) the n
 * checksums.  Keys and values may sit at any alignment, their spans may
 * overlap or repeat (one key or one value used by many records), and the two
 * blobs may lie any distance apart; koff, klen, voff, vlen and ts are 8-byte
 * aligned.  With d_out NULL the call is a size query: NKV_OK and the length
 * (d_out_off and d_crc are ignored and may be NULL).  A kernel checks every
 * span against its blob first and the host reads its verdict and the total
 * once (the call's one synchronize) before any writer is launched; after
 * NKV_OK the log is complete in stream order on the context's stream.
 * NKV_ERR_INVALID, with nothing written and the context still usable, for: a
 * null context, puts or out_len; n > 2^31 - 1; n > 0 with a null koff, klen,
 * voff or vlen; keys NULL with keys_len > 0, and the same for vals; a span
 * outside its blob (koff[i] > keys_len or klen[i] > keys_len - koff[i], the
 * same for values: a wrapped off + len is caught); out_cap < *out_len (the
 * length still reported, so the caller can retry); d_out_off NULL while d_out
 * is not and n > 0; keys_len + vals_len wrapping or n (30 + keys_len +
 * vals_len) >= 2^64 (checked before any launch); an output whose 16 KiB tiles
 * would pass 2^31 - 1.  n = 0 returns NKV_OK with *out_len = 0 and writes
 * nothing.  Under NKV_TIMING_EVENTS the "leaf" interval is everything before
 * the writer, the "reduce" interval the writer, the checksums and the patch of
 * the Crc fields. */
int nkv_encode_records_dev(nkv_ctx *ctx, const nkv_puts *puts, void *d_out, uint64_t out_cap,
                           uint64_t *d_out_off, uint32_t *d_crc, uint64_t *out_len);
/* Host-memory form: the same struct with host pointers; uploads, runs the
 * device form and downloads.  out (out_cap bytes) receives the log,
 * out_rec_size the n TotalSizes, crc_out (nullable) the n checksums.  With out
 * NULL it is a size query.  Synchronous. */
int nkv_encode_records(nkv_ctx *ctx, const nkv_puts *puts, uint8_t *out, uint64_t out_cap,
                       uint64_t *out_rec_size, uint32_t *crc_out, uint64_t *out_len);

/* ---- framing (core/record/record.go:119-172 in a loop) ----
 * Every records entry above takes the record boundaries from its caller.  For
 * bytes that come from disk the reference learns them by calling
 * record.Deserialize until it reports EOF: over a Data file in lsmtree.merge
 * (lsmtree.go:137-231) and over each WAL segment in wal.readEntireSegment
 * (wal.go:293-328).  This entry is that loop in closed form, for a stream cut
 * into S segments.
 *
 * Segment j is [d_seg_off[j], d_seg_off[j + 1]), the last one ends at
 * stream_len; d_seg_off NULL with S = 0 means the one segment [0, stream_len).
 * Offsets are non-decreasing and at most stream_len; equal neighbours are an
 * empty segment; bytes before d_seg_off[0] belong to no segment and are never
 * read as records.  Per segment, with p its start and end its end: the record
 * at p is accepted iff 30 header bytes fit (end - p >= 30), KeySize <= end - p
 * - 30 and ValueSize <= end - p - 30 - KeySize (no sum is formed before the
 * compare); an accepted record advances p by 30 + KeySize + ValueSize; the
 * first p that fails ends the segment and [p, end) is its tail -- Deserialize
 * returning eof on io.EOF or io.ErrUnexpectedEOF at whichever field.  A record
 * never crosses a segment end.
 *
 * Deviations from the reference: a KeySize or ValueSize so large that Go's make
 * panics is a tail like any other size that does not fit; and checksums are
 * not checked here (Deserialize panics on a bad one): nkv_record_crc_dev over
 * the framed records does that.
 *
 * Device form.  d_rec_off (8-byte aligned, rec_cap entries) receives the
 * accepted offsets, ascending, *n_out of them; d_seg_first (nullable, S + 1
 * entries) the index of each segment's first record, d_seg_first[S] = n;
 * d_seg_len (nullable, S entries) the bytes of whole records in each segment.
 * With S = 0 that is the one entry d_seg_first[0] = n and no d_seg_len entry.
 * stats: [0] n, [1] the sum of the segments' whole-record bytes, [2] the number
 * of segments with a non-empty tail, [3] the lowest such segment (UINT64_MAX if
 * none).  Exactly those extents are written.  With d_rec_off NULL the call is
 * a size query: NKV_OK, *n_out and stats, nothing written.  The call
 * synchronizes: the host reads the counts before any output is written.
 *
 * NKV_ERR_INVALID, with no device output written and the context usable, for:
 * a null context, n_out or stats; a null stream with stream_len > 0; S > 0 with
 * a null d_seg_off; segment offsets that decrease or pass stream_len (a kernel
 * checks them before any kernel follows one); n or S above 2^31 - 1; rec_cap <
 * n (*n_out and stats still reported, so the caller can retry); NKV_FRAME_STRICT
 * with stats[2] > 0 (*n_out and stats still reported: stats[1] is where a
 * one-segment stream's tail starts).  stream_len = 0 gives NKV_OK with n = 0.
 * Under NKV_TIMING_EVENTS the "leaf" interval is mark, scans and successor
 * (walk: the count pass and its scan), the "reduce" interval the doubling
 * rounds and the compaction (walk: the write pass).  NKV_OPT_FRAME_PATH picks
 * the path, NKV_OPT_FRAME_BUDGET bounds the speculative path's scratch. */
#define NKV_FRAME_STRICT 1  /* any tail is NKV_ERR_INVALID (a Data table); without it tails are
                               dropped as Deserialize's EOF drops them (a WAL) */
int nkv_frame_records_dev(nkv_ctx *ctx, const void *d_stream, uint64_t stream_len,
                          const uint64_t *d_seg_off, uint64_t S, int flags, uint64_t *d_rec_off,
                          uint64_t rec_cap, uint64_t *d_seg_first, uint64_t *d_seg_len,
                          uint64_t *n_out, uint64_t stats[4]);
/* Host-memory form: uploads, runs the device form and returns the TotalSize of
 * each record in rec_size_out (rec_cap entries) instead of offsets; with tails
 * dropped, the sizes of segment j add up to seg_len_out[j].  seg_first_out
 * (S + 1 entries) and seg_len_out (S entries) are nullable; rec_size_out NULL
 * is the size query.  Synchronous. */
int nkv_frame_records(nkv_ctx *ctx, const uint8_t *stream, uint64_t stream_len,
                      const uint64_t *seg_off, uint64_t S, int flags, uint64_t *rec_size_out,
                      uint64_t rec_cap, uint64_t *seg_first_out, uint64_t *seg_len_out,
                      uint64_t *n_out, uint64_t stats[4]);

/* ---- sketches: HyperLogLog (ds/hll) and Count-Min Sketch (ds/cmsketch) ----
 * The only typed values the reference's engine knows (WrapperEngine.PutHLL /
 * PutCMS, engine/wrappereng/wrappereng.go:57-83).  Both hash every key with
 * MurmurHash3_x86_32 (spaolacci/murmur3 Sum32), as the filter does.
 *
 * HLL, precision p in [NKV_HLL_MIN_PRECISION, NKV_HLL_MAX_PRECISION], 2^p
 * registers of one byte.  Add(key) (hll.go:43-62): h = murmur3(key, seed 0),
 * Reg[h >> (32 - p)] = max(itself, 1 + TrailingZeros32(h)), which is 33 for
 * h == 0 (the empty key: it sets Reg[0] = 33).
 *
 * CMS, K rows of M uint32_t counters.  Row i hashes with seed seed0 + i
 * (cmsketch.go:28-38; the reference draws seed0 from the clock, here it is an
 * argument, modulo 2^32).  Insert (:76-87) adds 1 to Contents[i][murmur3(key,
 * seed0 + i) % M] in every row, in uint32_t arithmetic: a counter wraps at
 * 2^32.  Query (:91-111) is the minimum of those K counters.
 *
 * Deviations from the reference: cmsketch.New accepts epsilon = 0, delta = 0
 * and delta = 1 (+Inf conversions, K = 0); nkv_cms_params returns
 * NKV_ERR_INVALID unless 0 < epsilon <= 1, 0 < delta < 1 and M <= 2^32 - 1, and
 * the insert and query entries need M >= 1, K >= 1 and K M <= 2^31 - 1.  The gob
 * encodings (EncodeToBytes / DecodeFromBytes) are not covered.
 *
 * Argument rules, as for the filter entries: NKV_ERR_INVALID for a null
 * context, p outside [4, 16], m = 0, k = 0, K M too large, a null output (or
 * null d_table of the query), n > 2^31 - 1; then n = 0 returns NKV_OK and
 * touches nothing; then a null input is NKV_ERR_INVALID.  Max and wrapping add
 * commute: the result does not depend on NKV_OPT_SKETCH_PATH, on the grid or on
 * how the keys are split over calls. */
#define NKV_HLL_MIN_PRECISION 4
#define NKV_HLL_MAX_PRECISION 16
#define NKV_HLL_ESTIMATE_REFERENCE 0 /* hll.go:75-92, literal */
#define NKV_HLL_ESTIMATE_STANDARD 1  /* sum of 2^-Reg, same alpha and corrections */

/* Device forms, asynchronous on the context's stream.  Keys as for
 * nkv_bloom_insert_dev (d_keys + d_off[i], d_len[i], any alignment) or the keys
 * of the records at d_stream + d_rec_off[i]; the records forms return
 * NKV_ERR_INVALID (after a sync) if a header or key reaches outside the stream
 * (that record contributes nothing).  d_reg: 2^p bytes, 4-byte aligned, max-ed
 * in place, so several calls build one HLL.  d_table: k rows of m uint32_t, row
 * i at d_table + i * m, 4-byte aligned, added to in place. */
int nkv_hll_add_dev(nkv_ctx *ctx, const void *d_keys, const uint64_t *d_off, const uint64_t *d_len,
                    uint64_t n, int p, void *d_reg);
int nkv_hll_add_records_dev(nkv_ctx *ctx, const void *d_stream, uint64_t stream_len,
                            const uint64_t *d_rec_off, uint64_t n, int p, void *d_reg);
int nkv_cms_insert_dev(nkv_ctx *ctx, const void *d_keys, const uint64_t *d_off, const uint64_t *d_len,
                       uint64_t n, uint32_t m, uint32_t k, uint32_t seed0, uint32_t *d_table);
int nkv_cms_insert_records_dev(nkv_ctx *ctx, const void *d_stream, uint64_t stream_len,
                               const uint64_t *d_rec_off, uint64_t n, uint32_t m, uint32_t k,
                               uint32_t seed0, uint32_t *d_table);
/* d_out[i] = the minimum over the k rows */
int nkv_cms_query_dev(nkv_ctx *ctx, const void *d_keys, const uint64_t *d_off, const uint64_t *d_len,
                      uint64_t n, uint32_t m, uint32_t k, uint32_t seed0, const uint32_t *d_table,
                      uint32_t *d_out);

/* Host-pointer forms, synchronous, staged like nkv_bloom_build /
 * nkv_bloom_from_records (stream and rec_size as for nkv_tree_from_records);
 * reg (2^p bytes) and table (k m counters) are read, updated and written back. */
int nkv_hll_add(nkv_ctx *ctx, const uint8_t *keys, const uint64_t *off, const uint64_t *len,
                uint64_t n, int p, uint8_t *reg);
int nkv_hll_add_records(nkv_ctx *ctx, const uint8_t *stream, uint64_t stream_len,
                        const uint64_t *rec_size, uint64_t n, int p, uint8_t *reg);
int nkv_cms_insert(nkv_ctx *ctx, const uint8_t *keys, const uint64_t *off, const uint64_t *len,
                   uint64_t n, uint32_t m, uint32_t k, uint32_t seed0, uint32_t *table);
int nkv_cms_insert_records(nkv_ctx *ctx, const uint8_t *stream, uint64_t stream_len,
                           const uint64_t *rec_size, uint64_t n, uint32_t m, uint32_t k,
                           uint32_t seed0, uint32_t *table);
int nkv_cms_query(nkv_ctx *ctx, const uint8_t *keys, const uint64_t *off, const uint64_t *len,
                  uint64_t n, uint32_t m, uint32_t k, uint32_t seed0, const uint32_t *table,
                  uint32_t *out);

/* Pure host functions, no context.  nkv_cms_params: M = ceil(e / epsilon),
 * K = ceil(ln(1 / delta)) (cmsketch.go:18-24).  nkv_hll_estimate over 2^p
 * registers: mode NKV_HLL_ESTIMATE_REFERENCE is (*HLL).Estimate taken literally
 * -- its sum adds math.Pow(float64(-val), 2) with val a uint8, so -val wraps
 * and the term is (256 - val)^2 (0 for an empty register), not 2^-val; alpha =
 * 0.7213 / (1 + 1.079 / M); estimation = alpha M^2 / sum; below 2.5 M with
 * empty registers it is M ln(M / empty), above 2^32 / 30 it is -2^32 ln(1 -
 * estimation / 2^32).  In effect: linear counting while empty registers
 * remain, a meaningless small number after that, NaN for an empty HLL.  Mode
 * NKV_HLL_ESTIMATE_STANDARD sums 2^-val instead, the rest unchanged. */
int nkv_cms_params(double epsilon, double delta, uint32_t *m, uint32_t *k);
int nkv_hll_estimate(const uint8_t *reg, int p, int mode, double *out);

/* ---- Index and Summary tables (core/sstable/sstable.go:76-139) ----
 * makeIndexAndSummary over a Data table: for records i = 0..n-1 with key K_i
 * of ks_i bytes,
 *   Index    entry i = ks_i (u64 LE) | Offset (i64 LE) = the record's offset
 *            in the Data table (d_rec_off[i] as given) | K_i, the entries
 *            concatenated: index_len = 16 n + sum of ks_i bytes;
 *   Summary  MinKeySize u64 | MaxKeySize u64 | Payload u64 | MinKey = K_0 |
 *            MaxKey = K_(n-1), then one entry ks_i | Offset = the byte offset
 *            of Index entry i in the Index | K_i for every selected i in
 *            ascending order; record i is selected when i == 0, i % page_size
 *            == 0 or i == n - 1 (once each); Payload = the bytes of all the
 *            entries.  nkv_summary_entries(n, page_size) is their count: n for
 *            n <= 1, else 1 + (n - 1) / page + ((n - 1) % page ? 1 : 0).
 * n == 0 gives an empty Index and the 24 zero bytes of an empty header.
 * page_size == 0 is NKV_ERR_INVALID for n >= 2 (the reference divides by it
 * at i = 1) and accepted for n <= 1; nkv_summary_entries returns 0 for the
 * refused case.  Keys are encoded as they come: no order check, duplicates
 * and the empty key included.
 *
 * Device form.  d_stream / d_rec_off as for nkv_tree_from_records_dev (the
 * merge's d_out / d_out_off as they are).  d_index / d_summary (any byte
 * alignment) receive the images, *index_len / *summary_len (host) their
 * lengths, and exactly those extents are written.  With d_index and d_summary
 * both NULL the call is a size query: NKV_OK and the two lengths.  A kernel
 * checks every header and key span against the stream first, and the host
 * reads its verdict and the lengths once (the call's one synchronize) before
 * any writer is launched: NKV_ERR_INVALID, and nothing written, for a header
 * or a key that reaches outside the stream (lengths 0), and for index_cap <
 * *index_len or summary_cap < *summary_len (the lengths still reported, so
 * the caller can retry).  After NKV_OK the images are complete in stream
 * order.  Also NKV_ERR_INVALID: n > 2^31 - 1, a NULL index_len / summary_len,
 * one output NULL while its image is not empty, n (16 + stream_len) >= 2^64.
 * For a well-formed table (every key inside its own record, the records not
 * overlapping) index_cap = stream_len - 14 n is always enough: each record
 * spends 30 header bytes where its Index entry spends 16.  Under
 * NKV_TIMING_EVENTS the "leaf" interval is the measure kernel and the scans,
 * the "reduce" interval the writers. */
uint64_t nkv_summary_entries(uint64_t n, uint64_t page_size);
int nkv_index_summary_dev(nkv_ctx *ctx, const void *d_stream, uint64_t stream_len,
                          const uint64_t *d_rec_off, uint64_t n, uint64_t page_size, void *d_index,
                          uint64_t index_cap, void *d_summary, uint64_t summary_cap,
                          uint64_t *index_len, uint64_t *summary_len);
/* Host-memory form: stream and rec_size as for nkv_tree_from_records (the sizes
 * must add up to stream_len); uploads, runs the device form, copies the images
 * back.  Size query and capacities as above. */
int nkv_index_summary_from_records(nkv_ctx *ctx, const uint8_t *stream, uint64_t stream_len,
                                   const uint64_t *rec_size, uint64_t n, uint64_t page_size,
                                   uint8_t *index_out, uint64_t index_cap, uint8_t *summary_out,
                                   uint64_t summary_cap, uint64_t *index_len, uint64_t *summary_len);

/* ---- point lookup (engine/coreeng/coreeng.go:99-160, the disk part of get) ----
 * A batch of q keys looked up in T device-resident tables.  The reference
 * walks the tables in search order (levels ascending, runs descending: the
 * caller lists them that way) and per table runs Filter.Query, then
 * FindSummaryTableEntry, then FindIndexTableEntry, then record.Deserialize at
 * the Data offset; the first table that holds the key answers, even with a
 * tombstone.  Over a resident Data table the two Find steps have a closed form
 * (tests/lookup_ref.py holds it to a literal restatement): with keys K_0 <
 * ... < K_(n-1) compared as bytes.Compare does (unsigned, a proper prefix
 * sorts first), FindSummaryTableEntry gives Offset -1 exactly when key < K_0
 * or key > K_(n-1), and FindIndexTableEntry exactly when no K_j equals the
 * key.  The tables' keys are assumed strictly increasing -- what the merge
 * validates and writes; this call does not check it again.
 *
 * A table is its Data table (stream, rec_off as for nkv_tree_from_records_dev)
 * and, optionally, its filter: bits = the words nkv_bloom_insert[_records]_dev
 * leaves (((m + 31) / 32) * 4 bytes, 4-byte aligned) with its m, k and first
 * seed.  bits NULL: no filter, every key passes.  A filter that rejects a key
 * its table in fact holds makes that table report FILTER and the search move
 * on, exactly as the reference would. */
#define NKV_LOOKUP_MAX_TABLES 32
typedef struct nkv_lookup_table { /* all pointers on the context's device */
    const void *stream;      /* Data table, as for nkv_tree_from_records_dev */
    uint64_t stream_len;
    const uint64_t *rec_off; /* n record offsets */
    uint64_t n;              /* >= 1 */
    const void *bits;        /* filter words as nkv_bloom_insert_dev leaves them; NULL = no filter, every key passes */
    uint32_t m, k, seed0;
} nkv_lookup_table;

#define NKV_STAGE_NOT_SEARCHED 0 /* an earlier table answered */
#define NKV_STAGE_FILTER 1       /* Filter.Query said no */
#define NKV_STAGE_SUMMARY 2      /* key < K_0 or key > K_(n-1): FindSummaryTableEntry's Offset -1 */
#define NKV_STAGE_INDEX 3        /* in range, no equal key: FindIndexTableEntry's Offset -1 */
#define NKV_STAGE_FOUND 4
#define NKV_GET_ABSENT 0
#define NKV_GET_LIVE 1
#define NKV_GET_TOMBSTONE 2      /* found, Status & 1: the engine answers "not found" and stops */

/* Asynchronous on the context's stream.  Query i is the d_klen[i] bytes at
 * d_keys + d_koff[i], at any alignment; the empty key and duplicate queries are
 * allowed.  d_hit[i] = (table << 32) | record index of the first table, in the
 * order given, whose search ends FOUND, UINT64_MAX if none does; d_status[i]
 * one of the NKV_GET codes; d_stage (nullable, q * T bytes): d_stage[i * T + t]
 * the NKV_STAGE at which table t's search for query i ended.
 *
 * d_err (nullable, one uint32_t, need not be initialised) receives 1 if a
 * probed record's header or key span reaches outside its stream, else 0.  Such
 * a probe counts as "no match" (its table's search ends at INDEX) and nothing
 * outside the stream is read.  With d_err NULL the call synchronizes and
 * returns NKV_ERR_INVALID in that case.  Also NKV_ERR_INVALID, with nothing
 * launched: T outside 1..NKV_LOOKUP_MAX_TABLES, a table with n = 0 (the
 * reference cannot write one: New panics on zero leaves) or a NULL stream or
 * rec_off, a filter with k > 0 and m = 0, n or q above 2^31 - 1, a NULL
 * required pointer.  q = 0 returns NKV_OK and writes nothing.
 *
 * The found record's stored Crc is not checked (record.Deserialize does,
 * record.go:163-169): a caller who wants that runs nkv_record_crc_dev over the
 * table. */
int nkv_lookup_dev(nkv_ctx *ctx, const nkv_lookup_table *tables, int T, const void *d_keys,
                   const uint64_t *d_koff, const uint64_t *d_klen, uint64_t q, uint64_t *d_hit,
                   uint8_t *d_status, uint8_t *d_stage, uint32_t *d_err);
/* The Values of the LIVE hits, packed in query order: Value i is
 * d_out[d_out_off[i] .. d_out_off[i + 1]), and a query whose status is ABSENT
 * or TOMBSTONE contributes 0 bytes.  d_hit / d_status / tables as the lookup
 * took and left them.  d_out_off holds q + 1 entries; d_out may sit at any byte
 * alignment, and exactly *out_len (host) bytes of it are written.  With d_out
 * NULL the call is a size query (d_out_off may be NULL too): NKV_OK and the
 * length.  A kernel checks every hit's Value span against its stream first and
 * the host reads its verdict and the length once (the call's one synchronize)
 * before anything is written: NKV_ERR_INVALID, and nothing written, for a hit
 * that names no record or whose Value reaches outside its stream (length 0),
 * and for out_cap < *out_len (the length still reported, so the caller can
 * retry).  q = 0 gives *out_len = 0 and d_out_off[0] = 0.  Under
 * NKV_TIMING_EVENTS the "leaf" interval is the measure kernel, the scan and
 * the host's read of the length, the "reduce" interval the copy of the offsets
 * and the copy kernel. */
int nkv_lookup_values_dev(nkv_ctx *ctx, const nkv_lookup_table *tables, int T, const uint64_t *d_hit,
                          const uint8_t *d_status, uint64_t q, void *d_out, uint64_t out_cap,
                          uint64_t *d_out_off, uint64_t *out_len);

/* ---- index lookup (the same get, over tables whose Data file stays on disk) ----
 * nkv_lookup_dev answers over tables whose whole Data stream is resident.  The
 * engine's get never touches Data until Filter, Summary and Index have named
 * one record offset, and a table's Index is about a hundredth of its Data: a
 * key directory on the device -- the filter words and the Index of every table
 * -- takes a batch of keys and returns, per key, the answering table and the
 * record's Data-file offset; the host then does one pread per hit.
 *
 * Both files are chains of entries KeySize u64 | Offset i64 | Key with no
 * offsets beside them (the Summary behind MinKeySize u64 | MaxKeySize u64 |
 * Payload u64 | MinKey | MaxKey), so a table is opened first.  Call an
 * Index/Summary pair canonical when (n Index entries, s Summary entries)
 *   1. the Summary holds its 24-byte header, MinKey, MaxKey and Payload bytes
 *      (bytes behind them are ignored, as the reference ignores them);
 *   2. the payload is a whole chain of s >= 1 entries ending exactly at Payload;
 *   3. the Index is a whole chain of n >= 1 entries ending exactly at index_len;
 *   4. every Summary entry's Offset is the byte offset of an Index entry with
 *      the same KeySize and Key, the first names Index entry 0, the last names
 *      entry n - 1, and the named entries strictly ascend;
 *   5. the Index keys strictly increase under bytes.Compare;
 *   6. MinKey = K_0 and MaxKey = K_(n-1).
 * An entry whose KeySize reaches past the end of its image ends its chain
 * there (the reference's Read reports EOF).  Everything makeIndexAndSummary
 * writes from a flushed or merged table is canonical at any page size, and so
 * is any other partition into pages.  On a canonical pair FindSummaryTableEntry
 * and FindIndexTableEntry reduce to: SUMMARY exactly when key < K_0 or key >
 * K_(n-1); else, with j the lower bound of the key among the Index keys, FOUND
 * with entry j's stored Offset if K_j equals the key and that stored Offset is
 * not -1 (coreeng.go:138 tests the stored field), INDEX otherwise
 * (tests/index_open_ref.py holds this to the literal restatement).  A pair that
 * is not canonical is refused by the open and never reaches the locate: the
 * reference's answer on it depends on its scan order, and its one-key host
 * reader remains the way to serve it. */
#define NKV_INDEX_BAD_HEADER 1         /* condition 1 */
#define NKV_INDEX_BAD_SUMMARY_CHAIN 2  /* condition 2 */
#define NKV_INDEX_BAD_INDEX_CHAIN 4    /* condition 3 */
#define NKV_INDEX_BAD_LINK 8           /* condition 4 */
#define NKV_INDEX_BAD_ORDER 16         /* condition 5 */
#define NKV_INDEX_BAD_RANGE 32         /* condition 6 */
/* Parse and validate one pair.  Synchronous: it hands n to the host.  Both
 * images on the context's device, at any byte alignment; d_ent_off (8-byte
 * aligned, ent_cap entries) receives the n byte offsets of the Index entries,
 * ascending -- exactly n entries, and only when the verdict is 0.  n_out, s_out
 * and verdict are host pointers.  *verdict = 0 for a canonical pair, else a bit
 * mask whose lowest set bit names the first failed condition (later ones are
 * not evaluated); a refused pair returns NKV_OK with *n_out = *s_out = 0.  With
 * d_ent_off NULL the call is a size query: n, s and the verdict.  ent_cap < n
 * returns NKV_ERR_INVALID with n still reported; index_len / 16 entries are
 * always enough.  NKV_ERR_INVALID, with nothing launched: a NULL context, image
 * or host pointer, index_len or summary_len of 0; and n or s above 2^31 - 1.
 * Nothing outside the two images is read, whatever their bytes say.
 *
 * The Summary chain is followed by one lane or in chunks
 * (NKV_OPT_INDEX_OPEN_PATH); the Index chain by one lane per Summary page, so a
 * table written as one giant page parses at the one-lane rate.  Scratch is the
 * context's: about index_len / 2 + 2 * Payload bytes. */
int nkv_index_open_dev(nkv_ctx *ctx, const void *d_index, uint64_t index_len, const void *d_summary,
                       uint64_t summary_len, uint64_t *d_ent_off, uint64_t ent_cap, uint64_t *n_out,
                       uint64_t *s_out, uint32_t *verdict);

typedef struct nkv_index_table { /* all pointers on the context's device */
    const void *index;       /* the Index file's bytes, any alignment */
    uint64_t index_len;
    const uint64_t *ent_off; /* n entry offsets, from a verdict-0 nkv_index_open_dev */
    uint64_t n;              /* >= 1 */
    const void *bits;        /* filter words, as nkv_lookup_table */
    uint32_t m, k, seed0;
} nkv_index_table;
#define NKV_GET_LOCATED 3 /* found in an Index; Status is in the Data record on disk */

/* Asynchronous on the context's stream.  Queries as nkv_lookup_dev takes them.
 * Per table, in the order given: the filter test, the range test against
 * entries 0 and n - 1, a lower bound over ent_off with each probed key read in
 * place.  For the first table whose search ends FOUND: d_hit[i] =
 * ((uint64_t)(table_base + t) << 32) | entry index, d_data_off[i] = the entry's
 * stored Offset, d_status[i] = NKV_GET_LOCATED; when none does: UINT64_MAX, -1
 * and NKV_GET_ABSENT.  d_stage (nullable, q * T bytes) holds the NKV_STAGE
 * codes; a stored Offset of -1 ends that table's search at INDEX.
 *
 * With overlay 1 a query whose d_status[i] is not NKV_GET_ABSENT is left
 * exactly as it was in d_hit, d_data_off and d_status, and its stage row is all
 * NOT_SEARCHED: the call lays the disk tables under the answers of
 * nkv_lookup_dev and nkv_memtable_find_dev (d_data_off is then read only where
 * the status is LOCATED).  The search order is the caller's: every resident
 * table ahead of every Index-only one.
 *
 * d_err as in nkv_lookup_dev: 1 if a probed entry reaches outside its image
 * (that probe counts as no match); with d_err NULL the call synchronizes and
 * returns NKV_ERR_INVALID in that case.  Also NKV_ERR_INVALID, with nothing
 * launched: T outside 1..NKV_LOOKUP_MAX_TABLES, table_base + T above 65536, a
 * table with n = 0 or a NULL index or ent_off, a filter with k > 0 and m = 0, n
 * or q above 2^31 - 1, a NULL required pointer.  q = 0 writes nothing. */
int nkv_locate_dev(nkv_ctx *ctx, const nkv_index_table *tables, int T, uint32_t table_base,
                   const void *d_keys, const uint64_t *d_koff, const uint64_t *d_klen, uint64_t q,
                   int overlay, uint64_t *d_hit, int64_t *d_data_off, uint8_t *d_status,
                   uint8_t *d_stage, uint32_t *d_err);

/* ---- live memtable (core/memtable/memtable.go:40-90 over core/skiplist) ----
 * Memtable.Add, Find, Count and ShouldFlush over a write log that stays on the
 * device: the log nkv_encode_records_dev leaves (or a framed WAL segment) and
 * nkv_sort_records_dev, the flush, takes.  A put batch, a read of it and the
 * flush share one copy of the bytes.  There is no host-pointer form: the
 * structure's state lives on the device.
 *
 * The index is caller-owned device memory: nkv_memtable_index_bytes(slots)
 * bytes, 8-byte aligned, slots a power of two.  Its bytes are opaque and may
 * differ from run to run; no answer derived from it does.  d_state is four
 * uint64_t, 8-byte aligned: [0] Count, [1] memusage, [2] records indexed, [3]
 * flush_at.
 *
 * What the reference's Add computes (tests/live_memtable_ref.py restates it
 * statement by statement): the last write of a key replaces the whole record
 * whatever its Timestamp or Status (skiplist.go:81), Add returns true exactly
 * for the first write of a key since the clear, and memusage is the sum of
 * TotalSize over those first writes -- an overwrite adds nothing, because
 * skiplist.Write's oldNode aliases the node it has just updated
 * (skiplist.go:80-81; DESIGN.md "Live memtable").  ShouldFlush (memtable.go:
 * 70-73) is (strategy & NKV_FLUSH_BY_CAPACITY && Count == capacity) ||
 * (strategy & NKV_FLUSH_BY_THRESHOLD && memusage >= threshold): equality for
 * the capacity, so a memtable already above it never fires by capacity.
 * Memtable.Remove (never called by the engine: Delete goes through put) and
 * the LRU step of get are not provided. */
#define NKV_FLUSH_BY_CAPACITY 1  /* coreconf.go:22 */
#define NKV_FLUSH_BY_THRESHOLD 2 /* coreconf.go:23 */
#define NKV_MEMTABLE_STATE_WORDS 4
/* 8 * slots; 0 unless slots is a power of two in 2..2^32 */
uint64_t nkv_memtable_index_bytes(uint64_t slots);
/* skiplist.Clear + memusage = 0 (memtable.go:97-98): every slot empty, Count,
 * memusage and the indexed count 0, flush_at UINT64_MAX.  Asynchronous.
 * NKV_ERR_INVALID for a NULL pointer or a refused slots. */
int nkv_memtable_clear_dev(nkv_ctx *ctx, void *d_index, uint64_t slots, uint64_t *d_state);
/* Memtable.Add of records [n_done, n) of the log (d_log, log_len, d_rec_off as
 * nkv_sort_records_dev takes them: dense, log_len the bytes up to the end of
 * record n - 1), whose records [0, n_done) earlier calls indexed; the log's
 * bytes and offsets up to n_done must be unchanged since (the caller's
 * contract, not checked).  Asynchronous on the context's stream.
 *
 * After a successful add d_state[0] and [1] are what n sequential Adds since
 * the clear leave, with no flush in between, [2] = n, and [3] = flush_at: the
 * smallest arrival index i in [n_done, n) after whose Add ShouldFlush() is true
 * under strategy / capacity / threshold, UINT64_MAX if there is none.  When it
 * is set the caller does what the engine does (coreeng.go:214-218): flush
 * records [0, flush_at], clear, add the rest as a new log.  d_is_new (nullable,
 * n - n_done bytes at any address): d_is_new[i - n_done] = Add's return value
 * for write i.  n == n_done writes flush_at = UINT64_MAX (and 0 to d_err) and
 * nothing else.
 *
 * NKV_ERR_INVALID, with nothing launched: a NULL required pointer, n_done > n,
 * n above 2^31 - 1, slots not a power of two in 2..2^32, n > slots / 2 (the
 * load stays at or below one half, so every probe is finite), log_len / 30 < n.
 * Device-side verdicts go to d_err (nullable, one uint32_t, need not be
 * initialised; nonzero = the add was refused and the index, d_state and
 * d_is_new are unchanged): bit 0 a record whose span does not hold or that
 * does not end where the next starts (the last: at log_len), bit 1 an indexed
 * count d_state[2] that is not n_done; bit 2 a probe that met no empty slot or
 * a slot that names no record of this log -- the index was not cleared or is
 * another log's, and may have been written.  With d_err NULL the call
 * synchronizes and returns NKV_ERR_INVALID in those cases.
 *
 * Under NKV_TIMING_EVENTS the "leaf" interval is the validation, the insert
 * and the new-write flags, the "reduce" interval the two scans, the flush
 * point and the state update. */
int nkv_memtable_add_dev(nkv_ctx *ctx, const void *d_log, uint64_t log_len, const uint64_t *d_rec_off,
                         uint64_t n_done, uint64_t n, void *d_index, uint64_t slots, int strategy,
                         uint64_t capacity, uint64_t threshold, uint64_t *d_state, uint8_t *d_is_new,
                         uint32_t *d_err);
/* Memtable.Find for q keys (queries as nkv_lookup_dev takes them: any
 * alignment, the empty key and duplicates allowed) over the n indexed records.
 * For a key the memtable holds, tombstones included (get then answers "not
 * found" and stops, coreeng.go:80-85): d_hit[i] = ((uint64_t)table_id << 32) |
 * arrival index of its latest write, d_status[i] = NKV_GET_LIVE or
 * NKV_GET_TOMBSTONE (Status & 1).  For a key it does not hold: with overlay 0
 * UINT64_MAX and NKV_GET_ABSENT; with overlay 1 both entries are left exactly
 * as they were, so the call overlays nkv_lookup_dev's answers, and
 * nkv_lookup_values_dev packs the Values of both with the log listed as table
 * table_id (stream = d_log, rec_off, n, no filter).
 *
 * d_err (nullable, one uint32_t, need not be initialised) receives 1 if a
 * probed record's key span reaches outside the log or a slot names no record
 * below n, else 0; that probe counts as no match and nothing outside the log
 * is read.  With d_err NULL the call synchronizes and returns NKV_ERR_INVALID
 * in that case.  Also NKV_ERR_INVALID, with nothing launched: a NULL required
 * pointer (d_log and d_rec_off may be NULL when n = 0), a refused slots, n or q
 * above 2^31 - 1, table_id >= NKV_LOOKUP_MAX_TABLES.  q = 0 returns NKV_OK and
 * writes nothing.  The call records no timing interval. */
int nkv_memtable_find_dev(nkv_ctx *ctx, const void *d_log, uint64_t log_len, const uint64_t *d_rec_off,
                          uint64_t n, const void *d_index, uint64_t slots, const void *d_keys,
                          const uint64_t *d_koff, const uint64_t *d_klen, uint64_t q, uint32_t table_id,
                          int overlay, uint64_t *d_hit, uint8_t *d_status, uint32_t *d_err);

/* ---- engine admission (engine/coreeng/coreeng.go:47-75, 165-199, 223-234
 *      over ds/tokenbucket/tokenbucket.go:51-83) ----
 * The step CoreEngine.Put, Get and Delete run first, for a batch of n requests
 * (user, key, now) in arrival order: IsLegal(key) -- a key whose first
 * start_len bytes equal conf.InternalStart is refused before any bucket is
 * read, so it is not part of its user's sequence -- then the user's token
 * bucket, getTokenBucket -> HasEnoughTokens.  A bucket is (MaxTokens, Tokens,
 * Timestamp, ResetInterval), four int64; ToBytes writes them as four
 * little-endian u64 in that order, 32 bytes.  HasEnoughTokens at time now: if
 * now - Timestamp > ResetInterval then Timestamp = now, Tokens = MaxTokens - 1,
 * allow; else if Tokens > 0 then Tokens--, allow; else deny with the state
 * unchanged.  The engine puts the bucket record (key InternalStart ++ user,
 * Value = the image) for every allowed request and nothing for a denied one.
 * Every time.Now().Unix() of one request is the one caller-supplied now_i
 * here.  tests/admit_ref.py restates all of it statement by statement.
 *
 * Requests: user i is the ulen[i] bytes at users + uoff[i] (any alignment, the
 * empty user and repeated or overlapping spans allowed), key i likewise; with
 * koff NULL there is no IsLegal step and every request is legal.  ts holds n
 * times, or is NULL and ts_all is the time of all (as nkv_puts).  Times must be
 * non-decreasing over the whole batch, not only within a user: that is what
 * makes a user's windows well defined, and with the range below it keeps
 * now - Timestamp from wrapping.  Stored buckets (buckets, boff and bstatus
 * NULL together = every bucket fresh): bstatus[i] is a status byte as
 * nkv_lookup_dev / nkv_memtable_find_dev write it, NKV_GET_LIVE meaning "the 32
 * bytes at buckets + boff[i] (any alignment) are user i's stored bucket",
 * anything else a fresh bucket tokenbucket.New(max_tokens, reset_interval) at
 * that request's time.  A caller looks InternalStart ++ user up for all n
 * requests (duplicates are fine there) and hands the answers over unchanged:
 * only the entry of a user's first legal request is read; the others, and
 * boff where bstatus is not LIVE, are ignored.  A stored bucket brings its own
 * MaxTokens and ResetInterval (FromBytes), not the call's.  uoff, ulen, koff,
 * klen, ts and boff are 8-byte aligned.
 *
 * Outputs, by request (all but d_verdict nullable):
 *   d_verdict  n bytes at any address: NKV_ADMIT_ILLEGAL, _ALLOWED, _THROTTLED.
 *   d_bucket   32 n bytes, 8-byte aligned: the ToBytes image after the request;
 *              for an allowed one the Value of the bucket record the engine
 *              puts, for a throttled one the unchanged state, for an illegal
 *              one zeros.
 *   d_wait     n int64: the "seconds to go" a throttled request prints,
 *              ResetInterval - (now - Timestamp); 0 otherwise.
 *   d_group    n uint64: the arrival index of the first legal request of the
 *              same user, UINT64_MAX for an illegal one.  Its fixed points are
 *              the distinct users.
 *   d_last     n bytes at any address: 1 iff the request is its user's last
 *              legal one in the batch; its d_bucket entry is then the user's
 *              final state, what the next batch finds stored.
 * The answers are those of the n requests served one after the other.
 * Asynchronous on the context's stream; scratch comes from the context.
 *
 * NKV_ERR_INVALID, with nothing launched: a null context, req or start; n >
 * 2^31 - 1; start_len outside 1..64 (coreconf.validate refuses the empty
 * string); max_tokens or reset_interval outside 1..2^62 - 1; users NULL with
 * users_len > 0, and the same for keys; koff given without klen; buckets, boff
 * and bstatus not NULL together; with n > 0 a null uoff, ulen or d_verdict.
 * n = 0 returns NKV_OK and writes nothing.  Device-side verdicts go to d_err
 * (nullable, one uint32_t, need not be initialised; with d_err NULL the call
 * synchronizes and returns NKV_ERR_INVALID instead).  When the word is nonzero
 * no byte of any output has been written:
 *   bit 0  a user's or a key's span outside its blob (a wrapped off + len is
 *          caught);
 *   bit 1  a key shorter than start, where the reference indexes out of range;
 *   bit 2  a time that is negative, above 2^62 - 1, or smaller than the time of
 *          the request before it;
 *   bit 3  a stored bucket that is read and has MaxTokens or ResetInterval
 *          outside 1..2^62 - 1 or a Timestamp outside 0..2^62 - 1.  Tokens may
 *          be any int64, and a Timestamp may lie in the future.
 * Under NKV_TIMING_EVENTS the "leaf" interval is the validation, the grouping
 * and the sort, the "reduce" interval the windows, the ranks and the scatter. */
#define NKV_ADMIT_ILLEGAL 0
#define NKV_ADMIT_ALLOWED 1
#define NKV_ADMIT_THROTTLED 2
#define NKV_ADMIT_BAD_SPAN 1
#define NKV_ADMIT_BAD_KEY 2
#define NKV_ADMIT_BAD_TIME 4
#define NKV_ADMIT_BAD_BUCKET 8
typedef struct nkv_requests {  /* pointers on the context's device */
    const void *users;     uint64_t users_len; /* user i = users[uoff[i] .. uoff[i] + ulen[i]) */
    const uint64_t *uoff;  const uint64_t *ulen;
    const void *keys;      uint64_t keys_len;  /* key i  = keys[koff[i] .. koff[i] + klen[i]) */
    const uint64_t *koff;  const uint64_t *klen; /* koff NULL: no IsLegal step */
    const int64_t *ts;     /* n times, or NULL: ts_all for every request */
    int64_t ts_all;
    const void *buckets;   /* stored buckets: 32 bytes at buckets + boff[i] where bstatus[i] is NKV_GET_LIVE */
    const uint64_t *boff;  const uint8_t *bstatus;
    uint64_t n;
} nkv_requests;
int nkv_admit_dev(nkv_ctx *ctx, const nkv_requests *req, const void *start, uint64_t start_len,
                  int64_t max_tokens, int64_t reset_interval, uint8_t *d_verdict, void *d_bucket,
                  int64_t *d_wait, uint64_t *d_group, uint8_t *d_last, uint32_t *d_err);

/* ---- several tables per call (compaction's runs, consecutive flushes) ----
 * One table of device-resident leaves, described for nkv_trees_dev /
 * nkv_group_trees_dev (all pointers on the device that builds it). */
typedef enum nkv_table_kind {
    NKV_TABLE_STRIDED = 0, /* value i = base + i * stride, len bytes (nkv_tree_from_strided_dev) */
    NKV_TABLE_VALUES = 1,  /* value i = base + off[i], lens[i] bytes (nkv_tree_from_values_dev) */
    NKV_TABLE_RECORDS = 2, /* Data table: base = stream of base_len bytes, off = record offsets
                              (nkv_tree_from_records_dev; err nullable) */
    NKV_TABLE_VERIFY = 3   /* as RECORDS plus every record's Crc checked
                              (nkv_tree_verify_records_dev; crc, stats nullable) */
} nkv_table_kind;
typedef struct nkv_table {
    int kind;
    const void *base;
    uint64_t base_len;
    uint64_t stride, len;
    const uint64_t *off;
    const uint64_t *lens;
    uint64_t n;
    void *nodes; /* nkv_total_nodes(n) * 20 bytes */
    uint32_t *err;
    uint32_t *crc;
    uint64_t *stats;
} nkv_table;
/* The trees of k independent tables, asynchronous on the context's stream:
 * the tables are spread over NKV_OPT_TABLE_LANES streams of the context's
 * device (table t on lane t % lanes, forked from and joined back to the
 * context's stream), so one table's leaf kernel overlaps the tail and the tree
 * reduce of the one before.  Each table's results are those of its single-table
 * call.  A RECORDS table with err NULL: the call synchronizes and returns
 * NKV_ERR_INVALID if any of those tables has a header outside its stream. */
int nkv_trees_dev(nkv_ctx *ctx, const nkv_table *tables, int k);

/* ---- multi-GPU: one host process, one context per GPU ----
 * A group is one context per listed device and one RCCL communicator over
 * them (ncclCommInitAll).  Tables shard with no data-path exchange; the only
 * collective is the all-gather of 20-byte roots (an RCCL group call over the
 * members' streams).  Listing a device twice is allowed (several streams on
 * one GPU, e.g. to rehearse the split on one card): RCCL cannot join one
 * device twice, so such a group gathers by device-to-device copies instead
 * (nkv_group_transport). */
typedef struct nkv_group nkv_group;
#define NKV_TRANSPORT_RCCL 1
#define NKV_TRANSPORT_COPY 2
int nkv_group_create(const int *devices, int g, nkv_group **out);
void nkv_group_destroy(nkv_group *grp);
int nkv_group_size(const nkv_group *grp);
int nkv_group_transport(const nkv_group *grp);
/* Peer access between member i's GPU and member j's: nkv_group_create enables
 * xGMI peer mappings for every pair of distinct GPUs that supports them
 * (hipDeviceEnablePeerAccess; a pair already enabled counts), so GPU-to-GPU
 * copies (nkv_group_tree_fetch, the copy transport) go over xGMI.  *state:
 * NKV_PEER_ENABLED, NKV_PEER_SAME (both members on one GPU), or NKV_PEER_NONE
 * (not mappable: copies take the runtime's staged path). */
#define NKV_PEER_NONE 0
#define NKV_PEER_ENABLED 1
#define NKV_PEER_SAME 2
int nkv_group_peer_access(const nkv_group *grp, int i, int j, int *state);
/* member i's context (owned by the group): options, streams, *_dev calls */
int nkv_group_ctx(nkv_group *grp, int i, nkv_ctx **out);
int nkv_group_sync(nkv_group *grp);
/* d_roots[i]: 20 bytes on member i.  All-gather them: d_out[i] (nullable
 * array, or entries) receives the g * 20 bytes on member i (a d_roots or d_out
 * entry that is not device memory of member i's GPU: NKV_ERR_INVALID); roots_out
 * (nullable host buffer, g * 20 bytes) a copy (then the call synchronizes,
 * else it is asynchronous on the members' streams). */
int nkv_group_roots_allgather(nkv_group *grp, const void *const *d_roots, void *const *d_out,
                              uint8_t *roots_out);
/* Compaction over GPUs (lsmtree.go:71-128 merges runs; one output table per
 * GPU): table t is built on member t % g (its pointers live on that device,
 * nkv_trees_dev there), then every table's root is all-gathered so every member
 * holds all k roots in table order.  roots_out (host, k * 20 bytes, nullable):
 * then the call synchronizes; else asynchronous on the members' streams. */
int nkv_group_trees_dev(nkv_group *grp, const nkv_table *tables, int k, uint8_t *roots_out);
/* The same from host memory (cgo: what MakeTableSecondaries holds after a
 * merge): table t = values base[t] + off[t][i], len[t][i], on member t % g, one
 * host thread per member; outputs as nkv_tree_from_values (each nullable). */
typedef struct nkv_values {
    const uint8_t *base;
    const uint64_t *off;
    const uint64_t *len;
    uint64_t n;
    uint8_t *root20;
    uint8_t *nodes_out;
    uint8_t *img_out;
} nkv_values;
int nkv_group_trees_from_values(nkv_group *grp, const nkv_values *tables, int k);
/* One table over the group (a single compaction's output table, lsmtree.go:106-110):
 * padding only happens at a level's end (merkletree.go:32-34), so the tree splits
 * at 2^k-aligned leaf ranges: member r builds levels 0..k of leaves
 * [r * span, min(n, (r + 1) * span)), span = nkv_split_span(n, g) = 2^k, k =
 * max(1, ceil(log2(ceil(n / g)))); a partial last range re-hashes its lone top node
 * up to level k; the level-k nodes are all-gathered and every member reduces the
 * top ceil(log2 G) levels (G = ceil(n / span) ranges), so every member holds the
 * root.  Outputs as nkv_tree_from_values (each nullable; all host). */
uint64_t nkv_split_span(uint64_t n, int g);
int nkv_group_tree_from_values(nkv_group *grp, const uint8_t *base, const uint64_t *off, const uint64_t *len,
                               uint64_t n, uint8_t *root20, uint8_t *nodes_out, uint8_t *img_out);
/* The same over device-resident ranges: parts[r] describes member r's leaf range
 * (a STRIDED or VALUES table whose pointers live on member r's device, n = its
 * range's length, 0 for members past the last range; nodes ignored: the group
 * keeps the levels).  d_roots (nullable array of g entries, each nullable):
 * d_roots[r] is 20 bytes on member r's device that receive the root member r
 * reduced (every member's equals the root); root20 (host, nullable): then the
 * call synchronizes, else it is asynchronous on the members' streams.
 * nkv_group_tree_fetch then copies the latest such tree's nodes (level-major,
 * nkv_total_nodes(n) * 20 bytes) and/or its Serialize image to the host; after a
 * refused or failed split call there is no latest tree and it returns
 * NKV_ERR_INVALID. */
int nkv_group_tree_dev(nkv_group *grp, const nkv_table *parts, uint64_t n, void *const *d_roots,
                       uint8_t *root20);
int nkv_group_tree_fetch(nkv_group *grp, uint8_t *nodes_out, uint8_t *img_out);

#ifdef __cplusplus
}
#endif

#endif /* NKV_MERKLE_H */
