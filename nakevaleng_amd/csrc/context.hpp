// context.hpp -- the nkv_ctx definition and the host helpers shared by the
// C-ABI translation units: context.cpp (context services), stage.cpp (staging
// of host inputs), tree.cpp (leaf planning, tree entries), small_host.cpp (the
// small path), group.cpp (the multi-GPU group and the multi-table entries) and
// the *.hip units, each of which keeps its entries beside its kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <new>
#include <vector>

#include "host_stage.hpp"
#include "internal.hpp"
#include "nkv_merkle.h"

namespace nkv {

// ---------------------------------------------------------------------------
// tree shape (merkletree.go:31-64): n_0 = n, n_{L+1} = ceil(n_L / 2), until a
// level of one node that is not the leaf level.

inline int levels_of(uint64_t n) {
    if (n == 0) return 0;
    int lv = 1;
    uint64_t c = n;
    do {
        c = (c + 1) / 2;
        ++lv;
    } while (c > 1);
    return lv;
}

inline uint64_t count_of(uint64_t n, int L) { return L == 0 ? n : ((n - 1) >> L) + 1; }

inline uint64_t start_of(uint64_t n, int L) {
    uint64_t s = 0;
    for (int j = 0; j < L; ++j) s += count_of(n, j);
    return s;
}

inline uint64_t total_of(uint64_t n) { return start_of(n, levels_of(n)); }

// Image layout (merkletree.go:67-92) of levels given bottom-up counts[0..nlev)
// of 20-byte nodes stored level-major from node index 0: top level first, 21
// bytes per node, one 0x01 pad byte after every odd level below the top.
inline BfsLayout layout_of(const std::vector<uint64_t>& counts) {
    BfsLayout lay{};
    const int nlev = int(counts.size());
    lay.nlev = nlev;
    std::vector<uint64_t> start(nlev);
    uint64_t s = 0;
    for (int L = 0; L < nlev; ++L) {
        start[L] = s;
        s += counts[L];
    }
    uint64_t p = 0;
    for (int i = 0; i < nlev; ++i) {  // image order: top first
        const int L = nlev - 1 - i;
        lay.img_start[i] = p;
        lay.node_start[i] = start[L];
        lay.count[i] = counts[L];
        p += 21 * counts[L];
        if (L < nlev - 1 && (counts[L] & 1)) p += 1;
    }
    lay.total = p;
    return lay;
}

inline std::vector<uint64_t> counts_of(uint64_t n) {
    std::vector<uint64_t> c(levels_of(n));
    for (size_t L = 0; L < c.size(); ++L) c[L] = count_of(n, int(L));
    return c;
}

// ---------------------------------------------------------------------------
// status helpers

inline int st(hipError_t e) {
    if (e == hipSuccess) return NKV_OK;
    if (e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation) return NKV_ERR_NOMEM;
    return NKV_ERR_DEVICE;
}

// NKV_DEBUG=1 in the environment: every failing HIP call behind HIPTRY is
// named on stderr (the status code alone does not say which call failed)
inline bool debug_on() {
    static const bool on = [] {
        const char* e = getenv("NKV_DEBUG");
        return e && *e && *e != '0';
    }();
    return on;
}
inline int st_at(hipError_t e, const char* what, const char* file, int line) {
    if (e != hipSuccess && debug_on())
        fprintf(stderr, "nkv: %s:%d: %s -> %s\n", file, line, what, hipGetErrorString(e));
    return st(e);
}

#define TRY(x)                         \
    do {                               \
        int _rc = (x);                 \
        if (_rc != NKV_OK) return _rc; \
    } while (0)
#define HIPTRY(x) TRY(::nkv::st_at((x), #x, __FILE__, __LINE__))
// Every C-ABI entry is a function-try-block: a host allocation or thread start
// that throws inside the library becomes a status code, never an exception
// crossing the C boundary (cgo / ctypes callers cannot catch it).
#define NKV_CATCH                      \
    catch (const std::bad_alloc&) {    \
        return NKV_ERR_NOMEM;          \
    }                                  \
    catch (...) {                      \
        return NKV_ERR_DEVICE;         \
    }

// Largest batch: leaf indices are 32-bit in the sort and queue kernels
// (2^31 - 1 values of 4 KiB would be 8 TiB, far beyond one GPU's HBM).
constexpr uint64_t kMaxN = 0x7fffffffull;

inline uint64_t align16(uint64_t x) { return (x + 15) & ~uint64_t(15); }

// A device buffer that frees itself: nothing else calls hipFree on one.
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }  // for std::vector<DevBuf>
    ~DevBuf() { release(); }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr, cap = 0;
    }
};

// Grow a device buffer (contents are not kept).
int grow(DevBuf& b, size_t bytes);

// Bump-pointer carver of a scratch buffer.  An entry names its arrays in one
// sequence of take() calls and runs it twice: over no buffer, where bytes()
// is what grow() receives, and over the grown buffer, where the same calls
// hand out the pointers -- the size and the pointers cannot disagree.
struct Carver {
    uint8_t* base = nullptr;  // nullptr: measuring
    uint64_t at = 0;
    explicit Carver(void* p = nullptr) : base(static_cast<uint8_t*>(p)) {}
    // count elements of T at the next multiple of align
    template <class T>
    T* take(uint64_t count, uint64_t align = alignof(T)) {
        at = (at + align - 1) & ~(align - 1);
        T* p = base ? reinterpret_cast<T*>(base + at) : nullptr;
        at += count * sizeof(T);
        return p;
    }
    uint64_t bytes() const { return at; }
};

// ---------------------------------------------------------------------------
// small_host.cpp: the one-launch small-tree path of the host-buffer tree calls
// and its resident service.  Everything the path owns on a context:

struct SmallPath {
    int path = 1;                 // NKV_OPT_SMALL_PATH
    uint64_t max_n = 1024;        // NKV_OPT_SMALL_MAX_N
    uint64_t max_bytes = uint64_t(1) << 20;  // NKV_OPT_SMALL_MAX_BYTES
    // host-coherent pinned in / out buffers the kernel reads and writes across
    // PCIe, or (path 2) device copies of them
    uint8_t* h_sin = nullptr;
    uint8_t* h_sout = nullptr;
    size_t h_sin_cap = 0, h_sout_cap = 0;
    DevBuf d_sin, d_sout;
    uint32_t seq = 0;  // the kernel's completion word (per call)
    // the packed input in fine-grained device memory the host stores to
    // (kSmallSeg bytes; NKV_OPT_SERVICE_MAILBOX 0 on a large-BAR GPU)
    uint8_t* d_sin_bar = nullptr;
    bool sin_bar_tried = false;
    // path 3: the resident service's mailbox and stream (created on first use;
    // the kernel leaves when idle, at svc_stop or at nkv_ctx_destroy)
    SmallMailbox* h_mbox = nullptr;
    uint8_t* h_svc_in = nullptr;  // host packing buffer of an inline request (kSmallSeg bytes, host-coherent)
    // NKV_OPT_SERVICE_MAILBOX 0 on a large-BAR GPU: the request side (doorbell,
    // request line) and the service's input buffer in fine-grained device memory
    // the host stores to directly (one block: the mailbox, then kSmallSeg bytes)
    uint8_t* d_svc_box = nullptr;
    int svc_mailbox = 0;       // NKV_OPT_SERVICE_MAILBOX
    bool svc_box_dev = false;  // the live buffers are d_svc_box's (else h_mbox / h_svc_in)
    hipStream_t svc = nullptr;
    bool svc_live = false;   // a service launch was made and may still run
    bool svc_trace = false;  // nkv_ctx_small_service_trace: stamp each request's phases
    uint64_t svc_launches = 0;
};

}  // namespace nkv

// ---------------------------------------------------------------------------
// context

struct nkv_ctx {
    int device = 0;
    hipStream_t own = nullptr;
    hipStream_t stream = nullptr;
    int leaf_load = 4;  // NKV_OPT_LEAF_LOAD
    int bucket = 2;     // NKV_OPT_BUCKET
    uint32_t simds = 1024;  // SIMDs on the device (CUs x 4)
    int queue_split = 32;   // NKV_OPT_QUEUE_SPLIT
    int queue_waves = 3;    // NKV_OPT_QUEUE_WAVES
    int bloom_path = 2;     // NKV_OPT_BLOOM_PATH
    int sketch_path = 0;    // NKV_OPT_SKETCH_PATH
    int frame_path = 0;     // NKV_OPT_FRAME_PATH
    uint64_t frame_budget = 0;  // NKV_OPT_FRAME_BUDGET (0 = auto)
    int index_open_path = 0;   // NKV_OPT_INDEX_OPEN_PATH
    int index_open_chunk = 0;  // NKV_OPT_INDEX_OPEN_CHUNK (0 = the default)
    int crc_load = 0;       // NKV_OPT_CRC_LOAD
    int records_fused = 1;  // NKV_OPT_RECORDS_FUSED
    int table_lanes = 2;    // NKV_OPT_TABLE_LANES
    bool timing = false;
    bool timed = false;
    // NKV_OPT_TIMING_EVERY: the tree calls record their events on every k-th
    // call only (counted from nkv_ctx_set_timing); sampled: the current call
    int timing_every = 1;
    uint64_t timing_calls = 0;
    bool sampled = true;
    // per-call event triples (leaf start, leaf end / reduce start, reduce end),
    // the latest kTimingRing / 3 calls
    static constexpr size_t kTimingRing = 3 * 65536;
    std::vector<hipEvent_t> ring;
    size_t ring_used = 0;
    hipEvent_t host_ev[2] = {nullptr, nullptr};  // host-buffer call: before the upload, after the download
    bool host_timed = false;
    // State buffers: each carries an invariant from one call on the context to
    // the next (the stream orders the calls).  No entry uses one as scratch.
    struct State {
        // both pass-flag sets (internal.hpp kPassFlagWords) are reset except while a records
        // call runs: nkv_ctx_create fills them; k_leaf_records / k_leaf_verify reset the set the next call takes
        nkv::DevBuf d_flags;
        // k_len_range's ticket word is zero between launches: zeroed when allocated (plan_of);
        // the launch's last workgroup puts it back
        nkv::DevBuf d_ticket;
        // the length sort's bucket totals and ticket (its first sort_head_words() words) are zero between
        // sorts: zeroed when (re)allocated or sort_dirty (leaf_level); k_len_scatter_alloc's last workgroup restores them
        nkv::DevBuf d_keys;
        // word 0, k_small_tree's ticket, is zero between launches: zeroed when allocated
        // (small_tree); the kernel's last workgroup puts it back.  From byte 64 on: that kernel's scratch
        nkv::DevBuf d_small;
        // the clock probe's sums run from nkv_ctx_set_timing (which zeroes them) to nkv_ctx_clock:
        // the leaf kernels add into them while clock_probe is set
        nkv::DevBuf d_clk;
    } state;
    // Free scratch: any entry may take any of these for any use; the contents
    // never outlive a call.  The staging layer (stage.cpp) fills d_data, d_off /
    // d_len, d_aux and d_rec_off; d_nodes and d_img hold what goes back to the host.
    nkv::DevBuf d_data, d_off, d_len, d_aux, d_rec_off, d_nodes, d_img, d_tmp, d_err, d_stats, d_range, d_part, d_perm,
        d_queue, d_stmp, d_frame;
    int flag_set = 0;  // which of the two pass-flag sets in state.d_flags the next records call uses
    // the length sort's bucket totals may be non-zero (a sort was cut short):
    // the next sort clears them first (internal.hpp sort_head_words)
    bool sort_dirty = false;
    void* h_stage = nullptr;  // small pinned staging (offsets, lengths, stats)
    unsigned int* h_small = nullptr;  // 64 pinned bytes for device-to-host decisions
    size_t h_cap = 0;
    nkv::Stager stage;  // pipelined pinned staging of bulk bytes (host_stage.hpp)
    // stream hand-over (nkv_ctx_set_stream): the new stream waits for the old
    hipEvent_t switch_ev = nullptr;
    // multi-table entries (nkv_trees_dev): sub-contexts of the same device with
    // their own streams, forked from and joined to this context's stream
    std::vector<nkv_ctx*> lanes;
    hipEvent_t fork_ev = nullptr;
    std::vector<hipEvent_t> join_ev;
    bool clock_probe = false;  // NKV_TIMING_CLOCK: leaf kernels add their waves' clocks into state.d_clk
    // pinned blocks from nkv_host_alloc (the deferred-NewLeaf arena): calls whose
    // values lie inside one are copied straight from it (no staging gather), and
    // nkv_host_stream copies a block's settled prefix ahead of the call
    struct Pinned {
        uint8_t* p;
        uint64_t bytes;
        uint64_t streamed;  // bytes [0, streamed) already queued to d_arena
        nkv::DevBuf d_arena;  // device mirror of the block
        bool coherent;        // host-coherent (the small-tree kernel may read it in place)
    };
    std::vector<Pinned*> pinned;
    int arena_coherent = 1;  // NKV_OPT_ARENA_COHERENT: nkv_host_alloc blocks host-coherent
    // NKV_OPT_SIDE_GATE: the gated plan's input-order kernel on a second stream
    // (created on first use), forked after the range and joined before the levels
    int side_gate = 1;
    hipStream_t side = nullptr;
    hipEvent_t side_ev[2] = {nullptr, nullptr};
    nkv::SmallPath small;  // the one-launch small-tree path and its resident service (NKV_OPT_SMALL_*)
    int last_path = 0;     // NKV_PATH_* of the latest host-buffer tree call or frame call
};

namespace nkv {

// ---- context.cpp: context services ----
int bind(nkv_ctx* c);
int grow_host(nkv_ctx* c, size_t bytes);
// Record events around the leaf kernel and the reduce (which = 0, 1, 2).
int mark(nkv_ctx* c, int which);
// Events bracketing a host-buffer call (which = 0 before the upload, 1 after the download).
int host_mark(nkv_ctx* c, int which);
// The pinned block (nkv_host_alloc on this context) that holds every value
// base + off[i] .. + len[i], or null; *lo / *hi: the values' extent relative
// to the block.
nkv_ctx::Pinned* pinned_extent(nkv_ctx* c, const uint8_t* base, const uint64_t* off, const uint64_t* len, uint64_t n,
                               uint64_t* lo, uint64_t* hi);
// Queue bytes [from, to) of a pinned block to its device mirror on the context's stream.
int stream_block(nkv_ctx* c, nkv_ctx::Pinned* blk, uint64_t from, uint64_t to);

// ---- stage.cpp: host-pointer entries' inputs to the device, results back ----
// Pack n host values into d_data at 16-byte aligned offsets and upload their
// offsets/lengths to d_off / d_len (or use the device mirror of the pinned
// block they lie in).  *d_base / *aligned: where the kernels read the values.
int stage_values(nkv_ctx* c, const uint8_t* base, const uint64_t* off, const uint64_t* len, uint64_t n,
                 const uint8_t** d_base, bool* aligned);
// n host spans base + off[i], len[i] as they lie: the bytes up to the last
// span's end to d_data, off / len to d_off / d_len.
int stage_spans(nkv_ctx* c, const uint8_t* base, const uint64_t* off, const uint64_t* len, uint64_t n);
// A host stream of n records: NKV_ERR_INVALID unless the sizes fit it
// (records_fit); the bytes to d_data and the sizes to d_aux through the
// pipelined stager; *rec_off: the records' offsets, made on the device
// (nkv_record_offsets_dev) in d_rec_off.
int stage_records(nkv_ctx* c, const uint8_t* stream, uint64_t stream_len, const uint64_t* rec_size, uint64_t n,
                  const uint64_t** rec_off);
// The n sizes fit the stream (their sum <= stream_len) / add up to it exactly;
// term by term, so a wrapped sum cannot pass.
bool records_fit(const uint64_t* rec_size, uint64_t n, uint64_t stream_len);
bool records_fill(const uint64_t* rec_size, uint64_t n, uint64_t stream_len);
// A host stream and its n record sizes to d_stream / d_size, and the records'
// offsets made on the device into d_off (nkv_record_offsets_dev).
int upload_records(nkv_ctx* c, const uint8_t* stream, uint64_t stream_len, const uint64_t* rec_size, uint64_t n,
                   void* d_stream, uint64_t* d_size, uint64_t* d_off);
// A written table of n records and len bytes to the host (synchronizes):
// its bytes to out, and its offsets d_off as sizes to out_rec_size.
int download_table(nkv_ctx* c, const void* d_table, uint64_t len, const uint64_t* d_off, uint64_t n, uint8_t* out,
                   uint64_t* out_rec_size);
// The verdict of a validating kernel: the error word to the host and the
// stream synchronized; NKV_ERR_INVALID if the word is set.
int read_verdict(nkv_ctx* c, const unsigned int* d_err);
// The error word of an entry with a nullable d_err: the caller's, or the first
// word of d_stats; cleared on the stream.  d_stats is grown to 8 bytes at most
// and grow() never shrinks or moves a buffer that is large enough, so an entry
// that keeps more words behind this one sizes d_stats for all of them first
// and its pointers stay good.
int verdict_word(nkv_ctx* c, uint32_t* d_err, unsigned int** err);
// The end of such an entry: d_err given, NKV_OK (the caller reads the word);
// otherwise read_verdict over the word verdict_word handed out.
int finish_verdict(nkv_ctx* c, const uint32_t* d_err, const unsigned int* err);

// ---- tree.cpp: leaf planning and the tree entries' shared steps ----
// Level 0 in the plan NKV_OPT_BUCKET picks (host_len: the lengths on the host, nullable)
int leaf_level(nkv_ctx* c, const uint8_t* base, const uint64_t* off, const uint64_t* len, uint64_t n,
               bool aligned, uint8_t* nodes, const uint64_t* host_len);
int tree_from_device_values(nkv_ctx* c, const uint8_t* base, const uint64_t* off, const uint64_t* len,
                            uint64_t n, bool aligned, uint8_t* nodes, const uint64_t* host_len = nullptr,
                            const unsigned int* dev_range = nullptr);
// After a tree call: image / nodes / root to the host (any nullable), then a sync.
int finish_tree(nkv_ctx* c, uint8_t* nodes, uint64_t n, uint8_t* root20, uint8_t* nodes_out, uint8_t* img_out);

// ---- small_host.cpp (SmallPath above) ----
// The host-buffer tree of a small batch in one launch or one service request;
// *taken = false: not eligible, nothing done.
int small_tree(nkv_ctx* c, const uint8_t* base, const uint64_t* off, const uint64_t* len, uint64_t n,
               uint8_t* root20, uint8_t* nodes_out, uint8_t* img_out, bool* taken);
// Stop the resident service and release its mailbox, buffers and stream (made
// again on the next request).
void svc_stop(nkv_ctx* c);
// nkv_ctx_destroy, after svc_stop: the path's pinned and BAR buffers.
void small_free(nkv_ctx* c);

}  // namespace nkv
