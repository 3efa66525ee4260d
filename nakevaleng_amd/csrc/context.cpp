// context.cpp -- the context and its services: lifetime, options, streams,
// timing, the pinned arena, buffer growth, and the entries that belong to no
// path (build id, shapes, nkv_write_file, nkv_fill_splitmix64_dev).
//
// There is deliberately no CPU compute path in the library: every digest is
// produced by the gfx950 kernels in the *.hip units.  A missing/unusable device
// is reported as NKV_ERR_DEVICE.
#include <fcntl.h>
#include <hip/hip_runtime.h>
#include <unistd.h>

#include <algorithm>
#include <new>
#include <vector>

#include "context.hpp"

using namespace nkv;

namespace nkv {

int bind(nkv_ctx* c) {
    if (!c) return NKV_ERR_INVALID;
    return st(hipSetDevice(c->device));
}

int grow(DevBuf& b, size_t bytes) {
    if (bytes == 0) bytes = 16;
    if (b.cap >= bytes) return NKV_OK;
    const size_t old = b.cap;
    b.release();
    size_t want = std::max(bytes, old + old / 2);
    if (hipMalloc(&b.p, want) != hipSuccess) {
        (void)hipGetLastError();
        if (hipMalloc(&b.p, bytes) != hipSuccess) {
            (void)hipGetLastError();
            b.p = nullptr;
            return NKV_ERR_NOMEM;
        }
        want = bytes;
    }
    b.cap = want;
    return NKV_OK;
}

int grow_host(nkv_ctx* c, size_t bytes) {
    if (bytes == 0) bytes = 16;
    if (c->h_cap >= bytes) return NKV_OK;
    if (c->h_stage) (void)hipHostFree(c->h_stage);
    c->h_stage = nullptr;
    c->h_cap = 0;
    if (hipHostMalloc(&c->h_stage, bytes, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        c->h_stage = nullptr;
        return NKV_ERR_NOMEM;
    }
    c->h_cap = bytes;
    return NKV_OK;
}

nkv_ctx::Pinned* pinned_extent(nkv_ctx* c, const uint8_t* base, const uint64_t* off, const uint64_t* len,
                               uint64_t n, uint64_t* lo, uint64_t* hi) {
    if (c->pinned.empty() || n == 0) return nullptr;
    uint64_t a = ~uint64_t(0), b = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (len[i] > (uint64_t(1) << 62) || off[i] > (uint64_t(1) << 62)) return nullptr;
        a = std::min(a, off[i]);
        b = std::max(b, off[i] + len[i]);
    }
    const uintptr_t s = reinterpret_cast<uintptr_t>(base) + a, e = reinterpret_cast<uintptr_t>(base) + b;
    if (e < s) return nullptr;
    for (nkv_ctx::Pinned* blk : c->pinned) {
        const uintptr_t p = reinterpret_cast<uintptr_t>(blk->p);
        if (s >= p && e <= p + blk->bytes) {
            *lo = s - p;
            *hi = e - p;
            return blk;
        }
    }
    return nullptr;
}

// The block is library-owned memory, so the DMA may outlive the call.
int stream_block(nkv_ctx* c, nkv_ctx::Pinned* blk, uint64_t from, uint64_t to) {
    if (to <= from) return NKV_OK;
    if (!blk->d_arena.p) TRY(grow(blk->d_arena, blk->bytes));
    HIPTRY(hipMemcpyAsync(static_cast<uint8_t*>(blk->d_arena.p) + from, blk->p + from, to - from,
                          hipMemcpyHostToDevice, c->stream));
    return NKV_OK;
}

// Events around the leaf kernel and the reduce of one tree call; kept per
// call (no host sync) so a timed loop can be summarised afterwards.
int mark(nkv_ctx* c, int which) {
    if (!c->timing) return NKV_OK;
    if (which == 0) c->sampled = c->timing_calls++ % uint64_t(c->timing_every) == 0;
    if (!c->sampled) return NKV_OK;
    if (which == 0) {
        if (c->ring_used + 3 > nkv_ctx::kTimingRing) c->ring_used = 0;  // restart the window
        if (c->ring_used + 3 > c->ring.size()) {
            for (int i = 0; i < 3; ++i) {
                hipEvent_t e;
                HIPTRY(hipEventCreateWithFlags(&e, hipEventDisableSystemFence));  // timing only: no cache writeback per record
                c->ring.push_back(e);
            }
        }
        c->ring_used += 3;
    }
    // one event per mark: each record is a timestamp packet on the stream
    // (a few us of GPU time), so the timed loop carries three per tree
    HIPTRY(hipEventRecord(c->ring[c->ring_used - 3 + which], c->stream));
    if (which == 2) c->timed = true;
    return NKV_OK;
}

// Events around a host-buffer tree call (which = 0 before the upload, 1 after
// the outputs are back): with the three mark() events of the same call they
// split it into upload, kernels and download (nkv_ctx_last_host_timing).
int host_mark(nkv_ctx* c, int which) {
    if (!c->timing) return NKV_OK;
    // which 0 comes before the call's mark(0): the call is sampled when the
    // count it is about to take is
    const bool sampled = which == 0 ? c->timing_calls % uint64_t(c->timing_every) == 0 : c->sampled;
    if (!sampled) {
        c->host_timed = false;
        return NKV_OK;
    }
    if (!c->host_ev[which]) HIPTRY(hipEventCreate(&c->host_ev[which]));
    HIPTRY(hipEventRecord(c->host_ev[which], c->stream));
    if (which == 1) c->host_timed = c->timed;
    return NKV_OK;
}

}  // namespace nkv

#ifndef NKV_SRC_HASH
#define NKV_SRC_HASH "unknown"
#endif

extern "C" {

const char* nkv_build_id(void) { return "nkv-src-sha256:" NKV_SRC_HASH; }

int nkv_abi_version(void) { return NKV_ABI_VERSION; }

const char* nkv_strerror(int s) {
    switch (s) {
        case NKV_OK: return "ok";
        case NKV_ERR_EMPTY: return "cannot build Merkle Tree from 0 nodes";
        case NKV_ERR_INVALID: return "invalid argument";
        case NKV_ERR_DEVICE: return "HIP device error";
        case NKV_ERR_NOMEM: return "out of memory";
        case NKV_ERR_IO: return "file I/O error";
        default: return "unknown error";
    }
}

int nkv_device_count(int* count) try {
    if (!count) return NKV_ERR_INVALID;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        *count = 0;
        return NKV_ERR_DEVICE;
    }
    *count = n;
    return NKV_OK;
} NKV_CATCH

int nkv_ctx_create(int device, nkv_ctx** out) try {
    if (!out) return NKV_ERR_INVALID;
    *out = nullptr;
    int cnt = 0;
    if (nkv_device_count(&cnt) != NKV_OK || device < 0 || device >= cnt) return NKV_ERR_DEVICE;
    nkv_ctx* c = new nkv_ctx();
    c->device = device;
    int rc = st(hipSetDevice(device));
    if (rc == NKV_OK) rc = st(hipStreamCreateWithFlags(&c->own, hipStreamNonBlocking));
    if (rc == NKV_OK) rc = st(hipHostMalloc(reinterpret_cast<void**>(&c->h_small), 64, hipHostMallocDefault));
    if (rc == NKV_OK) rc = grow(c->state.d_flags, 4 * 2 * kPassFlagWords);
    if (rc == NKV_OK) {  // both pass-flag sets start reset (each records call resets the other)
        uint32_t init[2 * kPassFlagWords] = {};
        for (uint32_t k = 0; k < 2; ++k) init[kPassFlagWords * k + 6] = init[kPassFlagWords * k + 7] = ~0u;
        rc = st(hipMemcpy(c->state.d_flags.p, init, sizeof(init), hipMemcpyHostToDevice));
    }
    if (rc != NKV_OK) {
        nkv_ctx_destroy(c);
        return rc;
    }
    c->stream = c->own;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
        c->simds = uint32_t(prop.multiProcessorCount) * 4;
    *out = c;
    return NKV_OK;
} NKV_CATCH

// Order: nothing may still run when its memory goes.  The device buffers free
// themselves (DevBuf) when the context is deleted, after everything else.
void nkv_ctx_destroy(nkv_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->own) (void)hipStreamSynchronize(c->own);
    svc_stop(c);  // the resident small-tree service leaves before anything it reads is freed
    if (c->clock_probe) (void)set_clock_probe(nullptr, c->own);  // kernels must not add into freed memory
    for (nkv_ctx* l : c->lanes) nkv_ctx_destroy(l);
    (void)hipSetDevice(c->device);
    for (nkv_ctx::Pinned* blk : c->pinned) {
        (void)hipHostFree(blk->p);
        delete blk;
    }
    if (c->h_stage) (void)hipHostFree(c->h_stage);
    if (c->h_small) (void)hipHostFree(c->h_small);
    small_free(c);
    for (hipEvent_t e : c->ring) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->join_ev) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->host_ev)
        if (e) (void)hipEventDestroy(e);
    if (c->fork_ev) (void)hipEventDestroy(c->fork_ev);
    if (c->side) (void)hipStreamSynchronize(c->side);
    for (hipEvent_t e : c->side_ev)
        if (e) (void)hipEventDestroy(e);
    if (c->side) (void)hipStreamDestroy(c->side);
    if (c->switch_ev) (void)hipEventDestroy(c->switch_ev);
    if (c->own) (void)hipStreamDestroy(c->own);
    delete c;
}

// Stream hand-over: work already queued on the old stream (an asynchronous
// *_dev call) is ordered before anything the context queues on the new one --
// the state buffers (context.hpp) carry state from one call to the next on a
// context.
static int switch_stream(nkv_ctx* c, hipStream_t s) {
    if (s == c->stream) return NKV_OK;
    if (!c->switch_ev) HIPTRY(hipEventCreateWithFlags(&c->switch_ev, hipEventDisableTiming));
    HIPTRY(hipEventRecord(c->switch_ev, c->stream));
    HIPTRY(hipStreamWaitEvent(s, c->switch_ev, 0));
    c->stream = s;
    return NKV_OK;
}

int nkv_ctx_set_stream(nkv_ctx* c, void* s) try {
    TRY(bind(c));
    return switch_stream(c, static_cast<hipStream_t>(s));  // NULL = the device's null stream
} NKV_CATCH

int nkv_ctx_use_own_stream(nkv_ctx* c) try {
    TRY(bind(c));
    return switch_stream(c, c->own);
} NKV_CATCH

int nkv_ctx_set_option(nkv_ctx* c, int key, int64_t value) try {
    TRY(bind(c));
    struct Ranged {  // an option that is an int in [lo, hi]
        int* at;
        int64_t lo, hi;
    };
    const Ranged r = [&]() -> Ranged {
        switch (key) {
            case NKV_OPT_BUCKET: return {&c->bucket, 0, 2};
            case NKV_OPT_BLOOM_PATH: return {&c->bloom_path, 0, 2};
            case NKV_OPT_SKETCH_PATH: return {&c->sketch_path, 0, 2};
            case NKV_OPT_FRAME_PATH: return {&c->frame_path, 0, 2};
            case NKV_OPT_INDEX_OPEN_PATH: return {&c->index_open_path, 0, 2};
            case NKV_OPT_HOST_THREADS: return {&c->stage.want_threads, 0, 256};
            case NKV_OPT_RECORDS_FUSED: return {&c->records_fused, 0, 1};
            case NKV_OPT_QUEUE_WAVES: return {&c->queue_waves, 1, 3};  // 12 KiB ring per wave: <= 13 per CU
            case NKV_OPT_TABLE_LANES: return {&c->table_lanes, 1, 8};
            case NKV_OPT_SMALL_PATH: return {&c->small.path, 0, 3};
            case NKV_OPT_ARENA_COHERENT: return {&c->arena_coherent, 0, 1};
            case NKV_OPT_SIDE_GATE: return {&c->side_gate, 0, 1};
            default: return {nullptr, 0, 0};
        }
    }();
    if (r.at) {
        if (value < r.lo || value > r.hi) return NKV_ERR_INVALID;
        *r.at = int(value);
        return NKV_OK;
    }
    switch (key) {
        case NKV_OPT_LEAF_LOAD:
            if (value != 4 && value != 11) return NKV_ERR_INVALID;
            c->leaf_load = int(value);
            return NKV_OK;
        case NKV_OPT_QUEUE_SPLIT:
            if (value < 0 || value > 0xFFFFFFFFll) return NKV_ERR_INVALID;
            c->queue_split = int(std::min<int64_t>(value, 0x7FFFFFFF));
            return NKV_OK;
        case NKV_OPT_CRC_LOAD:
            if (value != 0 && value != 8) return NKV_ERR_INVALID;
            c->crc_load = int(value);
            return NKV_OK;
        case NKV_OPT_FRAME_BUDGET:
            if (value < 0) return NKV_ERR_INVALID;
            c->frame_budget = uint64_t(value);
            return NKV_OK;
        case NKV_OPT_INDEX_OPEN_CHUNK:
            if (value != 0 && (value < 16 || value > (int64_t(1) << 24) || (value & 15))) return NKV_ERR_INVALID;
            c->index_open_chunk = int(value);
            return NKV_OK;
        case NKV_OPT_STAGE_CHUNK:
            if (value < 4096 || value > (int64_t(1) << 32) || (value & 4095)) return NKV_ERR_INVALID;
            if (c->stage.drain() != hipSuccess) return NKV_ERR_DEVICE;
            c->stage.chunk = size_t(value);
            return NKV_OK;
        case NKV_OPT_TIMING_EVERY:
            if (value < 1 || value > 1000000) return NKV_ERR_INVALID;
            c->timing_every = int(value);
            c->timing_calls = 0;
            return NKV_OK;
        case NKV_OPT_SMALL_MAX_N:
            if (value < 0 || value > int64_t(kSmallMaxN)) return NKV_ERR_INVALID;
            c->small.max_n = uint64_t(value);
            return NKV_OK;
        case NKV_OPT_SERVICE_MAILBOX:
            if (value < 0 || value > 1) return NKV_ERR_INVALID;
            if (int(value) != c->small.svc_mailbox) {
                TRY(bind(c));
                svc_stop(c);  // the next request makes the buffers in the new place
                c->small.svc_mailbox = int(value);
            }
            return NKV_OK;
        case NKV_OPT_QUEUE_PAIR:  // retired: one wave per group (the pair kernel failed its GPU parity run)
            return value == 0 ? NKV_OK : NKV_ERR_INVALID;
        case NKV_OPT_SMALL_MAX_BYTES:
            if (value < 0 || value > (int64_t(1) << 30)) return NKV_ERR_INVALID;
            c->small.max_bytes = uint64_t(value);
            return NKV_OK;
        case NKV_OPT_DEEP_PREFETCH:  // retired: the one path left (ABI version 1)
            return value == 3 ? NKV_OK : NKV_ERR_INVALID;
        case NKV_OPT_QUEUE_RING:  // retired: the 3-slot ring (ABI version 1)
            return value == 13 ? NKV_OK : NKV_ERR_INVALID;
        default:
            return NKV_ERR_INVALID;
    }
} NKV_CATCH

int nkv_ctx_last_path(nkv_ctx* c, int* path) try {
    if (!c || !path) return NKV_ERR_INVALID;
    *path = c->last_path;
    return NKV_OK;
} NKV_CATCH

int nkv_ctx_sync(nkv_ctx* c) try {
    TRY(bind(c));
    return st(hipStreamSynchronize(c->stream));
} NKV_CATCH

// ---- timing ----
int nkv_ctx_set_timing(nkv_ctx* c, int enable) try {
    TRY(bind(c));
    if (enable & ~(NKV_TIMING_EVENTS | NKV_TIMING_CLOCK)) return NKV_ERR_INVALID;
    c->timing = (enable & NKV_TIMING_EVENTS) != 0;
    c->timed = false;
    c->ring_used = 0;
    c->timing_calls = 0;
    for (nkv_ctx* l : c->lanes) {
        l->timing = c->timing;
        l->timed = false;
        l->ring_used = 0;
        l->timing_calls = 0;
    }
    DevBuf& d_clk = c->state.d_clk;
    if (enable & NKV_TIMING_CLOCK) {
        TRY(grow(d_clk, kClockWords * sizeof(unsigned long long)));
        HIPTRY(hipMemsetAsync(d_clk.p, 0, kClockWords * sizeof(unsigned long long), c->stream));
        HIPTRY(set_clock_probe(static_cast<unsigned long long*>(d_clk.p), c->stream));
        c->clock_probe = true;
    } else if (c->clock_probe) {
        HIPTRY(set_clock_probe(nullptr, c->stream));
        c->clock_probe = false;
    }
    return NKV_OK;
} NKV_CATCH

int nkv_ctx_clock(nkv_ctx* c, double* mhz, uint64_t* waves) try {
    TRY(bind(c));
    if (!mhz || !waves) return NKV_ERR_INVALID;
    if (!c->state.d_clk.p) return NKV_ERR_INVALID;
    std::vector<unsigned long long> h(kClockWords);
    HIPTRY(hipStreamSynchronize(c->stream));
    for (nkv_ctx* l : c->lanes) HIPTRY(hipStreamSynchronize(l->stream));
    HIPTRY(hipMemcpy(h.data(), c->state.d_clk.p, kClockWords * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    // per slot: [0] shader-clock cycles, [1] 100 MHz reference ticks, summed over waves; [2] waves
    double cyc = 0, ticks = 0;
    uint64_t w = 0;
    for (uint32_t s = 0; s < kClockWords; s += 32) {
        cyc += double(h[s]);
        ticks += double(h[s + 1]);
        w += h[s + 2];
    }
    *mhz = ticks > 0 ? 100.0 * cyc / ticks : 0.0;
    *waves = w;
    return NKV_OK;
} NKV_CATCH

static int timing_sum(nkv_ctx* c, int* calls, double* a, double* b) {
    const size_t k = c->ring_used / 3;
    if (k) HIPTRY(hipEventSynchronize(c->ring[c->ring_used - 1]));
    for (size_t i = 0; i < k; ++i) {
        float x = 0.f, y = 0.f;
        HIPTRY(hipEventElapsedTime(&x, c->ring[3 * i], c->ring[3 * i + 1]));
        HIPTRY(hipEventElapsedTime(&y, c->ring[3 * i + 1], c->ring[3 * i + 2]));
        *a += x;
        *b += y;
    }
    *calls += int(k);
    return NKV_OK;
}

int nkv_ctx_timing_summary(nkv_ctx* c, int* calls, float* leaf_ms_total, float* reduce_ms_total) try {
    TRY(bind(c));
    if (!calls || !leaf_ms_total || !reduce_ms_total) return NKV_ERR_INVALID;
    int k = 0;
    double a = 0, b = 0;
    TRY(timing_sum(c, &k, &a, &b));
    for (nkv_ctx* l : c->lanes) TRY(timing_sum(l, &k, &a, &b));  // nkv_trees_dev's lanes
    *calls = k;
    *leaf_ms_total = float(a);
    *reduce_ms_total = float(b);
    return NKV_OK;
} NKV_CATCH

int nkv_ctx_last_host_timing(nkv_ctx* c, float* upload_ms, float* kernels_ms, float* download_ms) try {
    TRY(bind(c));
    if (!c->host_timed || !c->timed) return NKV_ERR_INVALID;
    hipEvent_t* ev = &c->ring[c->ring_used - 3];
    HIPTRY(hipEventSynchronize(c->host_ev[1]));
    float a = 0.f, b = 0.f, d = 0.f;
    HIPTRY(hipEventElapsedTime(&a, c->host_ev[0], ev[0]));
    HIPTRY(hipEventElapsedTime(&b, ev[0], ev[2]));
    HIPTRY(hipEventElapsedTime(&d, ev[2], c->host_ev[1]));
    if (upload_ms) *upload_ms = a;
    if (kernels_ms) *kernels_ms = b;
    if (download_ms) *download_ms = d;
    return NKV_OK;
} NKV_CATCH

int nkv_ctx_last_timing(nkv_ctx* c, float* leaf_ms, float* reduce_ms) try {
    TRY(bind(c));
    if (!c->timed) return NKV_ERR_INVALID;
    hipEvent_t* ev = &c->ring[c->ring_used - 3];
    HIPTRY(hipEventSynchronize(ev[2]));
    float a = 0.f, b = 0.f;
    HIPTRY(hipEventElapsedTime(&a, ev[0], ev[1]));
    HIPTRY(hipEventElapsedTime(&b, ev[1], ev[2]));
    if (leaf_ms) *leaf_ms = a;
    if (reduce_ms) *reduce_ms = b;
    return NKV_OK;
} NKV_CATCH

// ---- shape ----
int nkv_num_levels(uint64_t n) { return levels_of(n); }
uint64_t nkv_level_count(uint64_t n, int L) {
    return (n == 0 || L < 0 || L >= levels_of(n)) ? 0 : count_of(n, L);
}
uint64_t nkv_level_start(uint64_t n, int L) {
    return (n == 0 || L < 0 || L >= levels_of(n)) ? 0 : start_of(n, L);
}
uint64_t nkv_total_nodes(uint64_t n) { return total_of(n); }
uint64_t nkv_bfs_size(uint64_t n) { return n == 0 ? 0 : layout_of(counts_of(n)).total; }

// ---- pinned arena ----
constexpr uint64_t kEagerMirrorBytes = uint64_t(64) << 20;
int nkv_host_alloc(nkv_ctx* c, uint64_t bytes, void** out) try {
    if (!out) return NKV_ERR_INVALID;
    *out = nullptr;
    TRY(bind(c));
    void* p = nullptr;
    // host-coherent by default (NKV_OPT_ARENA_COHERENT): DMA reads it as any
    // pinned block, and the small-tree kernel may read it in place (uncached on
    // the GPU side, so a block rewritten flush after flush is never stale there)
    const unsigned flags = c->arena_coherent ? hipHostMallocCoherent : hipHostMallocDefault;
    if (hipHostMalloc(&p, bytes ? bytes : 1, flags) != hipSuccess) {
        (void)hipGetLastError();
        return NKV_ERR_NOMEM;
    }
    nkv_ctx::Pinned* blk = new (std::nothrow)
        nkv_ctx::Pinned{static_cast<uint8_t*>(p), bytes ? bytes : 1, 0, {}, c->arena_coherent != 0};
    if (!blk) {
        (void)hipHostFree(p);
        return NKV_ERR_NOMEM;
    }
    // a large block's device mirror now, not inside the first flush that
    // streams into it (an arena reserved at engine start costs a flush
    // nothing); small blocks, and any block whose mirror does not fit the HBM
    // free right now, get theirs on first use (stream_block): a caller whose
    // values only ever take the small path never needs it
    if (blk->bytes >= kEagerMirrorBytes && grow(blk->d_arena, blk->bytes) != NKV_OK) (void)hipGetLastError();
    c->pinned.push_back(blk);
    *out = p;
    return NKV_OK;
} NKV_CATCH

int nkv_host_free(nkv_ctx* c, void* p) try {
    TRY(bind(c));
    if (!p) return NKV_OK;
    for (size_t i = 0; i < c->pinned.size(); ++i) {
        nkv_ctx::Pinned* blk = c->pinned[i];
        if (blk->p != p) continue;
        // copies from the block (nkv_host_stream, a tree call) may still be queued
        HIPTRY(hipStreamSynchronize(c->stream));
        c->pinned.erase(c->pinned.begin() + long(i));
        delete blk;  // its device mirror with it
        break;
    }
    return st(hipHostFree(p));
} NKV_CATCH

int nkv_host_stream(nkv_ctx* c, const void* block, uint64_t upto) try {
    TRY(bind(c));
    if (!block) return NKV_ERR_INVALID;
    for (nkv_ctx::Pinned* blk : c->pinned) {
        if (blk->p != block) continue;
        if (upto > blk->bytes) return NKV_ERR_INVALID;
        if (upto < blk->streamed) blk->streamed = 0;  // a new batch: its bytes replace the old ones
        TRY(stream_block(c, blk, blk->streamed, upto));
        blk->streamed = std::max(blk->streamed, upto);
        return NKV_OK;
    }
    return NKV_ERR_INVALID;  // not a block nkv_host_alloc returned on this context
} NKV_CATCH

// ---- entries of no path ----
int nkv_write_file(const char* fname, const uint8_t* data, uint64_t len) try {
    if (!fname || (!data && len)) return NKV_ERR_INVALID;
    int fd = open(fname, O_WRONLY | O_CREAT, 0666);  // no O_TRUNC: merkletree.go:68
    if (fd < 0) return NKV_ERR_IO;
    // one sequential write (positioned writes from several threads measured no
    // faster: buffered writes to one file serialise on its inode lock)
    uint64_t done = 0;
    while (done < len) {
        ssize_t w = write(fd, data + done, size_t(std::min<uint64_t>(len - done, 1ull << 30)));
        if (w <= 0) {
            close(fd);
            return NKV_ERR_IO;
        }
        done += uint64_t(w);
    }
    return close(fd) == 0 ? NKV_OK : NKV_ERR_IO;
} NKV_CATCH

int nkv_fill_splitmix64_dev(nkv_ctx* c, void* d_buf, uint64_t nbytes, uint64_t seed) try {
    TRY(bind(c));
    if (nbytes == 0) return NKV_OK;
    if (!d_buf) return NKV_ERR_INVALID;
    return st(launch_fill(static_cast<uint8_t*>(d_buf), nbytes, seed, c->stream));
} NKV_CATCH

}  // extern "C"
