// small_host.cpp -- host side of the small path (small_tree.hip): the
// one-launch small tree of the host-buffer tree calls, its BAR-mapped input and
// the resident service's mailbox.  State: nkv_ctx::small (context.hpp SmallPath)
// and the ticket word of state.d_small.
//
// The reference engine's own flush and compaction sizes (coreconf.go:33-34,
// :39: 10-record memtables, 4 runs) hash a few KiB per call, where the grid
// path's copies and per-level launches cost far more than the work.  A batch
// of at most small.max_n values and small.max_bytes of (16-byte aligned)
// payload instead goes as ONE launch (k_small_tree): the values are packed into
// a host-coherent pinned buffer that the kernel reads across PCIe
// (NKV_OPT_SMALL_PATH 1) or that is copied to HBM first (2), the kernel writes
// nodes + image into a pinned output buffer (or HBM, then one copy back), and
// the call synchronizes once.
#include <hip/hip_runtime.h>
#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>

#include "context.hpp"

using namespace nkv;

namespace {

constexpr uint64_t kSmallMaxExtent = 0xFFFFFFF0ull;  // the kernel's 32-bit extent of in-place values
constexpr int64_t kSmallSpinUs = 2000;  // host spin on the completion word before the runtime's wait
constexpr uint64_t kSvcIdleUs = 20000;   // the resident service leaves after this long without a request
constexpr uint64_t kSvcLifeUs = 200000;  // ... or, between requests, once it has run this long
constexpr int64_t kSvcTimeoutUs = 10000000;  // a request unanswered this long (service alive) is an error

// A host-coherent pinned buffer of at least `bytes` (contents not kept): the
// small-tree kernel reads / writes it across PCIe, uncached on the GPU side.
int grow_coherent(uint8_t** p, size_t* cap, size_t bytes) {
    if (*cap >= bytes) return NKV_OK;
    if (*p) (void)hipHostFree(*p);
    *p = nullptr;
    *cap = 0;
    const size_t want = std::max(bytes, size_t(64) << 10);
    if (hipHostMalloc(reinterpret_cast<void**>(p), want, hipHostMallocCoherent) != hipSuccess) {
        (void)hipGetLastError();
        *p = nullptr;
        return NKV_ERR_NOMEM;
    }
    *cap = want;
    return NKV_OK;
}

// Device memory the host may store to directly: fine-grained memory of a
// large-BAR GPU is mapped into the host's address space at the address the GPU
// uses (tools/bar_probe.hip on MI355X: hostBaseAddress == the pointer, host
// stores and loads work, no grant needed).
bool host_mapped(const void* p) {
    hsa_amd_pointer_info_t info;
    memset(&info, 0, sizeof info);
    info.size = sizeof info;
    if (hsa_amd_pointer_info(p, &info, nullptr, nullptr, nullptr) != HSA_STATUS_SUCCESS) return false;
    return info.hostBaseAddress == p;
}

// Host stores to device memory through the BAR may be write-combined: drained
// before the doorbell (the request's bytes land first: PCIe keeps posted writes
// in order) and after it (so it leaves now, not when the buffer fills).
inline void store_fence() { asm volatile("sfence" ::: "memory"); }

// `bytes` of fine-grained device memory the host stores to, on a large-BAR GPU;
// nullptr where there is none.
void* bar_alloc(nkv_ctx* c, size_t bytes) {
    int large = 0;
    void* d = nullptr;
    const bool got = hipDeviceGetAttribute(&large, hipDeviceAttributeIsLargeBar, c->device) == hipSuccess && large &&
                     hipExtMallocWithFlags(&d, bytes, hipDeviceMallocFinegrained) == hipSuccess;
    if (got && !host_mapped(d)) {
        (void)hipFree(d);
        d = nullptr;
    }
    (void)hipGetLastError();
    return got ? d : nullptr;
}

// The service's mailbox, its input buffer and its stream (created on first
// use, and again after svc_stop).  The answer side (served, done, refused,
// stamps) is host-coherent memory, where the host spins.  The request side
// (doorbell, request line) and the service's input buffer go, with
// NKV_OPT_SERVICE_MAILBOX 0 on a large-BAR GPU, to fine-grained device memory
// the host stores to: the service then polls and reads local memory instead of
// crossing PCIe for each poll and for the input (tools/bar_probe.hip: a 4 KiB
// request's round trip 7.7 -> 5.8 us); otherwise they share the host mailbox.
int svc_buffers(nkv_ctx* c) {
    SmallPath& s = c->small;
    if (!s.h_mbox) {
        uint8_t* p = nullptr;
        size_t cap = 0;
        TRY(grow_coherent(&p, &cap, sizeof(SmallMailbox)));
        memset(p, 0, sizeof(SmallMailbox));
        s.h_mbox = reinterpret_cast<SmallMailbox*>(p);
        s.svc_box_dev = false;
        if (void* d = s.svc_mailbox == 0 ? bar_alloc(c, sizeof(SmallMailbox) + kSmallSeg) : nullptr) {
            memset(d, 0, sizeof(SmallMailbox));  // doorbell 0 == served 0
            store_fence();
            s.d_svc_box = static_cast<uint8_t*>(d);
            s.svc_box_dev = true;
        }
    }
    if (!s.h_svc_in) {
        size_t cap = 0;
        TRY(grow_coherent(&s.h_svc_in, &cap, kSmallSeg));
    }
    if (!s.svc) HIPTRY(hipStreamCreateWithFlags(&s.svc, hipStreamNonBlocking));
    return NKV_OK;
}

// The one-launch path's input buffer in device memory the host stores to
// (made once, on a large-BAR GPU with NKV_OPT_SERVICE_MAILBOX 0), or nullptr:
// a packed input of at most kSmallSeg bytes is copied there, so the kernel
// stages it from local memory instead of across PCIe.
uint8_t* small_input_bar(nkv_ctx* c) {
    SmallPath& s = c->small;
    if (s.svc_mailbox != 0) return nullptr;
    if (!s.d_sin_bar && !s.sin_bar_tried) {
        s.sin_bar_tried = true;
        s.d_sin_bar = static_cast<uint8_t*>(bar_alloc(c, kSmallSeg));
    }
    return s.d_sin_bar;
}

// The request side as the host stores to it (the device's address too).
SmallMailbox* svc_request_side(nkv_ctx* c) {
    return c->small.svc_box_dev ? reinterpret_cast<SmallMailbox*>(c->small.d_svc_box) : c->small.h_mbox;
}

// One request to the resident service: an inline request's packed input
// (descriptors + values at h_svc_in, in_bytes) moved to the device buffer when
// that is where the service reads it, the request line, then the doorbell
// (release: x86 keeps the stores in order; the fences drain a write-combined
// mapping; the service reads them after its system-scope acquire), then a
// spin on `done`.  Each 256 polls look at the service stream: a service that
// has left is started again.
int small_service_call(nkv_ctx* c, const uint64_t* d_desc, const uint8_t* d_vals, uint32_t vbytes, uint32_t n,
                       uint8_t* d_out, uint32_t img_at, uint32_t seq, bool inline_in) {
    TRY(svc_buffers(c));
    SmallPath& s = c->small;
    SmallMailbox* mb = s.h_mbox;
    SmallMailbox* rb = svc_request_side(c);
    void *dmb = nullptr, *din = nullptr;
    HIPTRY(hipHostGetDevicePointer(&dmb, mb, 0));
    const SmallMailbox* drb = s.svc_box_dev ? rb : static_cast<const SmallMailbox*>(dmb);
    if (s.svc_box_dev) {
        din = s.d_svc_box + sizeof(SmallMailbox);
        if (inline_in) {
            memcpy(din, s.h_svc_in, 16 * size_t(n) + vbytes);
            d_desc = static_cast<const uint64_t*>(din);
            d_vals = static_cast<const uint8_t*>(din) + 16 * size_t(n);
        }
    } else {
        HIPTRY(hipHostGetDevicePointer(&din, s.h_svc_in, 0));
    }
    const uint8_t* fixed_in = static_cast<const uint8_t*>(din);
    SmallRequest r;
    memset(&r, 0, sizeof r);
    r.n = n;
    r.vbytes = vbytes;
    r.img_at = img_at;
    r.trace = s.svc_trace ? 1u : 0u;
    r.desc = reinterpret_cast<uintptr_t>(d_desc);
    r.vals = reinterpret_cast<uintptr_t>(d_vals);
    r.out = reinterpret_cast<uintptr_t>(d_out);
    r.inline_in = inline_in ? 1u : 0u;
    memcpy(&rb->req, &r, sizeof r);
    if (s.svc_box_dev) store_fence();
    __atomic_store_n(&rb->doorbell, seq, __ATOMIC_RELEASE);
    if (s.svc_box_dev) store_fence();
    if (!s.svc_live) {
        HIPTRY(launch_small_service(static_cast<SmallMailbox*>(dmb), drb, fixed_in, kSvcIdleUs * 100, kSvcLifeUs * 100,
                                    s.svc));
        s.svc_live = true;
        ++s.svc_launches;
    }
    const auto t0 = std::chrono::steady_clock::now();
    const auto answered = [&] { return __atomic_load_n(&mb->done, __ATOMIC_ACQUIRE) == seq; };
    for (uint32_t k = 1; !answered(); ++k) {
        if ((k & 255u) == 0u) {
            const hipError_t q = hipStreamQuery(s.svc);
            if (q == hipSuccess) {  // the service has left (idle): start it again, unless it answered
                if (answered()) break;
                HIPTRY(launch_small_service(static_cast<SmallMailbox*>(dmb), drb, fixed_in, kSvcIdleUs * 100,
                                            kSvcLifeUs * 100, s.svc));
                ++s.svc_launches;
            } else if (q != hipErrorNotReady) {
                return st_at(q, "k_small_service", __FILE__, __LINE__);
            } else if (std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(kSvcTimeoutUs)) {
                return NKV_ERR_DEVICE;
            }
        }
        __builtin_ia32_pause();
    }
    return __atomic_load_n(&mb->refused, __ATOMIC_ACQUIRE) == seq ? NKV_ERR_DEVICE : NKV_OK;
}

// k_small_tree's last store is seq into the completion word, after every
// output byte: spin on it (a few us sooner than the runtime's completion
// wait); every 256 polls ask the stream whether it failed.  The spin is
// bounded (kSmallSpinUs): a kernel queued behind other work on a caller's
// stream is waited for by the runtime instead, so no host core spins for the
// length of someone else's queue.
int await_small_tree(nkv_ctx* c, volatile unsigned int* hdone, uint32_t seq) {
    const auto t_spin = std::chrono::steady_clock::now();
    const auto done = [&] { return __atomic_load_n(hdone, __ATOMIC_ACQUIRE) == seq; };
    for (uint32_t k = 1; !done(); ++k) {
        if ((k & 255u) == 0u) {
            const hipError_t q = hipStreamQuery(c->stream);
            if (q == hipSuccess) return done() ? NKV_OK : NKV_ERR_DEVICE;  // finished: the word is there now
            if (q != hipErrorNotReady) return st_at(q, "k_small_tree", __FILE__, __LINE__);
            if (std::chrono::steady_clock::now() - t_spin > std::chrono::microseconds(kSmallSpinUs)) {
                HIPTRY(hipStreamSynchronize(c->stream));
                return done() ? NKV_OK : NKV_ERR_DEVICE;
            }
        }
        __builtin_ia32_pause();
    }
    return NKV_OK;
}

}  // namespace

namespace nkv {

// Stop the resident service (nkv_ctx_destroy, a change of
// NKV_OPT_SERVICE_MAILBOX): the exit doorbell, then wait for the kernel to
// leave; its buffers are made again on the next request.
void svc_stop(nkv_ctx* c) {
    SmallPath& s = c->small;
    bool left = true;
    if (s.svc_live && s.h_mbox) {
        SmallMailbox* rb = svc_request_side(c);
        __atomic_store_n(&rb->doorbell, kSvcExit, __ATOMIC_RELEASE);
        if (s.svc_box_dev) store_fence();
        // the service leaves at its next poll (or its idle timeout); never wait
        // unboundedly in a destructor: a service that has not left after 2 s
        // keeps its mailbox and stream (leaked) rather than hang the caller
        const auto t0 = std::chrono::steady_clock::now();
        while (left && hipStreamQuery(s.svc) == hipErrorNotReady) {
            left = std::chrono::steady_clock::now() - t0 <= std::chrono::seconds(2);
            if (left) usleep(50);
        }
    }
    if (left) {
        if (s.svc) (void)hipStreamDestroy(s.svc);
        if (s.h_mbox) (void)hipHostFree(s.h_mbox);
        if (s.h_svc_in) (void)hipHostFree(s.h_svc_in);
        if (s.d_svc_box) (void)hipFree(s.d_svc_box);
    } else if (debug_on()) {
        fprintf(stderr, "nkv: the small-tree service did not leave; mailbox leaked\n");
    }
    s.svc_live = false;
    s.svc = nullptr;
    s.h_mbox = nullptr;
    s.h_svc_in = nullptr;
    s.d_svc_box = nullptr;
    s.svc_box_dev = false;
}

void small_free(nkv_ctx* c) {
    SmallPath& s = c->small;
    if (s.h_sin) (void)hipHostFree(s.h_sin);
    if (s.d_sin_bar) (void)hipFree(s.d_sin_bar);
    if (s.h_sout) (void)hipHostFree(s.h_sout);
    s.h_sin = s.h_sout = s.d_sin_bar = nullptr;
    s.h_sin_cap = s.h_sout_cap = 0;
}

int small_tree(nkv_ctx* c, const uint8_t* base, const uint64_t* off, const uint64_t* len, uint64_t n,
               uint8_t* root20, uint8_t* nodes_out, uint8_t* img_out, bool* taken) {
    SmallPath& s = c->small;
    *taken = false;
    if (s.path == 0 || n == 0 || n > s.max_n || n > kSmallMaxN) return NKV_OK;
    uint64_t vbytes = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (len[i] > s.max_bytes) return NKV_OK;
        vbytes += align16(len[i]);
        if (vbytes > s.max_bytes) return NKV_OK;
    }
    const uint64_t tot = total_of(n);
    const uint64_t img_len = layout_of(counts_of(n)).total;
    // img_at 0 tells the kernel to build no image: a caller that asked for none
    // (the mirrors' New, whose Serialize walks the live tree) pays none
    const uint64_t img_at = img_out ? align16(20 * tot) : 0;
    const uint64_t out_bytes = img_out ? img_at + align16(img_len) : align16(20 * tot);
    uint64_t lo = 0, hi = 0;
    nkv_ctx::Pinned* blk = pinned_extent(c, base, off, len, n, &lo, &hi);
    if (blk) blk->streamed = 0;  // a call over a pinned block ends its batch (nkv_host_stream)
    // values in a host-coherent arena block at 16-byte aligned places (the
    // mirrors' NewLeaf arena) are read where they lie: no pack, no copy
    // (only while their extent in the block, gaps included, stays within the
    // small bound: the kernel takes the extent as a 32-bit byte count)
    bool in_place = blk && blk->coherent && s.path != 2 && (lo & 15) == 0 &&
                    align16(hi) - lo <= std::min<uint64_t>(s.max_bytes, kSmallMaxExtent);
    const uint64_t adj = blk ? uint64_t(base - blk->p) : 0;
    for (uint64_t i = 0; in_place && i < n; ++i) in_place = ((adj + off[i]) & 15) == 0;
    // the resident service: a request whose descriptors and values fit its own
    // input buffer is packed there (a host copy of at most 16 KiB), so the
    // service reads it with the request line instead of one round trip later,
    // values in the arena included
    const bool svc = s.path == 3 && n <= kSvcMaxN;
    const bool svc_inline = svc && 16 * n + vbytes <= kSmallSeg;
    if (svc_inline) {
        in_place = false;
        TRY(svc_buffers(c));
    }
    // likewise the one-launch path (1): an input that fits 16 KiB is packed and
    // stored into BAR-mapped device memory (small_input_bar), arena values
    // included, rather than read across PCIe where it lies
    uint8_t* const bar = !svc && s.path == 1 && 16 * n + vbytes <= kSmallSeg ? small_input_bar(c) : nullptr;
    if (bar) in_place = false;
    const uint64_t vext = in_place ? align16(hi) - lo : vbytes;  // the values' extent
    const uint64_t in_bytes = 16 * n + (in_place ? 0 : vbytes);
    if (!svc_inline) TRY(grow_coherent(&s.h_sin, &s.h_sin_cap, in_bytes));
    uint8_t* const h_in = svc_inline ? s.h_svc_in : s.h_sin;
    TRY(grow_coherent(&s.h_sout, &s.h_sout_cap, out_bytes + 64));  // + the completion word
    DevBuf& d_small = c->state.d_small;
    const size_t small_cap = d_small.cap;
    TRY(grow(d_small, 64 + 20 * kSmallMaxN));
    if (d_small.cap != small_cap) HIPTRY(hipMemsetAsync(d_small.p, 0, 64, c->stream));  // the ticket
    uint64_t* desc = reinterpret_cast<uint64_t*>(h_in);
    if (in_place) {
        for (uint64_t i = 0; i < n; ++i) {
            desc[2 * i] = adj + off[i] - lo;
            desc[2 * i + 1] = len[i];
        }
    } else {
        uint8_t* vals = h_in + 16 * n;
        uint64_t p = 0;
        for (uint64_t i = 0; i < n; ++i) {
            desc[2 * i] = p;
            desc[2 * i + 1] = len[i];
            if (len[i]) memcpy(vals + p, base + off[i], len[i]);
            p += align16(len[i]);
        }
    }
    uint8_t* scratch = static_cast<uint8_t*>(d_small.p) + 64;
    unsigned int* ticket = static_cast<unsigned int*>(d_small.p);
    volatile unsigned int* hdone = reinterpret_cast<volatile unsigned int*>(s.h_sout + out_bytes);
    uint32_t seq = ++s.seq;
    if (seq == 0 || seq == kSvcExit) seq = s.seq = 1;  // 0 is the word's cleared state
    *hdone = 0;
    if (s.path == 2) {  // through HBM: one copy in, one launch, one copy out
        TRY(grow(s.d_sin, in_bytes));
        TRY(grow(s.d_sout, out_bytes));
        HIPTRY(hipMemcpyAsync(s.d_sin.p, s.h_sin, in_bytes, hipMemcpyHostToDevice, c->stream));
        const uint64_t* d_desc = static_cast<const uint64_t*>(s.d_sin.p);
        HIPTRY(launch_small_tree(d_desc, reinterpret_cast<const uint8_t*>(d_desc + 2 * n), uint32_t(vext),
                                 uint32_t(n), static_cast<uint8_t*>(s.d_sout.p), uint32_t(img_at), scratch, ticket,
                                 nullptr, 0, c->stream));
        HIPTRY(hipMemcpyAsync(s.h_sout, s.d_sout.p, out_bytes, hipMemcpyDeviceToHost, c->stream));
        HIPTRY(hipStreamSynchronize(c->stream));
    } else {  // the kernel or the service reads the values and writes its results across PCIe
        void *din = nullptr, *dout = nullptr, *dblk = nullptr;
        HIPTRY(hipHostGetDevicePointer(&din, h_in, 0));
        HIPTRY(hipHostGetDevicePointer(&dout, s.h_sout, 0));
        if (in_place) HIPTRY(hipHostGetDevicePointer(&dblk, blk->p, 0));
        const uint64_t* d_desc = static_cast<const uint64_t*>(din);
        const uint8_t* d_vals = in_place ? static_cast<const uint8_t*>(dblk) + lo
                                         : reinterpret_cast<const uint8_t*>(d_desc + 2 * n);
        if (svc) {  // the resident service: no launch, no runtime completion
            TRY(small_service_call(c, d_desc, d_vals, uint32_t(vext), uint32_t(n), static_cast<uint8_t*>(dout),
                                   uint32_t(img_at), seq, svc_inline));
        } else {
            // a packed input that fits the kernel's LDS stage goes to device memory
            // over the large BAR (posted writes: they land before the launch's
            // doorbell), so the kernel stages it without a PCIe read round trip
            if (bar) {
                memcpy(bar, s.h_sin, in_bytes);
                store_fence();
                d_desc = reinterpret_cast<const uint64_t*>(bar);
                d_vals = bar + 16 * n;
            }
            HIPTRY(launch_small_tree(d_desc, d_vals, uint32_t(vext), uint32_t(n), static_cast<uint8_t*>(dout),
                                     uint32_t(img_at), scratch, ticket,
                                     reinterpret_cast<unsigned int*>(static_cast<uint8_t*>(dout) + out_bytes), seq,
                                     c->stream));
            TRY(await_small_tree(c, hdone, seq));
        }
    }
    if (nodes_out) memcpy(nodes_out, s.h_sout, 20 * tot);
    if (root20) memcpy(root20, s.h_sout + 20 * (tot - 1), 20);
    if (img_out) memcpy(img_out, s.h_sout + img_at, img_len);
    c->last_path = NKV_PATH_SMALL;
    c->host_timed = false;
    *taken = true;
    return NKV_OK;
}

}  // namespace nkv

extern "C" {

int nkv_ctx_small_service_state(nkv_ctx* c, uint64_t out[8]) try {
    if (!c || !out) return NKV_ERR_INVALID;
    const SmallPath& s = c->small;
    for (int k = 0; k < 8; ++k) out[k] = 0;
    if (s.h_mbox) {
        out[0] = __atomic_load_n(&svc_request_side(c)->doorbell, __ATOMIC_ACQUIRE);
        out[6] = s.svc_box_dev ? 1u : 0u;
        out[7] = (uint64_t(__atomic_load_n(&s.h_mbox->xcc_id, __ATOMIC_ACQUIRE)) << 32) |
                 __atomic_load_n(&s.h_mbox->hw_id, __ATOMIC_ACQUIRE);
        out[1] = __atomic_load_n(&s.h_mbox->served, __ATOMIC_ACQUIRE);
        out[2] = __atomic_load_n(&s.h_mbox->done, __ATOMIC_ACQUIRE);
    }
    out[3] = s.svc_launches;
    out[4] = s.svc_live ? 1u : 0u;
    if (s.svc) {
        TRY(bind(c));
        out[5] = hipStreamQuery(s.svc) == hipErrorNotReady ? 1u : 0u;
    }
    return NKV_OK;
} NKV_CATCH

int nkv_ctx_small_service_trace(nkv_ctx* c, int enable, uint64_t out[14]) try {
    if (!c || enable < 0 || enable > 1) return NKV_ERR_INVALID;
    if (out) {
        for (int k = 0; k < kSvcStamps; ++k)
            out[k] = c->small.h_mbox ? __atomic_load_n(&c->small.h_mbox->stamps[k], __ATOMIC_ACQUIRE) : 0u;
    }
    c->small.svc_trace = enable != 0;
    return NKV_OK;
} NKV_CATCH

}  // extern "C"
