// small_tree.hip -- a whole small tree in one launch, and the resident service
// that serves one without a launch, on gfx950.
//
//   Ks  k_small_tree    a whole small tree (n <= 1024) and its image in one launch.
//       k_small_service the same from a mailbox, by one resident workgroup.
//
// The value loop's pieces are sha1_feed_dev.hpp's, the digests' storage
// tree_dev.hpp's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "internal.hpp"
#include "nkv_merkle.h"
#include "sha1_dev.hpp"
#include "sha1_feed_dev.hpp"
#include "tree_dev.hpp"

namespace nkv {

#ifdef NKV_DIAG
__device__ unsigned long long* g_diag = nullptr;  // NKV_STAMP (internal.hpp)
hipError_t set_diag_small(unsigned long long* p) { return hipMemcpyToSymbol(HIP_SYMBOL(g_diag), &p, sizeof(p)); }
#endif

// ---------------------------------------------------------------------------
// Ks: a whole small tree in ONE launch -- the sizes the reference engine runs at
// by default (coreconf.go:33-34: a flush of MEMTABLE_CAPACITY = 10 records;
// :39: a compaction of lsm_run_max = 4 such runs), where a launch per level
// and copies per buffer would cost more than the hashing.
//
// Input: n (offset, length) u64 pairs at desc and the values at vals + offset
// (16-byte aligned).  The host packs both into host-coherent pinned memory that
// the kernel reads across PCIe (no DMA), or copies them to HBM first
// (NKV_OPT_SMALL_PATH); values already in a host-coherent pinned arena block
// (the deferred-NewLeaf arena, nkv_host_alloc) are read where they lie.  One lane per leaf and one
// 256-lane workgroup per 256 leaves, so each wave runs alone on its SIMD (a
// leaf's SHA-1 is a serial chain: DESIGN.md section 4, lone-wave cadence); the
// last workgroup to finish (a ticket) takes every leaf digest, builds all levels
// (merkletree.go:31-64) and the Serialize image (merkletree.go:67-92,
// merklenode.go:37-63) in LDS, and stores nodes (level-major, 20 B each) at out
// and the image at out + img_at with 16-byte stores.  LDS: every node (at most
// 2 x 1024 - 1) plus one 16 KiB image segment, under the 64 KiB a workgroup
// gets without opting in.

constexpr uint32_t kSmallBlock = 256;

// SHA-1 of p[0, len), p 16-byte aligned, one block of register lookahead,
// with every lane of the wave issuing every compression.  A wave runs its VALU work up to 35 % slower on some CUs when fewer than ~48 of
// its lanes are active than with all of them (one clock, same instructions:
// tools/svc_shape.hip, profiles/r06_svc_shape_lanes.txt -- 10 active lanes take
// 11.2-15.1 us by CU for what 48 or 64 lanes do in 11.0 us on every CU), and a
// small tree's waves have few values.  So the full-block loop runs to the
// wave's largest block count (a lane past its own blocks compresses its stale
// block into a copy it drops) and the padding blocks run in every lane; a lane
// with no value (len 0) hashes the empty value, which its caller drops.  The
// caller calls it with every lane of the wave active.
__device__ __forceinline__ void sha1_value_all_lanes(const uint8_t* p, uint32_t len, uint32_t h[5]) {
    sha1_init(h);
    const uint32_t nfull = len >> 6;
    uint32_t most = nfull;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) most = max(most, uint32_t(__shfl_xor(int(most), o)));
    most = uint32_t(__builtin_amdgcn_readfirstlane(int(most)));  // wave-uniform trip count
    const uint4* q = reinterpret_cast<const uint4*>(p);
    uint4 cur[4], nxt[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        cur[k] = nfull ? q[k] : make_uint4(0u, 0u, 0u, 0u);
        nxt[k] = make_uint4(0u, 0u, 0u, 0u);
    }
    for (uint32_t b = 0; b < most; ++b) {
        if (b + 1 < nfull) {
#pragma unroll
            for (int k = 0; k < 4; ++k) nxt[k] = q[4 * (b + 1) + k];
        }
        uint32_t w[16], t[5];
        be16_from_raw(cur, w);
#pragma unroll
        for (int i = 0; i < 5; ++i) t[i] = h[i];
        sha1_compress(t, w);
        const bool mine = b < nfull;
#pragma unroll
        for (int i = 0; i < 5; ++i) h[i] = mine ? t[i] : h[i];
#pragma unroll
        for (int k = 0; k < 4; ++k) cur[k] = nxt[k];
    }
    sha1_tail<true>(p, len, h);
}

// bytes [0, bytes) of LDS src to dst (16-byte aligned both), 16 per store;
// B = the workgroup's threads
template <uint32_t B>
__device__ __forceinline__ void small_copy_out(const uint8_t* src, uint8_t* dst, uint32_t bytes) {
    const uint32_t whole = bytes & ~15u;
    for (uint32_t b = 16 * threadIdx.x; b < whole; b += 16 * B)
        *reinterpret_cast<uint4*>(dst + b) = *reinterpret_cast<const uint4*>(src + b);
    for (uint32_t b = whole + threadIdx.x; b < bytes; b += B) dst[b] = src[b];
}

__device__ __forceinline__ uint32_t small_count(uint32_t n, int L) { return L == 0 ? n : ((n - 1) >> L) + 1; }

// bytes [0, bytes) of src (16-byte aligned, host or device memory) into LDS
// dst: every thread's loads are issued before any store, so an input of up to
// 16 KiB crosses PCIe in one round trip
template <uint32_t B>
__device__ __forceinline__ void small_stage_in(const uint8_t* src, uint8_t* dst, uint32_t bytes) {
    const uint4* s4 = reinterpret_cast<const uint4*>(src);
    uint4* d4 = reinterpret_cast<uint4*>(dst);
    const uint32_t nq = (bytes + 15u) >> 4;
    for (uint32_t c0 = 0; c0 < nq; c0 += 4 * B) {
        uint4 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t c = c0 + threadIdx.x + k * B;
            v[k] = c < nq ? s4[c] : make_uint4(0u, 0u, 0u, 0u);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t c = c0 + threadIdx.x + k * B;
            if (c < nq) d4[c] = v[k];
        }
    }
}

// Every level above the leaf digests in sm (at least one; a lone last node is
// hashed alone, its sibling being the empty pad: merkletree.go:31-64), the
// nodes stored level-major at out, then the Serialize image at out + img_at,
// top level first: 0x00 + digest per node, one 0x01 after each odd level below
// the top (merklenode.go:37-63, MERKLE_NODE_EMPTY :11), built kSmallSeg bytes
// at a time in seg from whole node records clipped to the segment (as
// k_bfs_image does); img_at 0: no image.  Starts at a workgroup barrier.
template <uint32_t B>
__device__ __forceinline__ void small_levels_and_image(uint8_t* sm, uint8_t* seg, uint32_t n, uint8_t* out,
                                                       uint32_t img_at, uint64_t* trace = nullptr) {
    const uint32_t tid = threadIdx.x;
    // diagnostics (the service's traced requests): (s_memrealtime, s_memtime)
    // into trace[2k], trace[2k + 1] by thread 0
    auto mark = [&](int k) {
        if (trace && tid == 0) {
            __hip_atomic_store(trace + 2 * k, __builtin_amdgcn_s_memrealtime(), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_store(trace + 2 * k + 1, __builtin_amdgcn_s_memtime(), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_SYSTEM);
        }
    };
    __syncthreads();
    uint32_t cnt = n, base = 0;
    int lv = 1;
    do {
        const uint32_t pc = (cnt + 1) >> 1;
        // every lane of a wave that has a parent to build takes part (a lane
        // past the level's end rebuilds the last parent and drops it): a wave
        // with few active lanes computes slower on some CUs (sha1_value_all_lanes)
        for (uint32_t j0 = 0; j0 < pc; j0 += B) {
            const uint32_t j = j0 + tid;
            if ((j & ~63u) < pc) {
                const uint32_t jj = min(j, pc - 1u);
                const bool lone = 2 * jj + 1 >= cnt;
                uint32_t l[5], r[5] = {0u, 0u, 0u, 0u, 0u}, o[5];
                load_digest(sm, base + 2 * jj, l);
                if (!lone) load_digest(sm, base + 2 * jj + 1, r);
                sha1_parent(l, r, lone, o);
                if (j < pc) store_digest(sm, base + cnt + j, o);
            }
        }
        __syncthreads();
        base += cnt;
        cnt = pc;
        ++lv;
    } while (cnt > 1);
    NKV_STAMP(3);
    mark(0);
    const uint32_t total = base + 1;
    if (img_at == 0u) {  // the caller asked for no image (the nodes start at out + 0)
        small_copy_out<B>(sm, out, 20u * total);
        return;
    }
    uint32_t img_len = 0;
    for (int L = lv - 1; L >= 0; --L) {
        const uint32_t c = small_count(n, L);
        img_len += 21u * c + ((L < lv - 1 && (c & 1u)) ? 1u : 0u);
    }
    // (seg's staged input was last read before the first level's barrier)
    // The nodes leave with the first image segment, after it is built.
    // Every node record of the image is built by its own thread at once (all
    // levels together): the thread finds its record's level from the top,
    // loads the 20-byte digest as five LDS words and stores the 21 bytes, so
    // no LDS load waits inside a byte loop (per-level, byte-by-byte copying
    // cost 6 us for a 10-leaf tree, more than its four tree levels).
    for (uint32_t s0 = 0; s0 < img_len; s0 += kSmallSeg) {
        const uint32_t s1 = min(s0 + kSmallSeg, img_len);
        for (uint32_t r = tid; r < total; r += B) {
            uint32_t A = 0, before = 0;  // image offset of level L's first record; records above it
            int L = lv - 1;
            uint32_t c = small_count(n, L);
            while (r >= before + c) {
                A += 21u * c + ((L < lv - 1 && (c & 1u)) ? 1u : 0u);
                before += c;
                --L;
                c = small_count(n, L);
            }
            const uint32_t k = r - before;
            uint32_t ns = 0;  // node index of level L's first node (levels stored bottom-up)
            for (int jl = 0; jl < L; ++jl) ns += small_count(n, jl);
            const uint32_t* d = reinterpret_cast<const uint32_t*>(sm + 20u * (ns + k));
            uint32_t w[5];
#pragma unroll
            for (int q = 0; q < 5; ++q) w[q] = d[q];
            const int32_t pos = int32_t(A + 21u * k) - int32_t(s0);
            if (pos >= 0 && pos + 21 <= int32_t(s1 - s0)) {
                seg[pos] = 0u;
#pragma unroll
                for (int b = 0; b < 20; ++b) seg[pos + 1 + b] = uint8_t(w[b >> 2] >> (8 * (b & 3)));
            } else if (pos + 21 > 0 && pos < int32_t(s1 - s0)) {  // a record across a segment edge
#pragma unroll
                for (int b = 0; b < 21; ++b) {
                    const int32_t qb = pos + b;
                    if (qb >= 0 && qb < int32_t(s1 - s0)) seg[qb] = b == 0 ? 0u : uint8_t(w[(b - 1) >> 2] >> (8 * ((b - 1) & 3)));
                }
            }
        }
        // the pads: one 0x01 after each odd level below the top, by thread L
        if (tid + 1 < uint32_t(lv)) {
            const int L = int(tid);
            uint32_t A = 0;
            for (int Lu = lv - 1; Lu > L; --Lu) {
                const uint32_t cu = small_count(n, Lu);
                A += 21u * cu + ((Lu < lv - 1 && (cu & 1u)) ? 1u : 0u);
            }
            const uint32_t c = small_count(n, L);
            const uint32_t E = A + 21u * c;
            if ((c & 1u) && E >= s0 && E < s1) seg[E - s0] = NKV_MERKLE_NODE_EMPTY;
        }
        __syncthreads();
        if (s0 == 0) {
            mark(1);
            small_copy_out<B>(sm, out, 20u * total);
        }
        small_copy_out<B>(seg, out + img_at + s0, s1 - s0);
        if (s1 < img_len) __syncthreads();  // seg is rebuilt for the next segment
    }
}

// seq into the host-coherent completion word once every output byte of the
// workgroup is written at system scope.  One release for the workgroup, not one
// per wave (the guide's producer form: every storing wave waits for its own
// stores, a barrier, then ONE lane's release fence -- a single L2 write-back --
// its wait, and the flag); a fence in every wave cost each wave an L2
// write-back (16 of them in the service's first, 1024-thread form).
__device__ __forceinline__ void small_signal_done(unsigned int* done, uint32_t seq) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's output stores have completed
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");  // system scope
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the write-back before the flag (guide: compiler hazard)
        __hip_atomic_store(done, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// vbytes: the extent of vals the values lie in.  A one-workgroup launch whose
// descriptors and values fit kSmallSeg bytes stages both into LDS first (one
// PCIe round trip for the whole input instead of one per block of each lane).
// done (nullable, host-coherent): receives seq once every output byte is
// written, so the host can spin on it instead of waiting for the runtime's
// completion signal.
__global__ __launch_bounds__(kSmallBlock) void k_small_tree(const uint64_t* __restrict__ desc,
                                                            const uint8_t* __restrict__ vals, uint32_t vbytes,
                                                            uint32_t n, uint8_t* __restrict__ out, uint32_t img_at,
                                                            uint8_t* __restrict__ scratch,
                                                            unsigned int* __restrict__ ticket,
                                                            unsigned int* __restrict__ done, uint32_t seq) {
    __shared__ __attribute__((aligned(16))) uint8_t sm[20 * (2 * kSmallMaxN - 1) + 12];  // every node
    __shared__ __attribute__((aligned(16))) uint8_t seg[kSmallSeg];  // the staged input, then image segments
    __shared__ uint32_t is_last;
    const uint32_t tid = threadIdx.x;
    const uint32_t i = blockIdx.x * kSmallBlock + tid;
    NKV_STAMP(0);
    // the input may lie in fine-grained device memory the host stored to
    // (NKV_OPT_SERVICE_MAILBOX 0): no stale L2 line of an earlier call's input
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
    if (gridDim.x == 1 && 16u * n + vbytes <= kSmallSeg) {
        small_stage_in<kSmallBlock>(reinterpret_cast<const uint8_t*>(desc), seg, 16u * n);
        small_stage_in<kSmallBlock>(vals, seg + 16u * n, vbytes);
        __syncthreads();
        desc = reinterpret_cast<const uint64_t*>(seg);
        vals = seg + 16u * n;
    }
    NKV_STAMP(1);
    uint32_t h[5] = {0u, 0u, 0u, 0u, 0u};
    if ((i & ~63u) < n) {  // every lane of a wave with a value (sha1_value_all_lanes)
        const bool real = i < n;
        sha1_value_all_lanes(real ? vals + desc[2 * i] : vals, real ? uint32_t(desc[2 * i + 1]) : 0u,
                             h);  // NewLeaf, merklenode.go:27-34
    }
    NKV_STAMP(2);
    if (gridDim.x > 1) {
        if (i < n) store_digest(scratch, i, h);
        __threadfence();
        __syncthreads();
        if (tid == 0) is_last = atomicAdd(ticket, 1u) == gridDim.x - 1 ? 1u : 0u;
        __syncthreads();
        if (!is_last) return;
        __threadfence();
        if (tid == 0) atomicExch(ticket, 0u);  // the next launch counts from 0
        for (uint32_t j = tid; j < n; j += kSmallBlock) {
            const uint32_t* s = reinterpret_cast<const uint32_t*>(scratch + 20u * j);
            uint32_t* d = reinterpret_cast<uint32_t*>(sm + 20u * j);
#pragma unroll
            for (int k = 0; k < 5; ++k) d[k] = __atomic_load_n(s + k, __ATOMIC_RELAXED);
        }
    } else if (i < n) {
        store_digest(sm, i, h);
    }
    small_levels_and_image<kSmallBlock>(sm, seg, n, out, img_at);
    if (done) small_signal_done(done, seq);
}

// The resident small-tree service (NKV_OPT_SMALL_PATH 3): ONE workgroup of
// kSvcBlock threads stays on the GPU between calls and serves one request of at
// most kSvcMaxN leaves at a time from a mailbox, so a default-size flush pays neither a
// launch nor the runtime's completion path ("The
// small-flush floor").  The request side (rb: doorbell, request line; fixed_in:
// the service's own input buffer) lies in device memory the host stores to
// directly on a large-BAR GPU, else in host-coherent memory with the rest of
// the mailbox (rb == mb; NKV_OPT_SERVICE_MAILBOX); the answer side (mb: served,
// done, refused, stamps) is always host-coherent, where the host spins on it.
// Wave 0 polls the doorbell (relaxed
// system-scope loads, s_sleep between polls); a new seq is acquired at system
// scope, the request (the same descriptors, values and output layout
// k_small_tree takes) is served exactly as k_small_tree serves a one-workgroup
// launch -- leaves one lane each, every level and the image in LDS -- and seq
// goes to mb->done behind every output byte.  Every wave leaves when the
// doorbell reads kSvcExit (nkv_ctx_destroy), after idle_ticks of the 100 MHz
// real-time counter with no request, or between requests once it has lived
// life_ticks (the host relaunches on its next call), so the grid always drains
// and work queued behind it on a shared hardware queue waits a bounded time.
// s_getreg_b32 operands: HW_REG_HW_ID (id 4: wave, SIMD, CU, SH, SE ...) and
// HW_REG_XCC_ID (id 20, bits [3:0]), whole registers
constexpr int kHwRegHwId = 4 | (0 << 6) | (31 << 11);
constexpr int kHwRegXccId = 20 | (0 << 6) | (15 << 11);

template <uint32_t B>
__global__ __launch_bounds__(B) void k_small_service(SmallMailbox* __restrict__ mb, const SmallMailbox* rb,
                                                     const uint8_t* __restrict__ fixed_in, uint64_t idle_ticks,
                                                     uint64_t life_ticks) {
    __shared__ __attribute__((aligned(16))) uint8_t sm[20 * (2 * kSvcMaxN - 1) + 12];
    __shared__ __attribute__((aligned(16))) uint8_t seg[kSmallSeg];
    __shared__ uint32_t cmd;
    __shared__ uint32_t rq[16];  // the request line
    // Control flow stays wave-uniform: the whole of wave 0 polls (every lane
    // the same word, the value made scalar), and every decision after the
    // barrier is on a scalar.  A poll loop run by one LANE with a workgroup
    // barrier after it lets the compiler park that lane while its wave's other
    // lanes go round the outer loop's barrier on their own (the first build
    // served one request and then spun on it).
    const uint32_t tid = threadIdx.x;
    const bool poller = tid < 64;
    uint32_t served =
        __builtin_amdgcn_readfirstlane(__hip_atomic_load(&mb->served, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM));
    const uint64_t born = __builtin_amdgcn_s_memrealtime();
    if (tid == 0) {  // where this launch landed (nkv_ctx_small_service_state)
        __hip_atomic_store(&mb->hw_id, uint32_t(__builtin_amdgcn_s_getreg(kHwRegHwId)), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&mb->xcc_id, uint32_t(__builtin_amdgcn_s_getreg(kHwRegXccId)), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
    }
    uint64_t seen_rt = 0, seen_mt = 0;  // wave 0: when the latest doorbell was seen (traced requests)
    // (s_memrealtime, s_memtime) of a traced request's phase k into the mailbox
    auto stamp = [&](int k, uint64_t rt, uint64_t mt) {
        __hip_atomic_store(&mb->stamps[2 * k], rt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(&mb->stamps[2 * k + 1], mt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    };
    while (true) {
        if (poller) {
            const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
            uint32_t bell;
            while (true) {
                bell = __builtin_amdgcn_readfirstlane(
                    __hip_atomic_load(&rb->doorbell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM));
                seen_rt = __builtin_amdgcn_s_memrealtime();
                seen_mt = __builtin_amdgcn_s_memtime();
                if (bell != served) break;
                const uint64_t now = __builtin_amdgcn_s_memrealtime();
                if (now - t0 > idle_ticks || now - born > life_ticks) {
                    bell = kSvcExit;
                    break;
                }
                __builtin_amdgcn_s_sleep(2);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");  // system scope: the request's bytes
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (tid == 0) cmd = bell;
        }
        __syncthreads();
        const uint32_t seq = __builtin_amdgcn_readfirstlane(cmd);
        if (seq == kSvcExit) break;
        // One PCIe round trip for the request: the request line (16 lanes of
        // wave 0, one dword each) and, speculatively, the first kSvcSpec bytes
        // of the service's input buffer (16 per thread), all in flight at once;
        // a request packed there (inline_in) needs no second trip below 4 KiB.
        const uint4 spec = reinterpret_cast<const uint4*>(fixed_in)[tid];
        if (tid < 16)
            rq[tid] = __hip_atomic_load(reinterpret_cast<const uint32_t*>(&rb->req) + tid, __ATOMIC_RELAXED,
                                        __HIP_MEMORY_SCOPE_SYSTEM);
        __syncthreads();
        // readfirstlane returns an int: widen through uint32_t, or a low word
        // with its top bit set sign-extends into the pointer's high word (the
        // first build of this read faulted on exactly that)
        auto rq32 = [&](int k) { return uint32_t(__builtin_amdgcn_readfirstlane(rq[k])); };
        auto rq64 = [&](int k) { return uint64_t(rq32(k)) | (uint64_t(rq32(k + 1)) << 32); };
        const uint32_t n = rq32(0);
        const uint32_t vbytes = rq32(1);
        const uint32_t img_at = rq32(2);
        const bool traced = rq32(3) != 0u;
        const uint64_t* desc = reinterpret_cast<const uint64_t*>(rq64(4));
        const uint8_t* vals = reinterpret_cast<const uint8_t*>(rq64(6));
        uint8_t* out = reinterpret_cast<uint8_t*>(rq64(8));
        const bool inline_in = rq32(10) != 0u;
        if (traced && tid == 0) stamp(0, seen_rt, seen_mt);
        // the host never rings with other values; a request out of range is
        // refused (flagged, nothing read or written) rather than followed
        const bool sane = n >= 1 && n <= kSvcMaxN && desc && vals && out &&
                          ((reinterpret_cast<uintptr_t>(desc) | reinterpret_cast<uintptr_t>(vals) |
                            reinterpret_cast<uintptr_t>(out) | img_at) & 15u) == 0u;
        if (!sane && tid == 0) __hip_atomic_store(&mb->refused, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (sane) {
            const uint32_t in_bytes = 16u * n + vbytes;
            if (inline_in && in_bytes <= kSmallSeg) {  // descriptors + values at fixed_in, packed
                if (16u * tid < in_bytes) reinterpret_cast<uint4*>(seg)[tid] = spec;
                if (in_bytes > kSvcSpec)
                    small_stage_in<B>(fixed_in + kSvcSpec, seg + kSvcSpec, in_bytes - kSvcSpec);
                __syncthreads();
                desc = reinterpret_cast<const uint64_t*>(seg);
                vals = seg + 16u * n;
            } else if (in_bytes <= kSmallSeg) {
                small_stage_in<B>(reinterpret_cast<const uint8_t*>(desc), seg, 16u * n);
                small_stage_in<B>(vals, seg + 16u * n, vbytes);
                __syncthreads();
                desc = reinterpret_cast<const uint64_t*>(seg);
                vals = seg + 16u * n;
            }
            if (traced && tid == 0) stamp(1, __builtin_amdgcn_s_memrealtime(), __builtin_amdgcn_s_memtime());
            static_assert(kSvcMaxN <= B, "one leaf per thread");
            if ((tid & ~63u) < n) {  // every lane of a wave with a value (sha1_value_all_lanes)
                const bool real = tid < n;
                uint32_t h[5];
                sha1_value_all_lanes(real ? vals + desc[2 * tid] : vals, real ? uint32_t(desc[2 * tid + 1]) : 0u,
                                     h);  // NewLeaf, merklenode.go:27-34
                if (real) store_digest(sm, tid, h);
            }
            if (traced) {
                __syncthreads();
                if (tid == 0) stamp(2, __builtin_amdgcn_s_memrealtime(), __builtin_amdgcn_s_memtime());
            }
            small_levels_and_image<B>(sm, seg, n, out, img_at, traced ? mb->stamps + 10 : nullptr);
            if (traced && tid == 0) stamp(3, __builtin_amdgcn_s_memrealtime(), __builtin_amdgcn_s_memtime());
        }
        served = seq;
        if (tid == 0) __hip_atomic_store(&mb->served, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (traced && tid == 0) {  // before the completion word: the host reads the stamps after it
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            stamp(4, __builtin_amdgcn_s_memrealtime(), __builtin_amdgcn_s_memtime());
        }
        small_signal_done(&mb->done, seq);
    }
}

// ---------------------------------------------------------------------------
// host-side launchers

hipError_t launch_small_tree(const uint64_t* desc, const uint8_t* vals, uint32_t vbytes, uint32_t n, uint8_t* out,
                             uint32_t img_at, uint8_t* scratch, unsigned int* ticket, unsigned int* done, uint32_t seq,
                             hipStream_t s) {
    if (n == 0 || n > kSmallMaxN || (img_at & 15u) || (reinterpret_cast<uintptr_t>(vals) & 15u) ||
        (reinterpret_cast<uintptr_t>(desc) & 15u))
        return hipErrorInvalidValue;
    const unsigned grid = unsigned((n + kSmallBlock - 1) / kSmallBlock);
    hipLaunchKernelGGL(k_small_tree, dim3(grid), dim3(kSmallBlock), 0, s, desc, vals, vbytes, n, out, img_at, scratch,
                       ticket, done, seq);
    return hipGetLastError();
}

hipError_t launch_small_service(SmallMailbox* mb, const SmallMailbox* rb, const uint8_t* in, uint64_t idle_ticks,
                                uint64_t life_ticks, hipStream_t s) {
    if (!mb || !rb || !in || (reinterpret_cast<uintptr_t>(in) & 15u)) return hipErrorInvalidValue;
    static_assert(kSvcSpec <= kSmallSeg, "speculative read inside the input buffer");
    hipLaunchKernelGGL(k_small_service<kSvcBlock>, dim3(1), dim3(kSvcBlock), 0, s, mb, rb, in, idle_ticks,
                       life_ticks);
    return hipGetLastError();
}

}  // namespace nkv
