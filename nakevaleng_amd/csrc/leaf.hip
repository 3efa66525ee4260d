// leaf.hip -- the leaf level (NewLeaf, merklenode.go:27-34) on gfx950: level 0
// of the nodes buffer (tree_dev.hpp).
//
//   K1  k_leaf         one lane per leaf, 64 leaves per wavefront.
//   K1q k_leaf_queue   the same for ragged, length-sorted batches (work queue).
//   K1v k_leaf_verify  the compaction read: record checksum check + NewLeaf.
//   K1r k_leaf_records the records form: header parse + NewLeaf in one launch.
//
// The block loops are sha1_feed_dev.hpp's; what decides and prepares a pass
// (length sort, locate, scans) is plan.hip; the levels above are reduce.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "bytes_dev.hpp"
#include "crc_dev.hpp"
#include "internal.hpp"
#include "sha1_dev.hpp"
#include "sha1_feed_dev.hpp"
#include "tree_dev.hpp"

namespace nkv {

#ifdef NKV_DIAG
__device__ unsigned long long* g_diag = nullptr;  // NKV_STAMP (internal.hpp)
#endif

// Clock probe (NKV_TIMING_CLOCK; bench.py's sclk_mhz).  Each wave of a leaf
// kernel adds its lifetime in shader-clock cycles (s_memtime) and in 100 MHz
// reference ticks (s_memrealtime) to slot[0] / slot[1] and counts itself in
// slot[2] (slot = g_clk + 32 (workgroup % 8)); the host divides the sums: the
// shader clock the kernel's waves ran at, weighted by their lifetimes.  Off
// (g_clk null) it costs one uniform load.
__device__ unsigned long long* g_clk = nullptr;
struct ClockProbe {
    unsigned long long* p;
    uint64_t c0 = 0, r0 = 0;
    __device__ __forceinline__ ClockProbe() : p(g_clk) {
        if (p) {
            c0 = __builtin_amdgcn_s_memtime();
            r0 = __builtin_amdgcn_s_memrealtime();
        }
    }
    __device__ __forceinline__ void end() const {
        if (p) {
            const uint64_t c1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
            if ((threadIdx.x & 63) == 0) {  // 8 slots on their own 256-B lines: little contention
                unsigned long long* q = p + 32 * (blockIdx.x & 7);
                atomicAdd(q, (unsigned long long)(c1 - c0));
                atomicAdd(q + 1, (unsigned long long)(r1 - r0));
                atomicAdd(q + 2, 1ull);
            }
        }
    }
};

hipError_t set_clock_probe(unsigned long long* p, hipStream_t s) {
    (void)s;
    return hipMemcpyToSymbol(HIP_SYMBOL(g_clk), &p, sizeof(p));
}

// Pass flags (internal.hpp kPassFlagWords): block 0 resets the set the next
// call uses; a workgroup raises this call's deferred / bad-header words with
// one atomic each, skipped once another workgroup has raised them.
__device__ __forceinline__ void pass_flags_reset(uint32_t* f) {
    if (blockIdx.x == 0 && threadIdx.x < kPassFlagWords) f[threadIdx.x] = (threadIdx.x & ~1u) == 6u ? ~0u : 0u;
}
__device__ __forceinline__ void pass_flag_raise(uint32_t* f, uint32_t v) {
    if (__hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != v) atomicOr(f, v);
}

// Value offset of a record k_leaf_records already hashed (the length-sorted
// pass that follows it skips the value).
constexpr uint64_t kDone = ~uint64_t(0);

// CRC tables for k_leaf_verify (crc.hip keeps its own copy: no relocatable
// device code, so each translation unit defines its constants)
__constant__ CrcTables c_crc_leaf = make_crc_tables();

// ---------------------------------------------------------------------------
// K1: leaf SHA-1.
//
// MODE 0: value i at base + i*stride, length L.  MODE 1: base + off[i], len[i].
// perm (MODE 1 only, nullable): lane i hashes leaf perm[i]; a pass after
// k_leaf_records skips the values it hashed (off == kDone).
// No tree level is fused here: a wave-level step costs a whole SHA-1
// instruction stream however few lanes it keeps, so levels built inside the
// leaf kernel (6 per wave, or the workgroup's last wave finishing its 256-leaf
// subtree) cost 3-7 % of a 4 KiB leaf launch, more than k_reduce2 at full lane
// use plus its launch.
// LOAD 4: 16-byte aligned values in 128-byte runs straight into registers
// (sha1_blocks_runs<2>: eight global_load_dwordx4 per lane, every 128-byte line
// fetched once by one lane; 65 VGPRs, 7 waves per SIMD).  LOAD 11: values at
// any address, each wave by the first stage that fits it: the segment stage
// when its values share their offset mod 64 (sha1_blocks_shift), the 80-byte
// window stage when their full-block counts are equal (sha1_blocks_pair), else
// the value-relative LDS-DMA stream (sha1_blocks_lds).  The other load paths
// measured in rounds 1-2 (LDS-DMA stage for aligned values, direct and
// non-temporal loads, 256-byte runs, line-pair stage, runs at each value's own
// address, deep register prefetch) lost their A/Bs and are gone.
constexpr int kRunsWaves = 4;  // launch bound of the LOAD 4 kernel
template <int MODE, int LOAD>
__global__ __launch_bounds__(kBlock, LOAD == 4 ? kRunsWaves : kLeafWavesPerSimd) void k_leaf(
    const uint8_t* __restrict__ base, const uint64_t* __restrict__ off, const uint64_t* __restrict__ len,
    uint64_t stride, uint64_t L, const uint32_t* __restrict__ perm, uint64_t n, uint8_t* __restrict__ nodes,
    Gate gate) {
    static_assert(LOAD == 4 || LOAD == 11, "leaf load path");
    // LOAD 11: four wave-private 5 KiB stages (the window stage's 80-byte rows)
    __shared__ __attribute__((aligned(16))) uint8_t smem[LOAD == 11 ? kBlock * 80 : 16];
    if (!gate.open()) return;
    NKV_STAMP(0);
    const ClockProbe clk;
    const uint64_t g = blockIdx.x;
    const uint64_t t = g * kBlock + threadIdx.x;
    uint32_t h[5] = {0u, 0u, 0u, 0u, 0u};
    uint64_t leaf = t;
    // a length-sorted batch after k_leaf_records skips the values it hashed
    const bool live = t < n && (MODE == 0 || !perm || off[perm[t]] != kDone);
    const uint8_t* p = nullptr;
    uint64_t ln = 0;
    if (live) {
        if (MODE == 0) {
            p = base + t * stride;
            ln = L;
        } else {
            leaf = perm ? uint64_t(perm[t]) : t;
            p = base + off[leaf];
            ln = len[leaf];
        }
    }
    sha1_init(h);
    if constexpr (LOAD == 4) {
        if (live) {
            sha1_blocks_runs<2>(p, uint32_t(ln >> 6), h);
            // one length for all: a whole-block length's padding block is the
            // same message in every lane (its schedule on the scalar unit)
            if (MODE == 0 && (L & 63) == 0) sha1_pad_uniform(h, L);
            else sha1_tail<true>(p, ln, h);
            store_digest(nodes, leaf, h);
        }
    } else {
        // wave-cooperative stages of the full blocks, then the tail.  Every
        // stage reads only full blocks' bytes, so nothing past a value is read.
        const int lane = threadIdx.x & 63;
        const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        uint8_t* wbuf = smem + 5120 * wave;
        const uint32_t q = (uint32_t(lane) & 3u) ^ ((uint32_t(lane) >> 4) & 3u);
        const uint32_t my_nfull = live ? uint32_t(ln >> 6) : 0u;
        bool staged = sha1_blocks_shift(wbuf, p, live, my_nfull, h);
        if (!staged) staged = sha1_blocks_pair(wbuf, p, live, my_nfull, h);
        if (staged) {
            // done (wave-uniform)
        } else if (MODE == 0) {
            // value j of this wave at wave_base + j * stride.  Only a wave that
            // spans more than 4 GiB gets here (equal block counts: the window
            // stage refuses nothing else), so every offset is 64-bit: one
            // pointer per lane, the role's and the block's steps wave-uniform
            const uint64_t first = g * kBlock + 64 * uint64_t(wave);
            const uint8_t* wave_base = base + first * stride;
            const uint32_t nvalid = first < n ? uint32_t(min(uint64_t(64), n - first)) : 0u;
            const uint8_t* src0 = wave_base + (uint64_t(lane >> 2) * stride + 16u * q);
            const uint64_t kstep = 16ull * stride;
            const uint32_t nmax = nvalid ? uint32_t(L >> 6) : 0u;
            auto issue = [&](uint32_t b) {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (uint32_t(16 * k + (lane >> 2)) < nvalid)
                        __builtin_amdgcn_global_load_lds(src0 + (uint64_t(k) * kstep + 64ull * b),
                                                         wbuf + 1024 * k, 16, 0, 0);
            };
            sha1_blocks_lds(wbuf, nmax, my_nfull, issue, h);
        } else {
            const uint8_t* src[4];
            uint32_t nf[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int j = 16 * k + (lane >> 2);
                const uint64_t pj = uint64_t(__shfl(int64_t(reinterpret_cast<uintptr_t>(p)), j));
                src[k] = reinterpret_cast<const uint8_t*>(pj) + 16 * q;
                nf[k] = uint32_t(__shfl(int(my_nfull), j));
            }
            auto issue = [&](uint32_t b) {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (b < nf[k])
                        __builtin_amdgcn_global_load_lds(src[k] + 64ull * b, wbuf + 1024 * k, 16, 0, 0);
            };
            sha1_blocks_lds(wbuf, wave_max_u32(my_nfull), my_nfull, issue, h);
        }
        if constexpr (MODE == 1) {
            // reload the value's place instead of keeping it live through the
            // register stage (its two 16-dword segment sets need the VGPRs)
            asm volatile("" ::: "memory");
            if (live) {
                leaf = perm ? uint64_t(perm[t]) : t;
                p = base + off[leaf];
                ln = len[leaf];
            }
        }
        if (live) {
            sha1_tail<false>(p, ln, h);
            store_digest(nodes, leaf, h);
        }
    }
    clk.end();
    NKV_STAMP(1);
    NKV_STAMP(2);
#ifdef NKV_DIAG
    if (g_diag && (threadIdx.x & 63) == 0) {
        unsigned xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        unsigned hw;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        const size_t w_ = size_t(blockIdx.x) * (kBlock / 64) + (threadIdx.x >> 6);
        g_diag[w_ * 8 + 6] = (uint64_t(xcc) << 32) | hw;
    }
#endif
}

// k_leaf_verify's block hook: the CRC steps over the 16 big-endian words SHA-1
// takes, with the state byte-swapped (cs = bswap(crc)) against byte-swapped
// tables stored in reverse order (slot k = bswap(T[3 - k]), crc_dev.hpp), so
// the same x-form step indexes the right bytes and no extra byte swap runs.
// (Spreading the 16 steps over the rounds, one per one or two rounds, ran
// 0.3 % faster and 6 % slower: the lookups' latency is not what bounds it.)
struct CrcBE {
    uint32_t& cs;
    const uint32_t* swtab;
    const uint32_t* tab0;  // T[0], for the last 0-3 bytes
    __device__ __forceinline__ void be(const uint32_t* w) { cs = crc_block16<1>(cs, w, swtab); }
    __device__ __forceinline__ void operator()(const uint4*, const uint32_t* w) { be(w); }
    // the first nb (<= 64) bytes held by 16 big-endian words: whole words in
    // the swapped domain, then the 0-3 bytes of the partial word
    __device__ __forceinline__ void span(const uint32_t* w, uint32_t nb) {
        const uint32_t nfw = nb >> 2;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const uint32_t u = crc_x_last<1>(cs ^ w[i], swtab);
            cs = uint32_t(i) < nfw ? u : cs;
        }
        uint32_t pw = 0u;
#pragma unroll
        for (int i = 0; i < 16; ++i) pw = uint32_t(i) == nfw ? w[i] : pw;
        uint32_t crc = __builtin_bswap32(cs);
        for (uint32_t b = 0; b < (nb & 3u); ++b) crc = crc_byte<1>(crc, (pw >> (24u - 8u * b)) & 0xFFu, tab0);
        cs = __builtin_bswap32(crc);
    }
    // the value's last rem (< 64) bytes, from the words sha1_tail loaded
    __device__ __forceinline__ void tail(const uint32_t* w, uint32_t rem) { span(w, rem); }
};

// K1v: the compaction read of a Data table in one pass.  For every record it
// checks record.Deserialize's checksum (record.go:163-169: crc32.ChecksumIEEE
// of Key ++ Value against the stored Crc) and computes NewLeaf(Value)
// (merklenode.go:27-34), reading each byte once.  The value-relative LDS-DMA
// stream of k_leaf (LOAD 8) feeds both: each 64-byte block's 16 little-endian
// words step the CRC (slicing-by-4 from one LDS table copy) before the byte
// swap feeds SHA-1.  The key, which precedes the value, and the value's tail
// are checksummed bytewise from global memory.  SHA-1 is VALU-bound and leaves
// the LDS nearly idle, so the lookups ride along.  A record whose header points
// outside the stream sets stats[2] and gets the digest of an empty value, as
// in nkv_tree_from_records_dev.
//
// The header parse is k_locate's, so no separate locate pass runs.  policy
// (as k_leaf_records): 0 hashes every wave here; 1 (auto) hashes the waves
// whose value block counts are narrow by the plan rule and defers the others;
// 2 defers all.  A deferred wave only checksums its records here (crc_span
// over Key ++ Value, the CRC is cheap next to SHA-1) and leaves each value's
// voff / vlen for the length-sorted leaf pass; a hashed value's voff becomes
// kDone.  Each workgroup leaves (0, deferred ? ~0 : 0, 0) in part, folded by
// k_locate_fold into the range whose wide Gate opens the sorted pass.
constexpr int kVerifyWaves = 4;  // whole lines in registers with the CRC state: ~105 VGPRs
__global__ __launch_bounds__(kBlock, kVerifyWaves) void k_leaf_verify(
    const uint8_t* __restrict__ stream, uint64_t stream_len, const uint64_t* __restrict__ rec_off, uint64_t n,
    int policy, uint64_t* __restrict__ voff, uint64_t* __restrict__ vlen, uint8_t* __restrict__ nodes,
    uint32_t* __restrict__ crc_out, unsigned long long* __restrict__ stats, uint32_t* __restrict__ part,
    uint32_t* __restrict__ flags, uint32_t* __restrict__ flags_next) {
    if (flags) pass_flags_reset(flags_next);
    const ClockProbe clk;
    // ONE LDS object (a second one can cost the DMA loop its waits): four
    // 4 KiB wave stages, the 4 KiB of byte-swapped word tables (CrcBE), then
    // T[0] for the bytewise steps: 21 KiB, seven workgroups per CU
    __shared__ __attribute__((aligned(16))) uint8_t smem[kBlock * 64 + 4096 + 1024];
    uint32_t* swtab = reinterpret_cast<uint32_t*>(smem + kBlock * 64);
    uint32_t* tab = swtab + 4 * 256;
    for (int i = threadIdx.x; i < 4 * 256; i += kBlock)
        swtab[i] = __builtin_bswap32(c_crc_leaf.t[3 - (i >> 8)][i & 255]);
    for (int i = threadIdx.x; i < 256; i += kBlock) tab[i] = c_crc_leaf.t[0][i];
    __syncthreads();
    const uint64_t t = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool live = t < n;
    const uint8_t* key = stream;
    const uint8_t* p = stream;
    uint64_t ks = 0, ln = 0;
    uint32_t stored = 0;
    bool hdr_bad = false;
    if (live) {
        const uint64_t r = rec_off[t];
        if (header_in(r, stream_len)) {
            uint64_t k, v;
            ld_header_sizes(stream + r, k, v);
            if (k <= stream_len && v <= stream_len && r + 30 + k + v <= stream_len) {
                key = stream + r + 30;
                ks = k;
                p = key + k;
                ln = v;
                // the stored Crc (header bytes 0..3) from the one or two aligned
                // words that hold it
                const uint8_t* c = stream + r;
                const uint32_t mis = uint32_t(reinterpret_cast<uintptr_t>(c) & 3u);
                const uint32_t* cw = reinterpret_cast<const uint32_t*>(c - mis);
                const uint32_t c0 = cw[0];
                const uint32_t c1 = mis ? cw[1] : 0u;
                stored = mis ? (c0 >> (8u * mis)) | (c1 << (32u - 8u * mis)) : c0;
            } else {
                hdr_bad = true;
            }
        } else {
            hdr_bad = true;
        }
    }
    const uint64_t bl = ln >> 6;
    const uint32_t my_nfull = bl > 0xFFFFFFFFull ? 0xFFFFFFFFu : uint32_t(bl);
    const uint32_t wlo = wave_min_u32(live ? my_nfull : 0xFFFFFFFFu);
    const uint32_t whi = wave_max_u32(live ? my_nfull : 0u);
    const bool any = __any(live);
    const bool hash = any && (policy == 0 || (policy == 1 && whi <= wlo + max(1u, wlo / 16u)));
    uint32_t crc;
    if (hash) {
        uint32_t cs = 0xFFFFFFFFu;  // bswap(~0): the CRC starts in the swapped domain
        CrcBE hook{cs, swtab, tab};
        {  // the key, 64 bytes at a time from aligned 16-byte loads (most keys: one pass)
            const uint32_t kch = wave_max_u32(uint32_t(min<uint64_t>((ks + 63) >> 6, 0xFFFFFFFFull)));
            for (uint32_t c = 0; c < kch; ++c) {
                const uint64_t done = 64ull * c;
                const uint32_t avail = ks > done ? uint32_t(min<uint64_t>(64ull, ks - done)) : 0u;
                const uint8_t* kc = key + (avail ? done : 0ull);
                uint32_t d[20], w[16];
                load_window(kc, avail, d);
                be16_funnel(d, uint32_t(reinterpret_cast<uintptr_t>(kc) & 15u), w);
                hook.span(w, avail);
            }
        }
        uint8_t* wbuf = smem + 4096 * wave;
        const uint32_t q = (uint32_t(lane) & 3u) ^ ((uint32_t(lane) >> 4) & 3u);
        uint32_t h[5];
        sha1_init(h);
        const uint8_t* src[4];
        uint32_t nf[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int j = 16 * k + (lane >> 2);
            const uint64_t pj = uint64_t(__shfl(int64_t(reinterpret_cast<uintptr_t>(p)), j));
            src[k] = reinterpret_cast<const uint8_t*>(pj) + 16 * q;
            nf[k] = uint32_t(__shfl(int(my_nfull), j));
        }
        auto issue = [&](uint32_t b) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (b < nf[k]) __builtin_amdgcn_global_load_lds(src[k] + 64ull * b, wbuf + 1024 * k, 16, 0, 0);
        };
        // records of one size share their offset mod 64: each line once
        // through the segment stage (LOAD 11); else the value-relative stream
        if (!sha1_blocks_shift<decltype(hook), true>(wbuf, p, live, my_nfull, h, hook))
            sha1_blocks_lds(wbuf, whi, my_nfull, issue, h, hook);
        if (live) {
            sha1_tail<false>(p, ln, h, hook);  // the tail's checksum from the same loads
            store_digest(nodes, t, h);
            if (voff) {
                voff[t] = kDone;
                vlen[t] = 0;
            }
        }
        crc = ~__builtin_bswap32(cs);
    } else {
        // deferred: Key ++ Value is one contiguous span of the record
        crc = crc_span<1, true>(key, ks + ln, tab, swtab);
        if (live) {
            voff[t] = uint64_t(p - stream);
            vlen[t] = ln;
        }
    }
    if (live) {
        if (crc_out) crc_out[t] = crc;
        if (hdr_bad) {
            atomicOr(stats + 2, 1ull);
        } else if (crc != stored) {
            atomicAdd(stats, 1ull);
            atomicMin(stats + 1, (unsigned long long)t);
        }
    }
    if (part || flags) {  // one partial per workgroup, through the (now idle) stage LDS
        const bool wdefer = any && !hash;
        uint32_t* wf = reinterpret_cast<uint32_t*>(smem);
        __syncthreads();
        if (lane == 0) wf[threadIdx.x >> 6] = wdefer ? 1u : 0u;
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t f = 0u;
#pragma unroll
            for (int k = 0; k < kBlock / 64; ++k) f |= wf[k];
            if (flags) {
                if (f) pass_flag_raise(flags + 1, 0xFFFFFFFFu);
            } else {
                part[3 * blockIdx.x] = 0u;
                part[3 * blockIdx.x + 1] = f ? 0xFFFFFFFFu : 0u;
                part[3 * blockIdx.x + 2] = 0u;
            }
        }
    }
    clk.end();
}

// K1q: ragged batches, work-queue form.  Values are length-sorted, longest
// first, and cut into 64-value groups.  A group is one wavefront's work, and a
// group's 64 chains run as long as its longest value, so the batch can finish
// no sooner than its longest group.  Static dispatch places consecutive
// (= equally long) workgroups on one CU, which stacks the longest chains on a
// few SIMDs.  Here each wave (64-thread workgroup, two per SIMD) reads its
// SIMD id: the first wave on a SIMD pulls groups from the long end at priority
// 3, the others pull from the short end and fill the issue slots the long
// chain leaves.  The two ends meet; a per-group claim flag settles the last
// group.  Every wave exits once its end meets the other one.
//
// The other waves only take groups whose longest chain is at most split
// blocks (group index >= q[2], set by the sort's queue_header): long groups all go
// longest-first to the one raised-priority wave per SIMD, so the batch ends on
// short groups instead of on a medium one pulled late from the short end.
//
// q: [0] front ticket, [1] back ticket, [2] first short group, [3] unused,
//    [4, 4 + kSimdKeys) per-SIMD arrivals, then ngroups claim flags; zeroed
//    before the launch (kQueueHeader, kSimdKeys: internal.hpp).

// Values are staged through a pipelined wave-private LDS ring of
// value-relative chunks (sha1_blocks_ring_vc, kQueueRing = 3 slots of 4 KiB:
// two blocks of DMA lookahead; 3 waves per SIMD fit).  The other rings and the
// register-prefetch forms of rounds 1-2 lost their A/Bs.
constexpr int kQueueRing = 3;
__global__ __launch_bounds__(64, kQueueRing) void k_leaf_queue(const uint8_t* __restrict__ base,
                                                       const uint64_t* __restrict__ off,
                                                       const uint64_t* __restrict__ len,
                                                       const uint32_t* __restrict__ perm, uint64_t n,
                                                       uint32_t ngroups, uint32_t simds, uint32_t* __restrict__ q,
                                                       uint8_t* __restrict__ nodes, Gate gate) {
    __shared__ __attribute__((aligned(16))) uint8_t smem[4096 * kQueueRing];
    if (!gate.open()) return;
    const ClockProbe clk;
    const int lane = threadIdx.x;
    uint32_t hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    const uint32_t key = ((((xcc & 7) * 8 + ((hw >> 13) & 7)) * 2 + ((hw >> 12) & 1)) * 16 + ((hw >> 8) & 15)) * 4 +
                         ((hw >> 4) & 3);
    uint32_t slot = 0;
    if (lane == 0) slot = atomicAdd(q + kQueueHeader + key, 1u);
    slot = __builtin_amdgcn_readfirstlane(slot);
    const bool front = slot == 0;
    if (front) __builtin_amdgcn_s_setprio(3);
    // queue_header's results: the first group short enough for the
    // non-priority waves, and the batch's work; a throughput-bound batch (work
    // at least twice what the longest chain keeps every SIMD busy for) lets
    // every wave take any group
    const uint64_t work = reinterpret_cast<const unsigned long long*>(q)[2];
    const uint64_t longest = compressions(len[perm[0]]);
    const uint32_t first_short = __builtin_amdgcn_readfirstlane(
        work >= 2ull * simds * longest ? 0u : min(q[2], ngroups));
    uint32_t* claimed = q + kQueueHeader + kSimdKeys;
#ifdef NKV_DIAG
    uint64_t d_t0 = __builtin_amdgcn_s_memrealtime(), d_c0 = __builtin_amdgcn_s_memtime(), d_first = 0;
    uint64_t d_groups = 0, d_blocks = 0;
#endif
    while (true) {
        uint32_t g = 0xFFFFFFFFu;
        if (lane == 0) {
            const uint32_t t = atomicAdd(q + (front ? 0 : 1), 1u);
            if (t < ngroups) {
                const uint32_t c = front ? t : ngroups - 1 - t;
                if ((front || c >= first_short) && atomicExch(claimed + c, 1u) == 0u) g = c;
            }
        }
        g = __builtin_amdgcn_readfirstlane(g);
        if (g == 0xFFFFFFFFu) break;
        const uint64_t i = uint64_t(g) * 64 + lane;
        const uint64_t leaf = i < n ? perm[i] : 0;
        const uint64_t vo = i < n ? off[leaf] : kDone;
        const bool live = vo != kDone;  // kDone: hashed by k_leaf_records
        const uint8_t* p = live ? base + vo : base;
        const uint64_t ln = live ? len[leaf] : 0;
        uint32_t h[5];
        sha1_init(h);
        sha1_blocks_ring_vc<kQueueRing>(smem, p, uint32_t(ln >> 6), h);
        if (live) {
            sha1_tail<false>(p, ln, h);
            store_digest(nodes, leaf, h);
        }
#ifdef NKV_DIAG
        d_blocks += wave_max_u32(i < n ? uint32_t(len[perm[i]] >> 6) : 0u);
        if (d_groups++ == 0) d_first = __builtin_amdgcn_s_memrealtime();
#endif
    }
    clk.end();
#ifdef NKV_DIAG
    if (g_diag && lane == 0) {
        unsigned long long* d = g_diag + size_t(blockIdx.x) * 8;
        d[0] = d_t0;
        d[1] = __builtin_amdgcn_s_memrealtime();
        d[2] = d_c0;
        d[3] = __builtin_amdgcn_s_memtime();
        d[4] = (uint64_t(slot) << 32) | key;
        d[5] = d_groups;
        d[6] = d_blocks;
        d[7] = d_first;
    }
#endif
}

// K1r: the records form's leaf pass in one launch (nkv_tree_from_records*):
// k_locate's header parse (value = rec + 30 + KeySize, ValueSize bytes;
// record.go:191-199) and k_leaf's hash of the value, so the header line is
// read once and no separate locate pass runs.  policy 0 hashes every wave in
// input order; 1 (auto) hashes the waves whose full-block counts are narrow
// by the plan rule (max <= min + max(1, min / 16), Gate) and defers the others
// to the length-sorted work queue; 2 defers all.  A hashed value's voff is
// set to kDone (vlen 0): the sorted pass skips it.  A deferred value keeps its
// voff / vlen.  Each workgroup leaves (0, deferred ? ~0 : 0, bad) in part,
// which k_locate_fold turns into err and a range whose wide Gate opens the
// sorted pass only when something was deferred.  A header outside the
// stream flags bad and hashes the empty value (as k_locate).
constexpr int kRecordsWaves = 5;  // narrow waves of line-aligned records take whole lines: ~86 VGPRs
__global__ __launch_bounds__(kBlock, kRecordsWaves) void k_leaf_records(
    const uint8_t* __restrict__ stream, uint64_t stream_len, const uint64_t* __restrict__ rec_off, uint64_t n,
    int policy, uint64_t* __restrict__ voff, uint64_t* __restrict__ vlen, uint8_t* __restrict__ nodes,
    uint32_t* __restrict__ part, uint32_t* __restrict__ flags, uint32_t* __restrict__ flags_next) {
    __shared__ __attribute__((aligned(16))) uint8_t smem[kBlock * 80];
    if (flags) pass_flags_reset(flags_next);
    const ClockProbe clk;
    const uint64_t t = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    const bool live = t < n;
    uint64_t o = 0, l = 0;
    uint32_t bad = 0u;
    if (live) {
        const uint64_t r = rec_off[t];
        if (header_in(r, stream_len)) {
            uint64_t ks, vs;
            ld_header_sizes(stream + r, ks, vs);
            o = r + 30 + ks;
            l = vs;
            if (ks > stream_len || vs > stream_len || o + l > stream_len) {
                bad = 1u;
                o = 0;
                l = 0;
            }
        } else {
            bad = 1u;
        }
        voff[t] = o;
        vlen[t] = l;
    }
    const uint64_t bl = l >> 6;
    const uint32_t b32 = bl > 0xFFFFFFFFull ? 0xFFFFFFFFu : uint32_t(bl);
    const uint32_t wlo = wave_min_u32(live ? b32 : 0xFFFFFFFFu);
    const uint32_t whi = wave_max_u32(live ? b32 : 0u);
    const bool any = __any(live);
    const bool hash = any && (policy == 0 || (policy == 1 && whi <= wlo + max(1u, wlo / 16u)));
    // wave-level partials, so no per-lane flag stays live through the stage
    const bool wbad = __any(bad != 0u);
    const bool wdefer = any && !hash;
    if (hash) {
        const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        uint32_t h[5];
        sha1_init(h);
        sha1_blocks_any<true>(smem + 5120 * wave, stream + o, live, live ? b32 : 0u, h);
        // reload the value's place (written above by this lane) rather than
        // keeping it, or its addresses, live through the stage
        asm volatile("" ::: "memory");
        uint32_t tid = threadIdx.x;
        asm volatile("" : "+v"(tid));
        const uint64_t u = uint64_t(blockIdx.x) * kBlock + tid;
        if (u < n) {
            o = voff[u];
            l = vlen[u];
            sha1_tail<false>(stream + o, l, h);
            store_digest(nodes, u, h);
            voff[u] = kDone;
            vlen[u] = 0;
        }
    }
    // one partial per workgroup, folded through the (now idle) stage LDS: a
    // block_fold of its own would cost LDS, i.e. a workgroup per CU
    const int wv = threadIdx.x >> 6;
    uint32_t* wf = reinterpret_cast<uint32_t*>(smem);
    __syncthreads();  // every wave is done with its stage
    if ((threadIdx.x & 63) == 0) wf[wv] = (wdefer ? 2u : 0u) | (wbad ? 1u : 0u);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t f = 0u;
#pragma unroll
        for (int k = 0; k < kBlock / 64; ++k) f |= wf[k];
        if (flags) {  // the pass flags (no fold launch)
            if (f & 2u) pass_flag_raise(flags + 1, 0xFFFFFFFFu);
            if (f & 1u) pass_flag_raise(flags + 2, 1u);
        } else {
            part[3 * blockIdx.x] = 0u;
            part[3 * blockIdx.x + 1] = (f & 2u) ? 0xFFFFFFFFu : 0u;
            part[3 * blockIdx.x + 2] = f & 1u;
        }
    }
    clk.end();
}

// ---------------------------------------------------------------------------
// host-side launchers

template <int MODE, int LOAD>
static void leaf_kernel(const uint8_t* base, const uint64_t* off, const uint64_t* len, uint64_t stride, uint64_t L,
                        const uint32_t* perm, uint64_t n, uint8_t* nodes, hipStream_t s, Gate gate) {
    hipLaunchKernelGGL((k_leaf<MODE, LOAD>), dim3(blocks_for(n)), dim3(kBlock), 0, s, base, off, len, stride, L,
                       perm, n, nodes, gate);
}

// load (NKV_OPT_LEAF_LOAD): 4 = 128-byte register runs for 16-byte aligned
// values (anything else takes 11); 11 = the staged paths for every value
template <int MODE>
static void leaf_dispatch(int load, bool aligned, const uint8_t* base, const uint64_t* off, const uint64_t* len,
                          uint64_t stride, uint64_t L, const uint32_t* perm, uint64_t n, uint8_t* nodes,
                          hipStream_t s, Gate g) {
    if (load == 4 && aligned) leaf_kernel<MODE, 4>(base, off, len, stride, L, perm, n, nodes, s, g);
    else leaf_kernel<MODE, 11>(base, off, len, stride, L, perm, n, nodes, s, g);
}

hipError_t launch_leaf_strided(const uint8_t* base, uint64_t stride, uint64_t L, uint64_t n, int load,
                               uint8_t* nodes, hipStream_t s) {
    const bool al = ((reinterpret_cast<uintptr_t>(base) | stride) & 15) == 0;
    leaf_dispatch<0>(load, al, base, nullptr, nullptr, stride, L, nullptr, n, nodes, s, Gate{});
    return hipGetLastError();
}

hipError_t launch_leaf_offsets(const uint8_t* base, const uint64_t* off, const uint64_t* len, uint64_t n,
                               bool aligned, int load, uint8_t* nodes, hipStream_t s, Gate gate) {
    leaf_dispatch<1>(load, aligned, base, off, len, 0, 0, nullptr, n, nodes, s, gate);
    return hipGetLastError();
}

hipError_t launch_leaf_verify(const uint8_t* stream, uint64_t stream_len, const uint64_t* rec_off, uint64_t n,
                              int policy, uint64_t* voff, uint64_t* vlen, uint8_t* nodes, uint32_t* crc_out,
                              unsigned long long* stats, unsigned int* range, uint32_t* part, hipStream_t s,
                              uint32_t* flags, uint32_t* flags_next) {
    const unsigned nb = blocks_for(n);
    if (policy == 0) flags = nullptr;
    hipLaunchKernelGGL(k_leaf_verify, dim3(nb), dim3(kBlock), 0, s, stream, stream_len, rec_off, n, policy, voff,
                       vlen, nodes, crc_out, flags ? reinterpret_cast<unsigned long long*>(flags + 4) : stats,
                       (policy == 0 || flags) ? nullptr : part, flags, flags_next);
    if (policy != 0 && !flags) launch_locate_fold(part, nb, nullptr, range, s);
    return hipGetLastError();
}

hipError_t launch_leaf_queue(const uint8_t* base, const uint64_t* off, const uint64_t* len, const uint32_t* perm,
                             uint64_t n, uint32_t* q, uint32_t simds, uint32_t waves_per_simd, uint8_t* nodes,
                             hipStream_t s, Gate gate) {
    const uint32_t ngroups = uint32_t((n + 63) / 64);
    const uint32_t waves = simds * std::min<uint32_t>(std::max<uint32_t>(waves_per_simd, 1u), uint32_t(kQueueRing));
    hipLaunchKernelGGL(k_leaf_queue, dim3(waves), dim3(64), 0, s, base, off, len, perm, n, ngroups, simds, q, nodes,
                       gate);
    return hipGetLastError();
}

hipError_t launch_leaf_records(const uint8_t* stream, uint64_t stream_len, const uint64_t* rec_off, uint64_t n,
                               int policy, uint64_t* voff, uint64_t* vlen, uint8_t* nodes, unsigned int* err,
                               unsigned int* range, uint32_t* part, hipStream_t s, uint32_t* flags,
                               uint32_t* flags_next) {
    const unsigned nb = blocks_for(n);
    if (policy == 0) flags = nullptr;
    hipLaunchKernelGGL(k_leaf_records, dim3(nb), dim3(kBlock), 0, s, stream, stream_len, rec_off, n, policy, voff,
                       vlen, nodes, part, flags, flags_next);
    if (!flags) launch_locate_fold(part, nb, err, range, s);
    return hipGetLastError();
}

#ifdef NKV_DIAG
hipError_t set_diag_leaf(unsigned long long* p) { return hipMemcpyToSymbol(HIP_SYMBOL(g_diag), &p, sizeof(p)); }

extern "C" int nkv_diag_set_buffer(void* d) {
    unsigned long long* p = static_cast<unsigned long long*>(d);
    return set_diag_leaf(p) == hipSuccess && set_diag_small(p) == hipSuccess ? 0 : 3;
}
#endif

}  // namespace nkv
