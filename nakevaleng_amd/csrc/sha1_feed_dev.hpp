// sha1_feed_dev.hpp -- everything between a value's bytes and sha1_compress
// (sha1_dev.hpp): the big-endian word forms, the padding blocks, the wave
// reductions and the block loops that stage a wave's 64 values (registers,
// LDS-DMA stages, the pipelined ring).  Shared by the leaf kernels (leaf.hip),
// the small tree (small_tree.hip) and the stand-alone probes under tools/.
//
// Each lane hashes the value p[0 .. len).  Full 64-byte blocks are streamed
// with a one-block register prefetch; the 1-2 padding blocks are built from
// the remaining 0..63 bytes (FIPS 180-4 5.1.1).  A 16-byte aligned wave takes
// 4 x global_load_dwordx4 per block; otherwise each lane reads the five
// aligned 16-byte chunks that cover its 64 bytes and funnels them with
// v_perm_b32 (never touching an aligned chunk that holds no value byte, so it
// cannot step onto an unmapped page).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sha1_dev.hpp"

namespace nkv {

// SHA-1 compressions of a len-byte message (FIPS 180-4 padding: + 0x80 + 8 B)
__device__ __forceinline__ uint64_t compressions(uint64_t len) { return (len + 8) / 64 + 1; }

__device__ __forceinline__ void be16_from_raw(const uint4 c[4], uint32_t w[16]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        w[4 * q + 0] = bswap32(c[q].x);
        w[4 * q + 1] = bswap32(c[q].y);
        w[4 * q + 2] = bswap32(c[q].z);
        w[4 * q + 3] = bswap32(c[q].w);
    }
}

// d[0..19]: 20 little-endian dwords of the aligned 80-byte window; s = byte
// shift 0..15 of the stream start inside it.  Produces 16 big-endian words.
__device__ __forceinline__ void be16_funnel(const uint32_t d[20], uint32_t s, uint32_t w[16]) {
    // Dword select by k = s >> 2 in two v_perm_b32 steps (a plain ?: on the
    // array would be folded into a dynamically indexed private array).
    const uint32_t k = s >> 2;
    const uint32_t sel = be_sel(s & 3u);
    const uint32_t sel1 = (k & 1u) ? 0x07060504u : 0x03020100u;
    const uint32_t sel2 = (k & 2u) ? 0x07060504u : 0x03020100u;
    uint32_t m1[19];
#pragma unroll
    for (int j = 0; j < 19; ++j) m1[j] = __builtin_amdgcn_perm(d[j + 1], d[j], sel1);
    uint32_t m2[17];
#pragma unroll
    for (int j = 0; j < 17; ++j) m2[j] = __builtin_amdgcn_perm(m1[j + 2], m1[j], sel2);
#pragma unroll
    for (int j = 0; j < 16; ++j) w[j] = be_word(m2[j + 1], m2[j], sel);
}

__device__ __forceinline__ void load_window(const uint8_t* p, uint32_t avail, uint32_t d[20]) {
    // p: stream start; avail: value bytes available from p (>= 1 unless empty).
    // p - s (not an integer-to-pointer cast) keeps the global address space,
    // so these stay global_load_dwordx4 rather than flat loads
    const uint32_t s = uint32_t(reinterpret_cast<uintptr_t>(p) & 15);
    const uint4* q = reinterpret_cast<const uint4*>(p - s);
#pragma unroll
    for (int c = 0; c < 5; ++c) {
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (avail > 0 && uint32_t(16 * c) < s + avail) v = q[c];
        d[4 * c + 0] = v.x;
        d[4 * c + 1] = v.y;
        d[4 * c + 2] = v.z;
        d[4 * c + 3] = v.w;
    }
}

// ALIGNED: the caller guarantees p is 16-byte aligned (host-checked base and
// stride, or host-packed values); otherwise a wave-uniform test picks the path.
struct NoRaw;
template <bool ALIGNED, class Hook = NoRaw>
__device__ __forceinline__ void sha1_tail(const uint8_t* p, uint64_t len, uint32_t h[5], Hook hook = Hook{});

// The 1-2 padding blocks: rem = len % 64 value bytes, 0x80, zeros, 64-bit
// big-endian bit length (FIPS 180-4 5.1.1).  h holds the state after the full
// blocks.
// hook.tail(w, rem): the tail block's big-endian words before the padding is
// applied (rem = len % 64 value bytes), for k_leaf_verify's checksum.
template <bool ALIGNED, class Hook>
__device__ __forceinline__ void sha1_tail(const uint8_t* p, uint64_t len, uint32_t h[5], Hook hook) {
    uint32_t w[16];
    const uint64_t nfull = len >> 6;
    const uint32_t rem = uint32_t(len & 63);
    const uint64_t bits = len << 3;
    // A wave-level step issues every instruction whatever the exec mask, so the
    // branches below are taken on wave votes: a wave whose values are all
    // whole blocks (every 4 KiB SSTable value) pays neither the byte loads and
    // masking nor a second compression that no lane needs.
    if (__all(rem == 0u)) {
        w[0] = 0x80000000u;
#pragma unroll
        for (int j = 1; j < 14; ++j) w[j] = 0u;
        w[14] = uint32_t(bits >> 32);
        w[15] = uint32_t(bits);
        sha1_compress(h, w);
        return;
    }
    const uint8_t* pt = p + 64 * nfull;
    if (ALIGNED) {
        const uint4* q = reinterpret_cast<const uint4*>(pt);
        uint4 c[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) c[i] = (uint32_t(16 * i) < rem) ? q[i] : make_uint4(0u, 0u, 0u, 0u);
        be16_from_raw(c, w);
    } else {
        uint32_t d[20];
        load_window(pt, rem, d);
        be16_funnel(d, uint32_t(reinterpret_cast<uintptr_t>(pt) & 15), w);
    }
    hook.tail(w, rem);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const int v = int(rem) - 4 * j;  // value bytes inside word j
        uint32_t m = v >= 4 ? 0xFFFFFFFFu : (v <= 0 ? 0u : (0xFFFFFFFFu << (32 - 8 * v)));
        uint32_t x = w[j] & m;
        if (v >= 0 && v < 4) x |= 0x80u << (24 - 8 * v);
        w[j] = x;
    }
    const bool two = rem >= 56;
    if (!two) {
        w[14] = uint32_t(bits >> 32);
        w[15] = uint32_t(bits);
    }
    sha1_compress(h, w);
    if (__any(two)) {
        uint32_t h2[5];
#pragma unroll
        for (int j = 0; j < 14; ++j) w[j] = 0u;
        w[14] = uint32_t(bits >> 32);
        w[15] = uint32_t(bits);
#pragma unroll
        for (int i = 0; i < 5; ++i) h2[i] = h[i];
        sha1_compress(h2, w);
#pragma unroll
        for (int i = 0; i < 5; ++i) h[i] = two ? h2[i] : h[i];
    }
}

// Full 64-byte blocks of the 64 values owned by one wavefront, streamed
// HBM -> LDS with LDS-DMA (global_load_lds_dwordx4: no VGPR staging, fully
// used 64-byte runs per request), one 4 KiB stage per block, wave-private.
//
// Stage layout: value j's block at wbuf + 64 j, its 16-byte chunk q stored
// at chunk slot q ^ ((j >> 2) & 3), so the four ds_read_b128 of a block are
// bank-conflict free (every 16-lane ds_read_b128 group hits 16 distinct
// 16-byte bank slots).  DMA instruction k (k = 0..3) fills values
// 16k .. 16k+15: lane l loads chunk (l & 3) ^ ((l >> 4) & 3) of value
// 16k + (l >> 2), which lands at wbuf + 1024 k + 16 l -- exactly its slot.
//
// src[k] = chunk address of block 0 for this lane's DMA role k; nf[k] = full
// blocks of that value (0 for a dead lane).  my_nfull: this lane's own value.
// Wave reductions by ds_swizzle (xor pattern in the instruction, within each
// 32-lane half) and two readlanes: no lane-index VGPRs, which __shfl_xor
// computes once and the compiler then keeps live through a whole kernel.
template <int X>
__device__ __forceinline__ uint32_t swz_xor(uint32_t v) {
    return uint32_t(__builtin_amdgcn_ds_swizzle(int(v), (X << 10) | 0x1F));
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
    v = max(v, swz_xor<1>(v));
    v = max(v, swz_xor<2>(v));
    v = max(v, swz_xor<4>(v));
    v = max(v, swz_xor<8>(v));
    v = max(v, swz_xor<16>(v));
    return max(uint32_t(__builtin_amdgcn_readlane(int(v), 0)), uint32_t(__builtin_amdgcn_readlane(int(v), 32)));
}

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
    v = min(v, swz_xor<1>(v));
    v = min(v, swz_xor<2>(v));
    v = min(v, swz_xor<4>(v));
    v = min(v, swz_xor<8>(v));
    v = min(v, swz_xor<16>(v));
    return min(uint32_t(__builtin_amdgcn_readlane(int(v), 0)), uint32_t(__builtin_amdgcn_readlane(int(v), 32)));
}

template <int X>
__device__ __forceinline__ uint64_t min_swz64(uint64_t v) {
    const uint64_t u = (uint64_t(swz_xor<X>(uint32_t(v >> 32))) << 32) | swz_xor<X>(uint32_t(v));
    return u < v ? u : v;
}
__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v) {
    v = min_swz64<1>(v);
    v = min_swz64<2>(v);
    v = min_swz64<4>(v);
    v = min_swz64<8>(v);
    v = min_swz64<16>(v);
    const uint64_t a = (uint64_t(uint32_t(__builtin_amdgcn_readlane(int(uint32_t(v >> 32)), 0))) << 32) |
                       uint32_t(__builtin_amdgcn_readlane(int(uint32_t(v)), 0));
    const uint64_t b = (uint64_t(uint32_t(__builtin_amdgcn_readlane(int(uint32_t(v >> 32)), 32))) << 32) |
                       uint32_t(__builtin_amdgcn_readlane(int(uint32_t(v)), 32));
    return a < b ? a : b;
}

// issue(b) starts the four DMA instructions of block b (each lane for its DMA
// role); nmax = the wave's largest full-block count (wave-uniform).  raw(c, w)
// sees each of this lane's blocks as loaded (four little-endian quads) and as
// the 16 big-endian words SHA-1 takes (k_leaf_verify checksums them there);
// be(w), for the stages that only form the big-endian words.
struct NoRaw {
    __device__ __forceinline__ void operator()(const uint4*, const uint32_t*) const {}
    __device__ __forceinline__ void be(const uint32_t*) const {}
    __device__ __forceinline__ void tail(const uint32_t*, uint32_t) const {}
};

template <class Issue, class Raw = NoRaw>
__device__ __forceinline__ void sha1_blocks_lds(const uint8_t* wbuf, uint32_t nmax, uint32_t my_nfull,
                                                Issue issue, uint32_t h[5], Raw raw = Raw{}) {
    const int lane = threadIdx.x & 63;
    const uint4* rd = reinterpret_cast<const uint4*>(wbuf + 64 * lane);
    const uint32_t swz = (uint32_t(lane) >> 2) & 3u;
    uint32_t w[16];
    if (nmax == 0) return;
    issue(0u);
    for (uint32_t b = 0; b < nmax; ++b) {
        // block b's DMA has landed.  Explicit: the compiler's own LDS-DMA wait
        // depends on its alias analysis of the stage (a second __shared__
        // object in the kernel once made it drop this wait).
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        uint4 c[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) c[q] = rd[q ^ swz];
        be16_from_raw(c, w);
        if (b + 1 < nmax) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // stage reads done before refill
            issue(b + 1);
        }
        if (b < my_nfull) {
            raw(c, w);
            sha1_compress(h, w);
        }
    }
}

// Full blocks in runs of S blocks: each lane loads S*64 contiguous bytes of its
// value (4S x global_load_dwordx4) before compressing them, so every request
// stream touches a DRAM page for a longer run.
template <int S>
__device__ __forceinline__ void sha1_blocks_runs(const uint8_t* p, uint32_t nfull, uint32_t h[5]) {
    const uint4* q = reinterpret_cast<const uint4*>(p);
    uint32_t w[16];
    uint32_t b = 0;
    for (; b + S <= nfull; b += S) {
        uint4 c[4 * S];
#pragma unroll
        for (int i = 0; i < 4 * S; ++i) c[i] = q[4 * b + i];
#pragma unroll
        for (int j = 0; j < S; ++j) {
            be16_from_raw(c + 4 * j, w);
            sha1_compress(h, w);
        }
    }
    for (; b < nfull; ++b) {
        uint4 c[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) c[i] = q[4 * b + i];
        be16_from_raw(c, w);
        sha1_compress(h, w);
    }
}

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ u32x4 ds_read_b128_asm(uint32_t addr) {
    u32x4 v;
    asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(addr) : "memory");
    return v;
}
template <int OFF>
__device__ __forceinline__ u32x4 ds_read_b128_off(uint32_t addr) {
    u32x4 v;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "i"(OFF) : "memory");
    return v;
}

template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    if constexpr (N == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    else if constexpr (N == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    else if constexpr (N == 12) asm volatile("s_waitcnt vmcnt(12)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// Pipelined ring over VALUE-relative chunks: chunk c of a value is its bytes
// [64c, 64c + 64), fetched by LDS-DMA from the value's own (unaligned) address,
// so the LDS row already holds block c and no funnel is needed (16 v_perm
// byte swaps per block instead of 52).  Only full blocks are fetched, so every
// byte read belongs to the value.  A lane past its value's last block re-reads
// that block (a value with none re-reads another of the wave), so each issue is four
// wave-instructions.  Window b = chunk b; at block b the ring holds chunks
// b+1 .. b+R, and vmcnt(4 (R-1)) before reading window b+1 lets chunks
// b+2 .. b+R fly (R-1 blocks of lookahead).
// sink(b, w): block b's 16 big-endian words (clobbered), every lane, every
// b < the wave's longest value (sha1_blocks_ring_vc compresses the lane's own)
template <int R, class Sink>
__device__ __forceinline__ void ring_vc_blocks(uint8_t* wbuf, const uint8_t* p, uint32_t my_nfull, Sink&& sink) {
    static_assert(R >= 2 && R <= 4, "ring depth");
    const int lane = threadIdx.x & 63;
    // DMA role k of this lane: chunk (lane & 3) of value 16 k + (lane >> 2),
    // which lands at wbuf + 1024 k + 16 lane = row 64 j + 16 (lane & 3): rows
    // unswizzled, so a lane reads its window at one base + immediate offsets
    // (the 4-way bank conflicts cost LDS cycles the VALU-bound loop has spare)
    const uint32_t dq = uint32_t(lane) & 3u;
    const uint32_t nmax = wave_max_u32(my_nfull);
    if (nmax == 0) return;
    // wave base: the lowest value address among lanes with a full block
    const uint64_t pa = reinterpret_cast<uintptr_t>(p);
    const uint64_t wb = wave_min_u64(my_nfull ? pa : ~uint64_t(0));
    const uint32_t minfull = wave_min_u32(my_nfull ? my_nfull : 0xFFFFFFFFu);
    const uint32_t wb_nfull = wave_max_u32(my_nfull && pa == wb ? my_nfull : 0u);
    uint64_t relk[4];
    uint32_t lastk[4];  // byte offset of the role value's last full block
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int j = 16 * k + (lane >> 2);
        const uint64_t aj = uint64_t(__shfl(int64_t(pa), j));
        const uint32_t nj = uint32_t(__shfl(int(my_nfull), j));
        // a role whose value has no full block re-reads the wave base's value
        relk[k] = (nj ? aj - wb : 0ull) + 16u * dq;
        lastk[k] = 64u * ((nj ? nj : wb_nfull) - 1u);
    }
    const uint8_t* base = reinterpret_cast<const uint8_t*>(wb);
    // near: every 16-byte request ends inside the descriptor's 0xFFFFFFFF bytes
    // (one that reaches past them is out of range and delivers zeros)
    const bool near = __all(relk[0] + lastk[0] + 16ull <= 0xFFFFFFFFull && relk[1] + lastk[1] + 16ull <= 0xFFFFFFFFull &&
                            relk[2] + lastk[2] + 16ull <= 0xFFFFFFFFull && relk[3] + lastk[3] + 16ull <= 0xFFFFFFFFull);
    uint32_t rel[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) rel[k] = uint32_t(relk[k]);
    // Chunk c: while every live value still has block c (c < minfull) the
    // offsets are the per-role constants rel[k] from the uniform base + 64 c
    // (saddr-form DMA, no VALU); past that, each role clamps to its value's
    // last full block (a lane past its value re-reads it; rel + min(64 c, last)
    // stays below the near bound, where rel + 64 c could wrap).  Waves whose
    // values lie more than 4 GiB apart take 64-bit addresses throughout
    // (tests/test_gpu_far.py holds both sides of the bound).
    // buffer descriptor over [wb, wb + 4 GiB): the uniform chunk offset rides
    // in soffset, so the in-range issue has no VALU at all
    const __amdgpu_buffer_rsrc_t rsrc =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(base), short(0), int(0xFFFFFFFF), 0x00020000);
    auto issue = [&](uint32_t c) {
        uint8_t* dst = wbuf + 4096 * (c % R);
        const uint32_t cb = 64u * c;
        if (near && c < minfull) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(
                    rsrc, (__attribute__((address_space(3))) void*)(dst + 1024 * k), 16, rel[k],
                    int(cb), 0, 0);
        } else if (near) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(
                    rsrc, (__attribute__((address_space(3))) void*)(dst + 1024 * k), 16,
                    rel[k] + min(cb, lastk[k]), 0, 0, 0);  // at most rel + last: no 32-bit wrap
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                __builtin_amdgcn_global_load_lds(base + (relk[k] + min(cb, lastk[k])), dst + 1024 * k, 16, 0, 0);
        }
    };
    const uint32_t row = uint32_t(reinterpret_cast<uintptr_t>(wbuf)) + 64u * uint32_t(lane);
    auto read_window = [&](uint32_t b, u32x4 v[4]) {
        const uint32_t s0 = row + 4096u * (b % R);  // one VALU; the chunks at immediate offsets
        v[0] = ds_read_b128_off<0>(s0);
        v[1] = ds_read_b128_off<16>(s0);
        v[2] = ds_read_b128_off<32>(s0);
        v[3] = ds_read_b128_off<48>(s0);
    };
    // block b from cur while window b+1 lands in nxt; the loop below runs it
    // twice per iteration with the roles swapped, so no window is copied
    auto step = [&](uint32_t b, u32x4 cur[4], u32x4 nxt[4]) {
        issue(b + R);
        wait_vmcnt<4 * (R - 1)>();
        read_window(b + 1, nxt);
        uint4 c4[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) c4[q] = make_uint4(cur[q].x, cur[q].y, cur[q].z, cur[q].w);
        uint32_t w[16];
        be16_from_raw(c4, w);
        sink(b, w);
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(nxt[0]), "+v"(nxt[1]), "+v"(nxt[2]), "+v"(nxt[3]) : : "memory");
    };
#pragma unroll
    for (uint32_t c = 0; c < uint32_t(R); ++c) issue(c);
    wait_vmcnt<4 * (R - 1)>();
    u32x4 wa[4], wb4[4];
    read_window(0u, wa);
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(wa[0]), "+v"(wa[1]), "+v"(wa[2]), "+v"(wa[3]) : : "memory");
    uint32_t b = 0;
    for (; b + 2 <= nmax; b += 2) {
        step(b, wa, wb4);
        step(b + 1, wb4, wa);
    }
    if (b < nmax) step(b, wa, wb4);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

template <int R>
__device__ __forceinline__ void sha1_blocks_ring_vc(uint8_t* wbuf, const uint8_t* p, uint32_t my_nfull,
                                                    uint32_t h[5]) {
    ring_vc_blocks<R>(wbuf, p, my_nfull, [&](uint32_t b, uint32_t w[16]) {
        // the live lanes only: compressing in every lane (into a copy a lane
        // past its value drops) measured no faster on configs[2] and ran the
        // clock 1-2 % lower (profiles/r06_ab_ring_lanes.txt): its sorted groups
        // keep waves nearly full, unlike the small trees (sha1_value_all_lanes)
        if (b < my_nfull) sha1_compress(h, w);
    });
}

// The 80-byte window stage for values that are not 64-byte aligned and whose
// full-block counts are equal across the wave (records of one size whose
// offsets mod 64 differ).  Block b of a value at o = p & 63 lies in the five
// aligned quads from (p & ~15) + 64 b; five LDS-DMA instructions per block
// fetch them for all 64 values (quad g = 64 k + l of instruction k is quad
// g % 5 of value g / 5; quads past o + 63 are clamped to the last needed one,
// so every request is aligned, inside one line, and inside a line that holds
// bytes of the value's block).  Value j's row is 80 contiguous bytes at wbuf +
// 80 j, and the lane reads its 64-byte window with four byte-unaligned
// ds_read_b128 at 80 j + (o & 15): no register funnel, 16 v_perm per block as
// in the aligned path.  The addresses are a 32-bit offset per role from a
// wave-uniform base plus the uniform 64 b (the wave's rows must lie within 4
// GiB of the base).  Stage: 5 KiB per wave (eight waves per SIMD fit the 160 KiB
// LDS).  Returns false, doing nothing, when the wave does not qualify; the
// caller then runs the value-relative stream.
__device__ __forceinline__ bool sha1_blocks_pair(uint8_t* wbuf, const uint8_t* p, bool live, uint32_t my_nfull,
                                                 uint32_t h[5]) {
    constexpr int kDma = 5;  // DMA instructions per block
    constexpr uint32_t kRow = 80u;
    const int lane = threadIdx.x & 63;
    const uint32_t nmax = wave_max_u32(live ? my_nfull : 0u);
    if (nmax == 0) return true;  // no live value has a full block
    if (!__all(!live || my_nfull == nmax)) return false;
    const uint64_t a = reinterpret_cast<uintptr_t>(p) & ~uint64_t(63);
    const uint64_t wb = wave_min_u64(live ? a : ~uint64_t(0));
    const uint64_t rel = live ? a - wb : 0u;
    if (!__all(rel + 64ull * (uint64_t(nmax) + 1ull) <= 0xFFFFFFFFull)) return false;
    const uint32_t o = live ? uint32_t(reinterpret_cast<uintptr_t>(p) & 63u) : 0u;
    const uint8_t* base = reinterpret_cast<const uint8_t*>(wb);
    // lane 0 is live whenever any lane is (dead lanes are the grid's tail), so
    // dead values' roles re-read lane 0's quads into their unused rows
    uint32_t voff[kDma];
#pragma unroll
    for (int k = 0; k < kDma; ++k) {
        const uint32_t g = 64u * uint32_t(k) + uint32_t(lane);
        const int j = int(g / 5u);
        const uint32_t qi = g - 5u * uint32_t(j);
        const bool lj = __shfl(int(live), j) != 0;
        const uint32_t src = lj ? uint32_t(j) : 0u;
        const uint32_t rj = uint32_t(__shfl(int(uint32_t(rel)), int(src)));
        const uint32_t oj = uint32_t(__shfl(int(o), int(src)));
        const uint32_t qlast = (oj + 63u) >> 4;
        voff[k] = rj + 16u * min((oj >> 4) + qi, qlast);
    }
    auto issue = [&](uint32_t b) {
        const uint32_t cb = 64u * b;
#pragma unroll
        for (int k = 0; k < kDma; ++k) __builtin_amdgcn_global_load_lds(base + (voff[k] + cb), wbuf + 1024 * k, 16, 0, 0);
    };
    const uint32_t rd = uint32_t(reinterpret_cast<uintptr_t>(wbuf)) + kRow * uint32_t(lane) + (o & 15u);
    issue(0u);
    for (uint32_t b = 0; b < nmax; ++b) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        u32x4 v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = ds_read_b128_asm(rd + 16u * uint32_t(q));
        asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]) : : "memory");
        if (b + 1 < nmax) issue(b + 1);
        uint4 c4[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) c4[q] = make_uint4(v[q].x, v[q].y, v[q].z, v[q].w);
        uint32_t w[16];
        be16_from_raw(c4, w);
        if (live) sha1_compress(h, w);
    }
    return true;
}

// LOAD 11: values that share one misalignment o = (address mod 64) != 0
// across the wave (Data-table records of one size: Value at rec + 30 + KeySize,
// record.go:191-199).  Each lane streams its value's 64-byte ALIGNED segments
// straight into registers, in order, once: block b's window is bytes
// [o, o + 64) of segments b, b + 1, so segment b + 1 is loaded for block b and
// kept for block b + 1 (two register sets swap roles; the loop is unrolled by
// two).  The L2 then sees every 128-byte line requested by one lane in two
// consecutive blocks, as for 64-byte aligned values, where the window stages
// (LOAD 8/9/10) request each line in three consecutive blocks and the line
// falls out of the 4 MiB L2 in between (records form).
// The funnel is the 16 v_perm_b32 byte swaps the aligned path runs anyway: o is
// wave-uniform, so the dword offset o >> 2 selects one of 16 straight-line
// register patterns (scalar branch) and the byte offset o & 3 is the v_perm
// selector (an SGPR).  Every segment loaded holds a byte of the value's full
// blocks, so no load steps past the value's last full block (no page beyond
// the buffer is touched).  No LDS.  Returns false (and does nothing) when the
// wave's live values do not share o, or o == 0.
template <int Q>
__device__ __forceinline__ void funnel_q(const uint32_t a[16], const uint32_t b[16], uint32_t sel, uint32_t w[16]) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int j = Q + i;  // dword j of the 32-dword pair (a, b): the window's dword i
        const uint32_t lo = j < 16 ? a[j] : b[j - 16];
        const uint32_t hi = j + 1 < 16 ? a[j + 1] : b[j - 15];
        w[i] = be_word(hi, lo, sel);
    }
}

__device__ __forceinline__ void funnel_u(uint32_t q, const uint32_t a[16], const uint32_t b[16], uint32_t sel,
                                         uint32_t w[16]) {
    switch (q) {
        case 0: funnel_q<0>(a, b, sel, w); break;
        case 1: funnel_q<1>(a, b, sel, w); break;
        case 2: funnel_q<2>(a, b, sel, w); break;
        case 3: funnel_q<3>(a, b, sel, w); break;
        case 4: funnel_q<4>(a, b, sel, w); break;
        case 5: funnel_q<5>(a, b, sel, w); break;
        case 6: funnel_q<6>(a, b, sel, w); break;
        case 7: funnel_q<7>(a, b, sel, w); break;
        case 8: funnel_q<8>(a, b, sel, w); break;
        case 9: funnel_q<9>(a, b, sel, w); break;
        case 10: funnel_q<10>(a, b, sel, w); break;
        case 11: funnel_q<11>(a, b, sel, w); break;
        case 12: funnel_q<12>(a, b, sel, w); break;
        case 13: funnel_q<13>(a, b, sel, w); break;
        case 14: funnel_q<14>(a, b, sel, w); break;
        default: funnel_q<15>(a, b, sel, w); break;
    }
}

__device__ __forceinline__ void load_seg(const uint4* s, uint32_t r[16]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const uint4 v = s[q];
        r[4 * q + 0] = v.x;
        r[4 * q + 1] = v.y;
        r[4 * q + 2] = v.z;
        r[4 * q + 3] = v.w;
    }
}

// LINES: whole 128-byte lines into registers when the values' segments start
// lines (the caller's kernel must afford ~86 VGPRs: k_leaf_records runs 5
// waves per SIMD); else the LDS-DMA stage or 64-byte register segments.
template <class Hook = NoRaw, bool LINES = false>
__device__ __forceinline__ bool sha1_blocks_shift(uint8_t* wbuf, const uint8_t* p, bool live, uint32_t my_nfull,
                                                  uint32_t h[5], Hook hook = Hook{}) {
    const uint32_t o = live ? uint32_t(reinterpret_cast<uintptr_t>(p) & 63u) : 0u;
    // lane 0 is live whenever any lane is (dead lanes are the grid's tail)
    const uint32_t o0 = __builtin_amdgcn_readfirstlane(o);
    if (o0 == 0u || !__all(!live || o == o0)) return false;
    const uint32_t nmax = wave_max_u32(live ? my_nfull : 0u);
    if (nmax == 0) return true;
    const uint32_t q = o0 >> 2;
    const uint32_t sel = be_sel(o0 & 3u);
    uint32_t a[16], b[16], w[16];
    // Whole 128-byte lines into registers: when every live value's segment 0
    // starts a line and the block counts are equal, each lane loads its aligned
    // lines (two segments, eight 16-byte loads) once, no LDS.  Three segment
    // sets rotate over four blocks: block k takes segments k and k + 1.  Every
    // line loaded holds a needed segment, so no load leaves the value's pages.
    if (LINES && __all(!live || my_nfull == nmax) &&
        __all(!live || ((reinterpret_cast<uintptr_t>(p) - o) & 64u) == 0u)) {
        const uint4* seg = reinterpret_cast<const uint4*>(live ? p - o : p);
        uint32_t c[16];
        auto line = [&](uint32_t sg, uint32_t x[16], uint32_t y[16]) {
            if (live) {
                load_seg(seg + 4 * sg, x);
                load_seg(seg + 4 * (sg + 1), y);
            }
        };
        auto block = [&](const uint32_t lo[16], const uint32_t hi[16]) {
            funnel_u(q, lo, hi, sel, w);
            if (live) {
                hook.be(w);
                sha1_compress(h, w);
            }
            asm volatile("" ::: "memory");  // the next line's loads stay after this compress
        };
        line(0u, a, b);
        for (uint32_t k = 0; k < nmax; k += 4) {
            block(a, b);  // segments k, k + 1
            if (k + 1 >= nmax) break;
            line(k + 2, a, c);
            block(b, a);  // k + 1, k + 2
            if (k + 2 >= nmax) break;
            block(a, c);  // k + 2, k + 3
            if (k + 3 >= nmax) break;
            line(k + 4, a, b);
            block(c, a);  // k + 3, k + 4
        }
        return true;
    }
    if (wbuf && __all(!live || my_nfull == nmax)) {
        // Equal block counts: the segments go HBM -> LDS by LDS-DMA, one segment
        // of lookahead, in k_leaf's aligned stage layout (value j's segment at
        // wbuf + 64 j, chunks XOR-swizzled; sha1_blocks_lds), then into the
        // register pair.  32-bit offsets from a wave-uniform base (one VGPR per
        // DMA role) keep the register pair and the schedule within 64 VGPRs.
        const uint64_t sa = reinterpret_cast<uintptr_t>(p) - o;
        const uint64_t wb = wave_min_u64(live ? sa : ~uint64_t(0));
        const uint64_t rel = live ? sa - wb : 0u;
        if (__all(rel + 64ull * (uint64_t(nmax) + 1ull) <= 0xFFFFFFFFull)) {
            const int lane = threadIdx.x & 63;
            const uint8_t* base = reinterpret_cast<const uint8_t*>(wb);
            const uint32_t cq = (uint32_t(lane) & 3u) ^ ((uint32_t(lane) >> 4) & 3u);
            uint32_t voff[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                // dead values' roles re-read lane 0's segments into unused rows
                const int j = 16 * k + (lane >> 2);
                const bool lj = __shfl(int(live), j) != 0;
                voff[k] = uint32_t(__shfl(int(uint32_t(rel)), lj ? j : 0)) + 16u * cq;
            }
            auto issue = [&](uint32_t sg) {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    __builtin_amdgcn_global_load_lds(base + (voff[k] + 64u * sg), wbuf + 1024 * k, 16, 0, 0);
            };
            // chunk c of this lane's segment sits at (wbuf + 64 lane) + 16 (c ^ swz)
            // = rd0 ^ 16 c with rd0 = wbuf + 64 lane + 16 swz (64-B aligned rows).
            // One address VGPR, the other three are recomputed per read (the
            // asm hides rd0 from hoisting: four live addresses spill at 64 VGPRs)
            const uint32_t rd0 = uint32_t(reinterpret_cast<uintptr_t>(wbuf)) + 64u * uint32_t(lane) +
                                 16u * ((uint32_t(lane) >> 2) & 3u);
            auto take = [&](uint32_t r[16]) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                uint32_t ra = rd0;
                asm volatile("" : "+v"(ra));
                u32x4 v[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) v[c] = ds_read_b128_asm(ra ^ (16u * uint32_t(c)));
                // stage read before its refill; the in/out operands keep the
                // registers from being used before the wait
                asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]) : : "memory");
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    r[4 * c + 0] = v[c].x;
                    r[4 * c + 1] = v[c].y;
                    r[4 * c + 2] = v[c].z;
                    r[4 * c + 3] = v[c].w;
                }
            };
            // segments 0 .. nmax (block k's window spans segments k and k + 1)
            issue(0u);
            take(a);
            issue(1u);
            // sched_barrier: no instruction crosses a phase boundary, so the
            // scheduler cannot overlap one block's compression with the next
            // block's reads and funnel (two windows live at 64 VGPRs spill)
            for (uint32_t k = 0; k < nmax; k += 2) {
                take(b);  // segment k + 1
                if (k + 2 <= nmax) issue(k + 2);
                funnel_u(q, a, b, sel, w);
                __builtin_amdgcn_sched_barrier(0);
                if (live) {
                    hook.be(w);
                    sha1_compress(h, w);
                }
                __builtin_amdgcn_sched_barrier(0);
                if (k + 1 >= nmax) break;
                take(a);  // segment k + 2
                if (k + 3 <= nmax) issue(k + 3);
                funnel_u(q, b, a, sel, w);
                __builtin_amdgcn_sched_barrier(0);
                if (live) {
                    hook.be(w);
                    sha1_compress(h, w);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            return true;
        }
    }
    // p - o, not an integer-to-pointer cast: stays in the global address space
    const uint4* seg = reinterpret_cast<const uint4*>(live ? p - o : p);
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        a[i] = 0u;
        b[i] = 0u;
    }
    if (my_nfull) load_seg(seg, a);
    for (uint32_t k = 0; k < nmax; k += 2) {
        // block k: segments k (a) and k + 1 (b)
        if (k < my_nfull) load_seg(seg + 4 * (k + 1), b);
        funnel_u(q, a, b, sel, w);
        if (k < my_nfull) {
            hook.be(w);
            sha1_compress(h, w);
        }
        // keep each load after the previous compress: hoisted above it, a
        // segment set would be live through the compress and spill at 64 VGPRs
        // (the other resident waves cover the load latency)
        asm volatile("" ::: "memory");
        if (k + 1 >= nmax) break;
        // block k + 1: segments k + 1 (b) and k + 2 (a)
        if (k + 1 < my_nfull) load_seg(seg + 4 * (k + 2), a);
        funnel_u(q, b, a, sel, w);
        if (k + 1 < my_nfull) {
            hook.be(w);
            sha1_compress(h, w);
        }
        asm volatile("" ::: "memory");
    }
    return true;
}

// The full blocks of a wave's 64 values at any addresses (wbuf: the wave's
// 5 KiB of LDS): the segment stage when the values share their offset mod 64,
// else the 80-byte window stage when their full-block counts are equal, else
// the value-relative stream.  k_leaf's LOAD 11 for MODE 1 and k_leaf_records.
template <bool LINES = false>
__device__ __forceinline__ void sha1_blocks_any(uint8_t* wbuf, const uint8_t* p, bool live, uint32_t my_nfull,
                                                uint32_t h[5]) {
    if (sha1_blocks_shift<NoRaw, LINES>(wbuf, p, live, my_nfull, h)) return;
    if (sha1_blocks_pair(wbuf, p, live, my_nfull, h)) return;
    const int lane = threadIdx.x & 63;
    const uint32_t q = (uint32_t(lane) & 3u) ^ ((uint32_t(lane) >> 4) & 3u);
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
    sha1_blocks_lds(wbuf, wave_max_u32(my_nfull), my_nfull, issue, h);
}

}  // namespace nkv
