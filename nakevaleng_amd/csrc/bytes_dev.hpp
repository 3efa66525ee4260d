// bytes_dev.hpp -- helpers of the record kernels (merge.hip, index.hip,
// lookup.hip): fields and keys at any alignment, 16 source bytes at any
// alignment out of aligned 16-byte loads, and a workgroup's search in an
// ascending array.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "internal.hpp"  // kBlock

namespace nkv {

__device__ __forceinline__ uint64_t ld_le64(const uint8_t* p) {  // any alignment
    uint64_t v = 0;
#pragma unroll
    for (int b = 0; b < 8; ++b) v |= uint64_t(p[b]) << (8 * b);
    return v;
}

// bytes.Compare: unsigned lexicographic, a proper prefix sorts first
__device__ inline int cmp_bytes(const uint8_t* a, uint64_t la, const uint8_t* b, uint64_t lb) {
    const uint64_t m = la < lb ? la : lb;
    for (uint64_t i = 0; i < m; ++i) {
        const uint8_t x = a[i], y = b[i];
        if (x != y) return x < y ? -1 : 1;
    }
    return la < lb ? -1 : (la > lb ? 1 : 0);
}

__device__ __forceinline__ uint32_t sel4(uint32_t q, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    return q == 0 ? a : (q == 1 ? b : (q == 2 ? c : d));
}

// Bytes sh .. sh + 15 of the 32 bytes v (low) : w (high), 0 <= sh <= 15.
__device__ __forceinline__ uint4 funnel16(uint4 v, uint4 w, uint32_t sh) {
    const uint32_t d = sh >> 2, bs = sh & 3;
    const uint32_t x0 = sel4(d, v.x, v.y, v.z, v.w), x1 = sel4(d, v.y, v.z, v.w, w.x),
                   x2 = sel4(d, v.z, v.w, w.x, w.y), x3 = sel4(d, v.w, w.x, w.y, w.z),
                   x4 = sel4(d, w.x, w.y, w.z, w.w);
    return make_uint4(__builtin_amdgcn_alignbyte(x1, x0, bs), __builtin_amdgcn_alignbyte(x2, x1, bs),
                      __builtin_amdgcn_alignbyte(x3, x2, bs), __builtin_amdgcn_alignbyte(x4, x3, bs));
}

// The 16 bytes at address S, read as the one or two aligned 16-byte words that
// hold them (an aligned word with one of the bytes in it cannot cross a page)
// and funnel-shifted.
__device__ __forceinline__ uint4 ld16_any(uint64_t S) {
    const uint32_t sh = uint32_t(S & 15);
    const uint4* q = reinterpret_cast<const uint4*>(uintptr_t(S - sh));
    uint4 v = q[0];
    if (sh) v = funnel16(v, q[1], sh);
    return v;
}

// The cnt bytes at address S (1 <= cnt <= 16) in bytes 0 .. cnt - 1 of the
// result, the rest zero, placed d bytes up (d + cnt <= 16): only aligned words
// that hold one of the bytes are read.
__device__ __forceinline__ uint4 ld_piece(uint64_t S, uint32_t cnt, uint32_t d) {
    const uint32_t sh = uint32_t(S & 15);
    const uint4* q = reinterpret_cast<const uint4*>(uintptr_t(S - sh));
    uint4 v = q[0];
    if (sh) {
        uint4 w = make_uint4(0, 0, 0, 0);
        if (sh + cnt > 16) w = q[1];
        v = funnel16(v, w, sh);
    }
    if (cnt < 16) {
        const int c = int(cnt);
        v.x &= c >= 4 ? ~0u : (1u << (8 * c)) - 1u;
        v.y &= c >= 8 ? ~0u : (c <= 4 ? 0u : (1u << (8 * (c - 4))) - 1u);
        v.z &= c >= 12 ? ~0u : (c <= 8 ? 0u : (1u << (8 * (c - 8))) - 1u);
        v.w &= c <= 12 ? 0u : (1u << (8 * (c - 12))) - 1u;
        if (d) v = funnel16(make_uint4(0, 0, 0, 0), v, 16 - d);
    }
    return v;
}

// The first index in [lo, hi) with a[index] >= key (hi if none), a ascending,
// found by the whole workgroup: every lane probes one of kBlock evenly spaced
// places and the count of probes below the key picks the gap between two of
// them, so a million entries take three dependent loads instead of twenty.
// lo, hi and key must be the same in every lane; so is the result.
__device__ __forceinline__ uint64_t first_at_least(const uint64_t* __restrict__ a, uint64_t lo, uint64_t hi,
                                                   uint64_t key) {
    while (lo < hi) {
        const uint64_t step = (hi - lo + kBlock - 1) / kBlock;
        const uint64_t p = lo + threadIdx.x * step;
        const int c = __syncthreads_count(p < hi && a[p] < key);  // the probes below the key are the first c
        if (c == 0) return lo;
        const uint64_t next = lo + uint64_t(c) * step;  // the first probe not below the key, if it exists
        lo = lo + uint64_t(c - 1) * step + 1;
        hi = next < hi ? next : hi;
    }
    return lo;
}

}  // namespace nkv
