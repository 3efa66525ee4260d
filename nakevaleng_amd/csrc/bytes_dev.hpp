// bytes_dev.hpp -- byte movers and searches of the record kernels (merge.hip,
// memtable.hip, index.hip, lookup.hip, encode.hip and merge_copy_dev.hpp): 16
// source bytes at any alignment out of aligned 16-byte loads, a header's two
// size fields out of aligned 8-byte loads, searches in an ascending array by
// one lane and by a workgroup, and the scan's total.  The record format itself
// and the key order are record_dev.hpp's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "internal.hpp"  // kBlock; record_dev.hpp

namespace nkv {

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

// KeySize and ValueSize (header bytes 14..29, record.go:191-199) of the
// record at p, from two or three aligned 8-byte loads and a funnel shift
// instead of sixteen byte loads (one line request per lane per load rather
// than one per byte).  The third load is issued only when the fields are
// not 8-byte aligned; it then holds byte 29, so every load stays inside an
// aligned word that holds a header byte (no page can be crossed).  The header
// reader of the leaf and locate kernels (leaf.hip, plan.hip).
__device__ __forceinline__ void ld_header_sizes(const uint8_t* p, uint64_t& ks, uint64_t& vs) {
    // pointer arithmetic on p (not an integer-to-pointer cast) keeps the global
    // address space: global_load, not flat_load
    const uint8_t* f = p + 14;
    const uint32_t mis = uint32_t(reinterpret_cast<uintptr_t>(f) & 7u);
    const uint64_t* q = reinterpret_cast<const uint64_t*>(f - mis);
    const uint32_t sh = mis * 8u;
    const uint64_t q0 = q[0], q1 = q[1];
    const uint64_t q2 = sh ? q[2] : 0ull;
    ks = sh ? (q0 >> sh) | (q1 << (64u - sh)) : q0;
    vs = sh ? (q1 >> sh) | (q2 << (64u - sh)) : q1;
}

// The last index j in [lo, hi) with a[j] <= x; a ascending, a[lo] <= x.  The
// index type is the caller's: 32 bits where the array is a list in LDS.
template <class A, class I>
__device__ __forceinline__ I last_at_most(const A& a, I lo, I hi, uint64_t x) {
    while (hi - lo > 1) {
        const I mid = lo + (hi - lo) / 2;
        if (a[mid] <= x) lo = mid;
        else hi = mid;
    }
    return lo;
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

// Behind an exclusive scan of n sizes into off: off[n] = the total, and the
// total next to the error word for the host.  A template, so that only the
// translation units that launch it carry a copy.
template <class T>
__global__ void k_scan_total(const T* __restrict__ size, T* __restrict__ off, uint64_t n, T* __restrict__ total) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    off[n] = off[n - 1] + size[n - 1];
    *total = off[n];
}

}  // namespace nkv
