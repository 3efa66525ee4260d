// merge_copy_dev.hpp -- the record copy kernel shared by the compaction merge
// (merge.hip) and the memtable flush (memtable.hip): both end with a list of
// output offsets and source addresses and move the bytes the same way.  The
// kernel has internal linkage, so each translation unit that includes this
// header gets its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bytes_dev.hpp"  // ld16_any

namespace nkv {
namespace {

constexpr uint32_t kCopyTile = 16384;  // output bytes per workgroup
constexpr uint32_t kCopyChunk = 16;    // output bytes per lane and step
// records that can overlap one tile: at most kCopyTile / kHdr + 2 = 548
constexpr uint32_t kCopyList = 640;

// Output byte o of the merged table is byte o - off[j] of the record at
// src[j], for the j with off[j] <= o < off[j + 1].  Chunks lie on the 16-byte
// grid of d_out's address, so every full chunk is one aligned 16-byte store; a
// chunk inside one record is read as the one or two aligned 16-byte source
// words that hold it (an aligned word with one byte of the record in it cannot
// cross a page) and funnel-shifted; a chunk that crosses a record boundary or
// the ends of the output is put together byte by byte.
__global__ __launch_bounds__(kBlock) void k_merge_copy(uint8_t* __restrict__ out, const uint64_t* __restrict__ out_off,
                                                       const uint64_t* __restrict__ src_addr,
                                                       const uint64_t* __restrict__ totals) {
    __shared__ uint64_t l_off[kCopyList + 1];
    __shared__ uint64_t l_src[kCopyList];
    const uint64_t n_out = totals[0], out_len = totals[1];
    const uint64_t head = uint64_t(reinterpret_cast<uintptr_t>(out)) & 15;  // grid position p = o + head
    const uint64_t p0 = uint64_t(blockIdx.x) * kCopyTile, pend = head + out_len;
    if (n_out == 0 || p0 >= pend) return;
    const uint64_t o_lo = p0 > head ? p0 - head : 0;
    const uint64_t o_hi = p0 + kCopyTile < pend ? p0 + kCopyTile - head : out_len;
    // records overlapping [o_lo, o_hi): jlo = the last with off <= o_lo, up to the first with off >= o_hi
    uint64_t lo = 0, hi = n_out;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (out_off[mid] <= o_lo) lo = mid + 1;
        else hi = mid;
    }
    const uint64_t jlo = lo - 1;  // out_off[0] = 0 <= o_lo
    hi = n_out;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (out_off[mid] < o_hi) lo = mid + 1;
        else hi = mid;
    }
    uint32_t cnt = uint32_t(lo - jlo < kCopyList ? lo - jlo : kCopyList);
    for (uint32_t e = threadIdx.x; e < cnt; e += kBlock) {
        l_off[e] = out_off[jlo + e];
        l_src[e] = src_addr[jlo + e];
    }
    if (threadIdx.x == 0) l_off[cnt] = jlo + cnt < n_out ? out_off[jlo + cnt] : out_len;
    __syncthreads();
#pragma unroll 1
    for (uint32_t it = 0; it < kCopyTile / (kCopyChunk * kBlock); ++it) {
        const uint64_t p = p0 + uint64_t(it * kBlock + threadIdx.x) * kCopyChunk;
        if (p + kCopyChunk <= head || p >= pend) continue;
        const uint64_t ob = p > head ? p - head : 0;  // first output byte of the chunk
        uint32_t a = 0, b = cnt;                      // e = the last list entry with off <= ob
        while (b - a > 1) {
            const uint32_t m = (a + b) / 2;
            if (l_off[m] <= ob) a = m;
            else b = m;
        }
        uint32_t e = a;
        const bool whole = p >= head && p + kCopyChunk <= pend;
        if (whole && ob + kCopyChunk <= l_off[e + 1]) {
            const uint64_t S = l_src[e] + (ob - l_off[e]);
            const uint4 v = ld16_any(S);
            *reinterpret_cast<uint4*>(out + ob) = v;
        } else {
            uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
            for (uint32_t k = 0; k < kCopyChunk; ++k) {
                const uint64_t pb = p + k;
                if (pb < head || pb >= pend) continue;
                const uint64_t o = pb - head;
                while (e + 1 < cnt && o >= l_off[e + 1]) ++e;
                const uint8_t byte = *reinterpret_cast<const uint8_t*>(uintptr_t(l_src[e] + (o - l_off[e])));
                if (whole) w[k >> 2] |= uint32_t(byte) << (8 * (k & 3));
                else out[o] = byte;
            }
            if (whole) *reinterpret_cast<uint4*>(out + ob) = make_uint4(w[0], w[1], w[2], w[3]);
        }
    }
}

}  // namespace
}  // namespace nkv
