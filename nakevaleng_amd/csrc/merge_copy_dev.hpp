// merge_copy_dev.hpp -- the tail shared by the compaction merge (merge.hip)
// and the memtable flush (memtable.hip): both arrive at a flag, a size and a
// source word per slot, and from there compact them, list output offsets and
// source addresses and move the bytes the same way (write_table).  The kernels
// have internal linkage, so each translation unit that includes this header
// gets its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bytes_dev.hpp"  // ld16_any
#include "context.hpp"

namespace nkv {
namespace {

constexpr uint32_t kCopyTile = 16384;  // output bytes per workgroup
constexpr uint32_t kCopyChunk = 16;    // output bytes per lane and step
// records that can overlap one tile: at most kCopyTile / kHdr + 2 = 548
constexpr uint32_t kCopyList = 640;
static_assert(kCopyTile / kHdr + 2 <= kCopyList, "a tile's records fit the list");

// Per-slot arrays of n entries each, carved in this order.
struct Slots {
    uint64_t* flag;      // 1: the slot holds a surviving record
    uint64_t* osize;     // its TotalSize (0 where flag is 0)
    uint64_t* osrc;      // its source word
    uint64_t* idx;       // exclusive sum of flag: the output index
    uint64_t* ooff;      // exclusive sum of osize: the output offset
    uint64_t* src_addr;  // per output record: where its bytes lie
};
inline Slots take_slots(Carver& k, uint64_t n) {
    return Slots{k.take<uint64_t>(n), k.take<uint64_t>(n), k.take<uint64_t>(n),
                 k.take<uint64_t>(n), k.take<uint64_t>(n), k.take<uint64_t>(n)};
}

// One lane per slot: a surviving slot writes its output offset, its source
// word (out_src nullable) and its record's address, which `in` makes of the
// source word (in.record_at(w)); the last lane leaves totals = (n_out, out_len).
template <class In>
__device__ __forceinline__ void scatter_slots(const In& in, uint32_t n, const uint64_t* __restrict__ flag,
                                              const uint64_t* __restrict__ idx, const uint64_t* __restrict__ osize,
                                              const uint64_t* __restrict__ ooff, const uint64_t* __restrict__ osrc,
                                              uint64_t* __restrict__ out_off, uint64_t* __restrict__ out_src,
                                              uint64_t* __restrict__ src_addr, uint64_t* __restrict__ totals) {
    const uint64_t s = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (s >= n) return;
    if (flag[s]) {
        const uint64_t j = idx[s], w = osrc[s];
        out_off[j] = ooff[s];
        if (out_src) out_src[j] = w;
        src_addr[j] = uint64_t(reinterpret_cast<uintptr_t>(in.record_at(w)));
    }
    if (s == n - 1) {
        totals[0] = idx[s] + flag[s];
        totals[1] = ooff[s] + osize[s];
    }
}

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

// Behind the kernels that fill S.flag / S.osize / S.osrc: the two scans, the
// caller's scatter kernel (its arguments after the input and n are the ones
// given here), the copy over `tiles` tiles of d_out, and (n_out, out_len) read
// back.  With NKV_TIMING_EVENTS "reduce" is the copy kernel.  tmp: the scan's
// temporary of tb bytes.
template <class Kernel, class In>
int write_table(nkv_ctx* c, Kernel scatter, const In& in, uint64_t n, const Slots& S, void* tmp, size_t tb,
                uint64_t tiles, void* d_out, uint64_t* d_out_off, uint64_t* d_out_src, uint64_t* totals,
                uint64_t* n_out, uint64_t* out_len) {
    HIPTRY(scan_exclusive_u64(S.flag, S.idx, n, tmp, &tb, c->stream));
    HIPTRY(scan_exclusive_u64(S.osize, S.ooff, n, tmp, &tb, c->stream));
    hipLaunchKernelGGL(scatter, dim3(blocks_for(n)), dim3(kBlock), 0, c->stream, in, uint32_t(n), S.flag, S.idx,
                       S.osize, S.ooff, S.osrc, d_out_off, d_out_src, S.src_addr, totals);
    HIPTRY(hipGetLastError());
    TRY(mark(c, 1));
    // out_len is known on the device only: the grid covers the bound (the
    // bytes of the input), and tiles past out_len leave at once
    hipLaunchKernelGGL(k_merge_copy, dim3(unsigned(tiles)), dim3(kBlock), 0, c->stream, static_cast<uint8_t*>(d_out),
                       d_out_off, S.src_addr, totals);
    HIPTRY(hipGetLastError());
    TRY(mark(c, 2));
    uint64_t h_tot[2] = {0, 0};
    HIPTRY(hipMemcpyAsync(h_tot, totals, 16, hipMemcpyDeviceToHost, c->stream));
    HIPTRY(hipStreamSynchronize(c->stream));
    *n_out = h_tot[0];
    *out_len = h_tot[1];
    return NKV_OK;
}

}  // namespace
}  // namespace nkv
