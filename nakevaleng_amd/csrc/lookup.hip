// lookup.hip -- batched point lookup over device-resident SSTables, the disk
// part of the engine's get (engine/coreeng/coreeng.go:99-160): nkv_lookup_dev /
// nkv_lookup_values_dev.
//
// The reference walks the tables in search order and, per table, runs
// Filter.Query, FindSummaryTableEntry, FindIndexTableEntry and
// record.Deserialize, each over a file it re-opens and scans.  Over a resident
// Data table the Summary and Index steps have a closed form: the Summary
// refuses a key outside [K_0, K_(n-1)], the Index a key that no record holds.
//
//   k_lookup        the search layer's kernel (search_dev.hpp) over the record
//                   format: the key lies behind the 30-byte header, and a found
//                   record answers LIVE or TOMBSTONE.
//   k_value_measure one lane per query: the found record's Value span, checked
//                   against its stream.
//   scan            exclusive sums of the lengths = the packed offsets
//                   (k_scan_total puts the total behind them); the host reads
//                   the total and the verdict before the copy is launched.
//   k_value_copy    tiles the OUTPUT bytes as k_merge_copy does: a workgroup
//                   owns 16 KiB of d_out and every lane writes 16 destination-
//                   aligned bytes per step, put together in registers from
//                   aligned 16-byte loads of the one or more Values that
//                   overlap them.  Values can be empty, so a tile can
//                   overlap any number of queries: up to kCopyList of them are
//                   kept in LDS, more are searched in the offset array itself.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bytes_dev.hpp"
#include "context.hpp"
#include "search_dev.hpp"

using namespace nkv;

namespace {

constexpr uint32_t kCopyTile = 16384;  // output bytes per workgroup
constexpr uint32_t kCopyChunk = 16;    // output bytes per lane and step
constexpr uint32_t kCopyList = 1024;   // queries of a tile kept in LDS

// The entry format of a Data table: a record, its key behind the 30-byte
// header; a found record answers LIVE or TOMBSTONE from its Status byte.
struct RecordFormat {
    static constexpr uint64_t kKeyAt = kHdr;
    static constexpr bool kOverlay = false;
    NKV_HD static bool key_in(const uint8_t* s, uint64_t L, uint64_t o, uint64_t* ks) {
        return key_span_in(s, L, o, ks);
    }
    __device__ bool answer(const uint8_t* rec, uint8_t* st) const {
        *st = status_answer(rec[kAtStatus]);
        return true;
    }
    __device__ void store(uint64_t) const {}
};

__global__ __launch_bounds__(kBlock) void k_lookup(Tables R, const uint8_t* __restrict__ keys,
                                                   const uint64_t* __restrict__ koff,
                                                   const uint64_t* __restrict__ klen, uint64_t q,
                                                   uint64_t* __restrict__ hit, uint8_t* __restrict__ status,
                                                   uint8_t* __restrict__ stage, unsigned int* __restrict__ err) {
    search_tables(R, RecordFormat{}, keys, koff, klen, q, hit, status, stage, err);
}

// len[i] / src[i]: the Value of LIVE hit i (0 bytes for every other query)
__global__ __launch_bounds__(kBlock) void k_value_measure(Tables R, const uint64_t* __restrict__ hit,
                                                          const uint8_t* __restrict__ status, uint64_t q,
                                                          uint64_t* __restrict__ len, uint64_t* __restrict__ src,
                                                          unsigned int* __restrict__ err) {
    const uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= q) return;
    uint64_t vs = 0, at = 0;
    if (status[i] == NKV_GET_LIVE) {
        const uint64_t h = hit[i], t = h >> 32, j = h & 0xFFFFFFFFull;
        bool bad = t >= uint64_t(R.T) || j >= R.n[t < uint64_t(R.T) ? t : 0];
        if (!bad) {
            const uint8_t* s = R.img[t];
            const uint64_t o = R.off[t][j];
            uint64_t ks, v;
            bad = !record_span_in(s, R.len[t], o, &ks, &v);
            if (!bad) {
                vs = v;
                at = uint64_t(reinterpret_cast<uintptr_t>(s + o + kHdr + ks));
            }
        }
        if (bad) atomicOr(err, 1u);
    }
    len[i] = vs;
    src[i] = at;
}

// Output byte o is byte o - off[i] of the Value at src[i], for the i with
// off[i] <= o < off[i + 1] (off holds q + 1 entries, equal neighbours where a
// Value is empty: the last i with off[i] <= o is the one that holds o).  Chunks
// lie on the 16-byte grid of d_out's address, so every full chunk is one
// aligned 16-byte store, OR-ed together from the pieces of the Values that
// overlap it (ld_piece: one or two aligned 16-byte loads per piece, shifted
// and masked in registers); only the partial chunks at the two ends of the
// output go byte by byte.
__global__ __launch_bounds__(kBlock) void k_value_copy(uint8_t* __restrict__ out, const uint64_t* __restrict__ off,
                                                       const uint64_t* __restrict__ src, uint64_t q,
                                                       uint64_t out_len) {
    __shared__ uint64_t l_off[kCopyList + 1];
    __shared__ uint64_t l_src[kCopyList];
    const uint64_t head = uint64_t(reinterpret_cast<uintptr_t>(out)) & 15;  // grid position p = o + head
    const uint64_t p0 = uint64_t(blockIdx.x) * kCopyTile, pend = head + out_len;
    if (p0 >= pend) return;
    const uint64_t o_lo = p0 > head ? p0 - head : 0;
    const uint64_t o_hi = p0 + kCopyTile < pend ? p0 + kCopyTile - head : out_len;  // > o_lo
    // queries holding bytes of [o_lo, o_hi): from jlo, which holds o_lo, to jhi, which holds o_hi - 1
    // (found by the whole workgroup: off[0] = 0 <= o_lo, and jhi is the last with off < o_hi)
    const uint64_t jlo = first_at_least(off, 0, q, o_lo + 1) - 1;
    const uint64_t jhi = first_at_least(off, jlo + 1, q, o_hi) - 1;
    const bool listed = jhi - jlo < kCopyList;  // wave-uniform
    const uint32_t cnt = listed ? uint32_t(jhi - jlo + 1) : 0;
    for (uint32_t e = threadIdx.x; e < cnt; e += kBlock) {
        l_off[e] = off[jlo + e];
        l_src[e] = src[jlo + e];
    }
    if (threadIdx.x == 0) l_off[cnt] = off[jhi + 1];
    __syncthreads();
#pragma unroll 1
    for (uint32_t it = 0; it < kCopyTile / (kCopyChunk * kBlock); ++it) {
        const uint64_t p = p0 + uint64_t(it * kBlock + threadIdx.x) * kCopyChunk;
        if (p + kCopyChunk <= head || p >= pend) continue;
        const uint64_t ob = p > head ? p - head : 0;  // first output byte of the chunk
        const bool whole = p >= head && p + kCopyChunk <= pend;
        // e = the query that holds ob (index into the list, or jlo + e in the arrays)
        const uint64_t e0 = listed ? last_at_most(l_off, uint64_t(0), uint64_t(cnt), ob) : last_at_most(off, jlo, jhi + 1, ob) - jlo;
        const uint64_t off0 = listed ? l_off[e0] : off[jlo + e0];
        const uint64_t off1 = listed ? l_off[e0 + 1] : off[jlo + e0 + 1];
        const uint64_t src0 = listed ? l_src[e0] : src[jlo + e0];
        uint64_t e = e0, a = off0, b = off1, sa = src0;
        if (whole) {  // the pieces of the Values that overlap the chunk, one or two loads each
            uint4 acc = make_uint4(0, 0, 0, 0);
            const uint64_t oe = ob + kCopyChunk;  // <= o_hi: the queries up to jhi hold it all
            uint64_t o = ob;
            for (;;) {
                const uint64_t hi = b < oe ? b : oe;
                if (hi > o) {  // bytes [o, hi) are the Value's from o - a on
                    const uint4 v = ld_piece(sa + (o - a), uint32_t(hi - o), uint32_t(o - ob));
                    acc.x |= v.x;
                    acc.y |= v.y;
                    acc.z |= v.z;
                    acc.w |= v.w;
                    o = hi;
                }
                if (o >= oe) break;
                ++e;
                a = b;
                b = listed ? l_off[e + 1] : off[jlo + e + 1];
                sa = listed ? l_src[e] : src[jlo + e];
            }
            *reinterpret_cast<uint4*>(out + ob) = acc;
        } else {  // the two ends of the output: byte by byte
            for (uint32_t k = 0; k < kCopyChunk; ++k) {
                const uint64_t pb = p + k;
                if (pb < head || pb >= pend) continue;
                const uint64_t o = pb - head;
                while (o >= b) {  // o < out_len = off[q]: ends at the query that holds o
                    ++e;
                    a = b;
                    b = listed ? l_off[e + 1] : off[jlo + e + 1];
                    sa = listed ? l_src[e] : src[jlo + e];
                }
                out[o] = *reinterpret_cast<const uint8_t*>(uintptr_t(sa + (o - a)));
            }
        }
    }
}

// nkv_lookup_table as the search layer reads it
TableView view_of(const nkv_lookup_table& u) {
    return {u.stream, u.stream_len, u.rec_off, u.n, u.bits, u.m, u.k, u.seed0};
}

}  // namespace

extern "C" {

int nkv_lookup_dev(nkv_ctx* c, const nkv_lookup_table* tables, int T, const void* d_keys, const uint64_t* d_koff,
                   const uint64_t* d_klen, uint64_t q, uint64_t* d_hit, uint8_t* d_status, uint8_t* d_stage,
                   uint32_t* d_err) try {
    TRY(bind(c));
    Tables R;
    TRY(pack_tables(tables, T, 0, view_of, &R));
    if (q > kMaxN) return NKV_ERR_INVALID;
    if (q == 0) return NKV_OK;
    if (!d_keys || !d_koff || !d_klen || !d_hit || !d_status) return NKV_ERR_INVALID;
    unsigned int* err;
    TRY(verdict_word(c, d_err, &err));
    hipLaunchKernelGGL(k_lookup, dim3(blocks_for(q)), dim3(kBlock), 0, c->stream, R,
                       static_cast<const uint8_t*>(d_keys), d_koff, d_klen, q, d_hit, d_status, d_stage, err);
    HIPTRY(hipGetLastError());
    return finish_verdict(c, d_err, err);
} NKV_CATCH

int nkv_lookup_values_dev(nkv_ctx* c, const nkv_lookup_table* tables, int T, const uint64_t* d_hit,
                          const uint8_t* d_status, uint64_t q, void* d_out, uint64_t out_cap, uint64_t* d_out_off,
                          uint64_t* out_len) try {
    TRY(bind(c));
    if (!out_len) return NKV_ERR_INVALID;
    *out_len = 0;
    Tables R;
    TRY(pack_tables(tables, T, 0, view_of, &R));
    if (q > kMaxN) return NKV_ERR_INVALID;
    const bool query = !d_out;
    if (q == 0) {  // no Value: the one offset entry is 0
        if (!query && d_out_off) HIPTRY(hipMemsetAsync(d_out_off, 0, 8, c->stream));
        return NKV_OK;
    }
    if (!d_hit || !d_status || (!query && !d_out_off)) return NKV_ERR_INVALID;

    // scratch in d_stmp, which carries nothing from call to call: the lengths
    // (q), their exclusive sums (q + 1) and the Values' addresses (q)
    uint64_t *len, *off, *src;
    const auto carve = [&](Carver k) {
        len = k.take<uint64_t>(q);
        off = k.take<uint64_t>(q + 1);
        src = k.take<uint64_t>(q);
        return k.bytes();
    };
    TRY(grow(c->d_stmp, carve(Carver())));
    carve(Carver(c->d_stmp.p));
    size_t tb = 0;
    HIPTRY(scan_exclusive_u64(len, off, q, nullptr, &tb, c->stream));
    TRY(grow(c->d_tmp, tb));
    TRY(grow(c->d_stats, 16));  // [err | total]
    unsigned int* err = static_cast<unsigned int*>(c->d_stats.p);
    uint64_t* total = static_cast<uint64_t*>(c->d_stats.p) + 1;

    // with NKV_TIMING_EVENTS: "leaf" = measure, scan and the host's read of the
    // length, "reduce" = the offsets' copy and the copy kernel
    TRY(mark(c, 0));
    HIPTRY(hipMemsetAsync(err, 0, 16, c->stream));
    hipLaunchKernelGGL(k_value_measure, dim3(blocks_for(q)), dim3(kBlock), 0, c->stream, R, d_hit, d_status, q, len,
                       src, err);
    HIPTRY(hipGetLastError());
    HIPTRY(scan_exclusive_u64(len, off, q, c->d_tmp.p, &tb, c->stream));
    hipLaunchKernelGGL(k_scan_total<uint64_t>, dim3(1), dim3(1), 0, c->stream, len, off, q, total);
    HIPTRY(hipGetLastError());
    // the verdict and the length, before anything is written
    uint64_t h[2] = {0, 0};
    HIPTRY(hipMemcpyAsync(h, err, 16, hipMemcpyDeviceToHost, c->stream));
    HIPTRY(hipStreamSynchronize(c->stream));
    TRY(mark(c, 1));
    if (uint32_t(h[0])) {
        TRY(mark(c, 2));
        return NKV_ERR_INVALID;
    }
    *out_len = h[1];
    if (query) return mark(c, 2);
    // d_out's 16-byte grid over out_len bytes; no Value byte, no copy
    const uint64_t head = uint64_t(reinterpret_cast<uintptr_t>(d_out)) & 15;
    const uint64_t tiles = h[1] ? (head + h[1] + kCopyTile - 1) / kCopyTile : 0;
    if (out_cap < h[1] || tiles > 0x7fffffffull) {
        TRY(mark(c, 2));
        return NKV_ERR_INVALID;
    }
    HIPTRY(hipMemcpyAsync(d_out_off, off, 8 * (q + 1), hipMemcpyDeviceToDevice, c->stream));
    if (tiles) {
        hipLaunchKernelGGL(k_value_copy, dim3(unsigned(tiles)), dim3(kBlock), 0, c->stream,
                           static_cast<uint8_t*>(d_out), off, src, q, h[1]);
        HIPTRY(hipGetLastError());
    }
    return mark(c, 2);
} NKV_CATCH

}  // extern "C"
