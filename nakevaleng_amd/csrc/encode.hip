// encode.hip -- the first step of the write path on the device: record.New
// (core/record/record.go:49-60) and Record.ToBytes (record.go:175-187) over a
// batch of puts, the bytes wal.flushPartialBufferToSegment appends
// (core/wal/wal.go:199-232): nkv_encode_records_dev / nkv_encode_records.
// n (key, value) pairs in, the write log out: record i is
//   Crc u32 | Timestamp i64 | Status u8 | TypeInfo u8 | KeySize u64 | ValueSize u64 | Key | Value
// little endian, the records one behind the other in input order, and
// Crc = CRC-32/IEEE of Key ++ Value.
//
// Stages, all on the context's stream:
//   k_encode_measure one lane per put: both spans checked against their blobs
//                    (written so that a wrapped off + len is caught); the
//                    record's size, its payload length and the addresses of
//                    its key and its value.  Nothing follows an offset before
//                    the host has read this kernel's verdict.
//   scan             exclusive sums of the sizes = the record offsets, and
//                    k_scan_total puts the total behind them (n + 1 entries)
//                    and next to the error word; the host reads both once.
//   k_encode_write   tiles the OUTPUT bytes as the other writer kernels do:
//                    a workgroup owns 16 KiB of d_out on the 16-byte grid of
//                    its address and every lane stores one aligned uint4 per
//                    step.  A record is three pieces: its 30 header bytes, made
//                    in registers (Crc 0 for now), its key and its value.  A
//                    chunk inside one key or one value is ld16_any's one or
//                    two aligned loads, and a lane issues those of its four
//                    chunks before it shifts and stores the first; any other
//                    whole chunk is OR-ed together in registers from its
//                    pieces (ld_piece for key and value bytes), pieces of
//                    length 0 skipped; only the partial chunks at the two ends
//                    of the output go byte by byte.  A record is at least 30
//                    bytes, so a tile overlaps at most kCopyTile / 30 + 2
//                    records and its list always fits LDS.
//   checksums        on the written output, where Key ++ Value of record i is
//                    the one span at d_out + 30 + off[i]: the span kernel of
//                    nkv_crc32_dev (crc.hip) over it.
//   k_encode_patch   one lane per record: the 4 Crc bytes of its header (at
//                    any alignment: byte stores) and d_crc[i] when asked for.
// Every address and offset is a 64-bit quantity; there is no 32-bit shortcut.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bytes_dev.hpp"  // ld16_any, ld_piece, funnel16, first_at_least, last_at_most, k_scan_total
#include "context.hpp"

using namespace nkv;

namespace {

constexpr uint32_t kCopyTile = 16384;  // output bytes per workgroup
constexpr uint32_t kCopyChunk = 16;    // output bytes per lane and step
// records that can overlap one tile: at most kCopyTile / kHdr + 2 = 548 (the
// four lists take 17.3 KiB of LDS, which leaves room for 8 workgroups per CU)
constexpr uint32_t kCopyList = 552;

struct Puts {  // kernel argument: nkv_puts with the blobs as bytes
    const uint8_t* keys;
    uint64_t keys_len;
    const uint64_t* koff;
    const uint64_t* klen;
    const uint8_t* vals;
    uint64_t vals_len;
    const uint64_t* voff;
    const uint64_t* vlen;
    const int64_t* ts;  // nullptr: ts_all
    int64_t ts_all;
    const uint8_t* status;  // nullptr: 0
    const uint8_t* type;    // nullptr: 0
};

// scratch arrays over the puts, by index
struct Spans {
    uint64_t* size;  // 30 + KeySize + ValueSize
    uint64_t* plen;  // KeySize + ValueSize: the span the checksum covers
    uint64_t* ksrc;  // address of the key
    uint64_t* vsrc;  // address of the value
};

__device__ __forceinline__ bool span_in(uint64_t off, uint64_t len, uint64_t blob) {
    return off <= blob && len <= blob - off;
}

__global__ __launch_bounds__(kBlock) void k_encode_measure(Puts P, uint32_t n, Spans S, unsigned int* err) {
    const uint64_t g = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (g >= n) return;
    const uint64_t ko = P.koff[g], kl = P.klen[g], vo = P.voff[g], vl = P.vlen[g];
    const bool ok = span_in(ko, kl, P.keys_len) && span_in(vo, vl, P.vals_len);
    // a refused put counts as an empty one: the sums stay below n (30 + keys_len + vals_len)
    S.size[g] = kHdr + (ok ? kl + vl : 0);
    S.plen[g] = ok ? kl + vl : 0;
    S.ksrc[g] = uint64_t(reinterpret_cast<uintptr_t>(P.keys)) + (ok ? ko : 0);
    S.vsrc[g] = uint64_t(reinterpret_cast<uintptr_t>(P.vals)) + (ok ? vo : 0);
    if (!ok) atomicOr(err, 1u);
}

// The header fields of one record.
struct Head {
    uint64_t ts, kl, vl;
    uint32_t st, ty;
};

// Byte r (0 <= r < 30) of the header, Crc bytes 0.
__device__ __forceinline__ uint32_t head_byte(const Head& h, uint32_t r) {
    if (r < kAtTimestamp) return 0;
    if (r < kAtStatus) return uint32_t(h.ts >> (8 * (r - kAtTimestamp))) & 0xFFu;
    if (r == kAtStatus) return h.st;
    if (r == kAtTypeInfo) return h.ty;
    if (r < kAtValueSize) return uint32_t(h.kl >> (8 * (r - kAtKeySize))) & 0xFFu;
    return uint32_t(h.vl >> (8 * (r - kAtValueSize))) & 0xFFu;
}

// Bytes 0 .. cnt - 1 of v kept, the rest zero, placed d bytes up (1 <= cnt <=
// 16, d + cnt <= 16): what ld_piece does with the bytes it has read.
__device__ __forceinline__ uint4 keep_place(uint4 v, uint32_t cnt, uint32_t d) {
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

// Header bytes r .. r + cnt - 1 (r + cnt <= 30) in bytes d .. d + cnt - 1 of
// the result, the rest zero: the 30 bytes as eight words, funnel-shifted.
__device__ __forceinline__ uint4 head_piece(const Head& h, uint32_t r, uint32_t cnt, uint32_t d) {
    const uint4 lo = make_uint4(0u, uint32_t(h.ts), uint32_t(h.ts >> 32), h.st | (h.ty << 8) | (uint32_t(h.kl) << 16));
    const uint4 hi = make_uint4(uint32_t(h.kl >> 16), uint32_t(h.kl >> 48) | (uint32_t(h.vl) << 16),
                                uint32_t(h.vl >> 16), uint32_t(h.vl >> 48));
    const uint4 z = make_uint4(0, 0, 0, 0);
    uint4 v;
    if (r < 16) v = r ? funnel16(lo, hi, r) : lo;
    else v = r > 16 ? funnel16(hi, z, r - 16) : hi;
    return keep_place(v, cnt, d);
}

// Output byte o belongs to the record j with off[j] <= o < off[j + 1] (off
// holds n + 1 entries and increases strictly: a record is at least 30 bytes);
// at r = o - off[j] it is header byte r, key byte r - 30 or value byte r - 30 -
// KeySize.  Chunks lie on the 16-byte grid of d_out's address, so every full
// chunk is one aligned 16-byte store.
__global__ __launch_bounds__(kBlock) void k_encode_write(uint8_t* __restrict__ out, const uint64_t* __restrict__ off,
                                                         const uint64_t* __restrict__ ksrc,
                                                         const uint64_t* __restrict__ vsrc, Puts P, uint64_t n,
                                                         uint64_t out_len) {
    __shared__ uint64_t l_off[kCopyList + 1];
    __shared__ uint64_t l_ks[kCopyList];
    __shared__ uint64_t l_vs[kCopyList];
    __shared__ uint64_t l_kl[kCopyList];
    const uint64_t head = uint64_t(reinterpret_cast<uintptr_t>(out)) & 15;  // grid position p = o + head
    const uint64_t p0 = uint64_t(blockIdx.x) * kCopyTile, pend = head + out_len;
    if (p0 >= pend) return;
    const uint64_t o_lo = p0 > head ? p0 - head : 0;
    const uint64_t o_hi = p0 + kCopyTile < pend ? p0 + kCopyTile - head : out_len;  // > o_lo
    // records holding bytes of [o_lo, o_hi): from jlo, which holds o_lo, to jhi, which holds o_hi - 1
    // (found by the whole workgroup: off[0] = 0 <= o_lo, and jhi is the last with off < o_hi)
    const uint64_t jlo = first_at_least(off, 0, n, o_lo + 1) - 1;
    const uint64_t jend = jlo + kCopyList < n ? jlo + kCopyList : n;  // jhi lies below it: at most 548 records
    const uint64_t jhi = first_at_least(off, jlo + 1, jend, o_hi) - 1;
    const uint32_t cnt = uint32_t(jhi - jlo + 1 < kCopyList ? jhi - jlo + 1 : kCopyList);  // at most 548
    for (uint32_t e = threadIdx.x; e < cnt; e += kBlock) {
        l_off[e] = off[jlo + e];
        l_ks[e] = ksrc[jlo + e];
        l_vs[e] = vsrc[jlo + e];
        l_kl[e] = P.klen[jlo + e];
    }
    if (threadIdx.x == 0) l_off[cnt] = off[jlo + cnt];
    __syncthreads();
    const auto head_of = [&](uint32_t e, uint64_t a, uint64_t b, uint64_t kl) {
        const uint64_t j = jlo + e;
        Head h;
        h.ts = uint64_t(P.ts ? P.ts[j] : P.ts_all);
        h.st = P.status ? P.status[j] : 0u;
        h.ty = P.type ? P.type[j] : 0u;
        h.kl = kl;
        h.vl = b - a - kHdr - kl;
        return h;
    };
    // A lane's kSteps chunks lie 4 KiB apart.  First the chunks that lie inside
    // one key or one value: ld16_any's one or two aligned loads of all of them
    // are issued before the first is shifted and stored, so a lane keeps up to
    // 128 source bytes in flight.  Then, one by one, the chunks that hold a
    // piece boundary or an end of the output.
    constexpr uint32_t kSteps = kCopyTile / (kCopyChunk * kBlock);
    uint4 lo[kSteps], hi2[kSteps];
    uint32_t sh[kSteps];
    uint32_t plain = 0, mixed = 0;  // bit it: chunk it is of that kind
#pragma unroll
    for (uint32_t it = 0; it < kSteps; ++it) {
        const uint64_t p = p0 + uint64_t(it * kBlock + threadIdx.x) * kCopyChunk;
        lo[it] = hi2[it] = make_uint4(0, 0, 0, 0);
        sh[it] = 0;
        if (p + kCopyChunk <= head || p >= pend) continue;
        const uint64_t ob = p > head ? p - head : 0;  // first output byte of the chunk
        const bool whole = p >= head && p + kCopyChunk <= pend;
        const uint32_t e = last_at_most(l_off, 0u, cnt, ob);  // the record that holds ob
        const uint64_t a = l_off[e], b = l_off[e + 1], kl = l_kl[e];
        const uint64_t r0 = ob - a;
        const bool in_key = r0 >= kHdr && r0 + kCopyChunk <= kHdr + kl;
        const bool in_val = r0 >= kHdr + kl && ob + kCopyChunk <= b;
        if (whole && (in_key || in_val)) {
            const uint64_t S = in_key ? l_ks[e] + (r0 - kHdr) : l_vs[e] + (r0 - kHdr - kl);
            sh[it] = uint32_t(S & 15);
            // the address as an offset from its blob's pointer: a global load, which the LDS
            // reads of the next chunk's search do not wait for (a flat one counts as both)
            const uint8_t* blob = in_key ? P.keys : P.vals;
            const uint4* q = reinterpret_cast<const uint4*>(
                blob + ((S - sh[it]) - uint64_t(reinterpret_cast<uintptr_t>(blob))));
            lo[it] = q[0];
            if (sh[it]) hi2[it] = q[1];  // an aligned word with one of the bytes in it cannot cross a page
            plain |= 1u << it;
        } else {
            mixed |= 1u << it;
        }
    }
#pragma unroll
    for (uint32_t it = 0; it < kSteps; ++it) lo[it] = funnel16(lo[it], hi2[it], sh[it]);  // sh = 0: lo as it is
#pragma unroll
    for (uint32_t it = 0; it < kSteps; ++it) {  // behind the last load: no store waits for another
        if (!((plain >> it) & 1u)) continue;
        const uint64_t ob = p0 + uint64_t(it * kBlock + threadIdx.x) * kCopyChunk - head;  // whole: p >= head
        *reinterpret_cast<uint4*>(out + ob) = lo[it];
    }
#pragma unroll 1
    for (uint32_t it = 0; it < kSteps; ++it) {
        if (!((mixed >> it) & 1u)) continue;
        const uint64_t p = p0 + uint64_t(it * kBlock + threadIdx.x) * kCopyChunk;
        const uint64_t ob = p > head ? p - head : 0;
        const bool whole = p >= head && p + kCopyChunk <= pend;
        uint32_t e = last_at_most(l_off, 0u, cnt, ob);
        uint64_t a = l_off[e], b = l_off[e + 1], kl = l_kl[e];
        if (whole) {  // the pieces that overlap the chunk, in registers
            uint4 acc = make_uint4(0, 0, 0, 0);
            const uint64_t oe = ob + kCopyChunk;  // <= o_hi: the records up to jhi hold it all
            uint64_t o = ob;
            for (;;) {
                const uint64_t r = o - a, ke = a + kHdr + kl;  // ke: where the key ends
                uint4 v = make_uint4(0, 0, 0, 0);
                uint64_t hi;
                if (r < kHdr) {
                    hi = a + kHdr < oe ? a + kHdr : oe;
                    v = head_piece(head_of(e, a, b, kl), uint32_t(r), uint32_t(hi - o), uint32_t(o - ob));
                } else if (o < ke) {
                    hi = ke < oe ? ke : oe;
                    v = ld_piece(l_ks[e] + (r - kHdr), uint32_t(hi - o), uint32_t(o - ob));
                } else {
                    hi = b < oe ? b : oe;
                    if (hi > o) v = ld_piece(l_vs[e] + (r - kHdr - kl), uint32_t(hi - o), uint32_t(o - ob));
                }
                acc.x |= v.x;
                acc.y |= v.y;
                acc.z |= v.z;
                acc.w |= v.w;
                o = hi;
                if (o >= oe) break;
                if (o >= b) {  // the next record's header follows
                    ++e;
                    a = b;
                    b = l_off[e + 1];
                    kl = l_kl[e];
                }
            }
            *reinterpret_cast<uint4*>(out + ob) = acc;
        } else {  // the two ends of the output: byte by byte
            for (uint32_t k = 0; k < kCopyChunk; ++k) {
                const uint64_t pb = p + k;
                if (pb < head || pb >= pend) continue;
                const uint64_t o = pb - head;
                while (o >= b) {  // o < out_len = off[n]: ends at the record that holds o
                    ++e;
                    a = b;
                    b = l_off[e + 1];
                    kl = l_kl[e];
                }
                const uint64_t r = o - a;
                uint32_t byte;
                if (r < kHdr) byte = head_byte(head_of(e, a, b, kl), uint32_t(r));
                else if (r < kHdr + kl) byte = *reinterpret_cast<const uint8_t*>(uintptr_t(l_ks[e] + (r - kHdr)));
                else byte = *reinterpret_cast<const uint8_t*>(uintptr_t(l_vs[e] + (r - kHdr - kl)));
                out[o] = uint8_t(byte);
            }
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_encode_patch(uint8_t* __restrict__ out, const uint64_t* __restrict__ off,
                                                         const uint32_t* __restrict__ crc, uint32_t n,
                                                         uint32_t* __restrict__ crc_out) {
    const uint64_t g = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (g >= n) return;
    const uint32_t v = crc[g];
    uint8_t* h = out + off[g];
    h[0] = uint8_t(v);
    h[1] = uint8_t(v >> 8);
    h[2] = uint8_t(v >> 16);
    h[3] = uint8_t(v >> 24);
    if (crc_out) crc_out[g] = v;
}

// What both forms refuse before anything is launched or copied.
int check_puts(const nkv_puts* u, const uint64_t* out_len) {
    if (!u || !out_len || u->n > kMaxN) return NKV_ERR_INVALID;
    if (u->n && (!u->koff || !u->klen || !u->voff || !u->vlen)) return NKV_ERR_INVALID;
    if ((!u->keys && u->keys_len) || (!u->vals && u->vals_len)) return NKV_ERR_INVALID;
    // n (30 + keys_len + vals_len) < 2^64 bounds the sum of the sizes: no scan can wrap
    const uint64_t blob = u->keys_len + u->vals_len;
    if (blob < u->keys_len || blob + kHdr < blob) return NKV_ERR_INVALID;
    if (u->n && blob + kHdr > ~uint64_t(0) / u->n) return NKV_ERR_INVALID;
    return NKV_OK;
}

inline uint64_t up16(uint64_t x) { return (x + 15) & ~uint64_t(15); }

}  // namespace

extern "C" {

int nkv_encode_records_dev(nkv_ctx* c, const nkv_puts* puts, void* d_out, uint64_t out_cap, uint64_t* d_out_off,
                           uint32_t* d_crc, uint64_t* out_len) try {
    TRY(bind(c));
    TRY(check_puts(puts, out_len));
    const uint64_t n = puts->n;
    const bool query = !d_out;
    if (n && !query && !d_out_off) return NKV_ERR_INVALID;
    *out_len = 0;
    if (n == 0) return NKV_OK;
    const Puts P{static_cast<const uint8_t*>(puts->keys), puts->keys_len, puts->koff, puts->klen,
                 static_cast<const uint8_t*>(puts->vals), puts->vals_len, puts->voff, puts->vlen,
                 puts->ts, puts->ts_all, puts->status, puts->type};

    // scratch in d_stmp, which carries nothing from call to call: sizes (n),
    // payload lengths (n), offsets (n + 1), key and value addresses (n each),
    // checksums (n u32)
    Spans S;
    uint64_t* off;
    uint32_t* crc;
    const auto carve = [&](Carver k) {
        S.size = k.take<uint64_t>(n);
        S.plen = k.take<uint64_t>(n);
        off = k.take<uint64_t>(n + 1);
        S.ksrc = k.take<uint64_t>(n);
        S.vsrc = k.take<uint64_t>(n);
        crc = k.take<uint32_t>(n);
        return k.bytes();
    };
    TRY(grow(c->d_stmp, carve(Carver())));
    carve(Carver(c->d_stmp.p));
    size_t tb = 0;
    HIPTRY(scan_exclusive_u64(S.size, off, n, nullptr, &tb, c->stream));
    TRY(grow(c->d_tmp, tb));
    TRY(grow(c->d_stats, 16));  // [err | total]
    unsigned int* err = static_cast<unsigned int*>(c->d_stats.p);
    uint64_t* total = static_cast<uint64_t*>(c->d_stats.p) + 1;

    // with NKV_TIMING_EVENTS: "leaf" = everything before the writer (measure,
    // scan, the host's read of the verdict and the length, the offsets' copy),
    // "reduce" = the writer, the checksums and the patch
    TRY(mark(c, 0));
    HIPTRY(hipMemsetAsync(err, 0, 16, c->stream));
    hipLaunchKernelGGL(k_encode_measure, dim3(blocks_for(n)), dim3(kBlock), 0, c->stream, P, uint32_t(n), S, err);
    HIPTRY(hipGetLastError());
    HIPTRY(scan_exclusive_u64(S.size, off, n, c->d_tmp.p, &tb, c->stream));
    hipLaunchKernelGGL(k_scan_total<uint64_t>, dim3(1), dim3(1), 0, c->stream, S.size, off, n, total);
    HIPTRY(hipGetLastError());
    // the verdict and the length, before anything is written
    uint64_t h[2] = {0, 0};
    HIPTRY(hipMemcpyAsync(h, err, 16, hipMemcpyDeviceToHost, c->stream));
    HIPTRY(hipStreamSynchronize(c->stream));
    // d_out's 16-byte grid over out_len bytes
    const uint64_t head = uint64_t(reinterpret_cast<uintptr_t>(d_out)) & 15;
    const uint64_t tiles = (head + h[1] + kCopyTile - 1) / kCopyTile;
    const bool bad = uint32_t(h[0]) != 0;
    if (!bad) *out_len = h[1];
    if (bad || query || out_cap < h[1] || tiles > 0x7fffffffull) {  // nothing is written
        TRY(mark(c, 1));
        TRY(mark(c, 2));
        return bad || !query ? NKV_ERR_INVALID : NKV_OK;
    }
    uint8_t* out = static_cast<uint8_t*>(d_out);
    HIPTRY(hipMemcpyAsync(d_out_off, off, 8 * n, hipMemcpyDeviceToDevice, c->stream));
    TRY(mark(c, 1));
    hipLaunchKernelGGL(k_encode_write, dim3(unsigned(tiles)), dim3(kBlock), 0, c->stream, out, off, S.ksrc, S.vsrc, P,
                       n, h[1]);
    HIPTRY(hipGetLastError());
    // Key ++ Value of record i is the one span at out + 30 + off[i]
    HIPTRY(launch_crc_spans(out + kHdr, off, S.plen, n, crc, c->crc_load, c->stream));
    hipLaunchKernelGGL(k_encode_patch, dim3(blocks_for(n)), dim3(kBlock), 0, c->stream, out, off, crc, uint32_t(n),
                       d_crc);
    HIPTRY(hipGetLastError());
    return mark(c, 2);
} NKV_CATCH

int nkv_encode_records(nkv_ctx* c, const nkv_puts* puts, uint8_t* out, uint64_t out_cap, uint64_t* out_rec_size,
                       uint32_t* crc_out, uint64_t* out_len) try {
    TRY(bind(c));
    TRY(check_puts(puts, out_len));
    const uint64_t n = puts->n;
    const bool query = !out;
    if (n && !query && !out_rec_size) return NKV_ERR_INVALID;
    *out_len = 0;
    if (n == 0) return NKV_OK;
    // the sizes on the host, term by term (check_puts bounds their sum)
    uint64_t total = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t ko = puts->koff[i], kl = puts->klen[i], vo = puts->voff[i], vl = puts->vlen[i];
        if (ko > puts->keys_len || kl > puts->keys_len - ko || vo > puts->vals_len || vl > puts->vals_len - vo)
            return NKV_ERR_INVALID;
        total += kHdr + kl + vl;
    }
    *out_len = total;
    if (query) return NKV_OK;
    if (out_cap < total) return NKV_ERR_INVALID;

    // one device block: the five u64 arrays, Status and TypeInfo, then the two blobs at 16-byte places
    const uint64_t at_st = 5 * 8 * n, at_ty = at_st + n, at_keys = up16(at_ty + n),
                   at_vals = at_keys + up16(puts->keys_len), bytes = at_vals + up16(puts->vals_len);
    TRY(grow(c->d_data, bytes + 16));
    DevBuf& log = c->d_nodes;  // the encoded write log
    TRY(grow(log, total));
    TRY(grow(c->d_off, 8 * n));
    TRY(grow(c->d_len, 4 * n));
    uint8_t* d = static_cast<uint8_t*>(c->d_data.p);
    uint64_t* d64 = static_cast<uint64_t*>(c->d_data.p);
    const auto up = [&](uint64_t at, const void* src, uint64_t nb) {
        return nb ? hipMemcpyAsync(d + at, src, nb, hipMemcpyHostToDevice, c->stream) : hipSuccess;
    };
    HIPTRY(up(0, puts->koff, 8 * n));
    HIPTRY(up(8 * n, puts->klen, 8 * n));
    HIPTRY(up(16 * n, puts->voff, 8 * n));
    HIPTRY(up(24 * n, puts->vlen, 8 * n));
    if (puts->ts) HIPTRY(up(32 * n, puts->ts, 8 * n));
    if (puts->status) HIPTRY(up(at_st, puts->status, n));
    if (puts->type) HIPTRY(up(at_ty, puts->type, n));
    HIPTRY(up(at_keys, puts->keys, puts->keys_len));
    HIPTRY(up(at_vals, puts->vals, puts->vals_len));
    nkv_puts dp = *puts;
    dp.keys = d + at_keys;
    dp.vals = d + at_vals;
    dp.koff = d64;
    dp.klen = d64 + n;
    dp.voff = d64 + 2 * n;
    dp.vlen = d64 + 3 * n;
    dp.ts = puts->ts ? reinterpret_cast<const int64_t*>(d64 + 4 * n) : nullptr;
    dp.status = puts->status ? d + at_st : nullptr;
    dp.type = puts->type ? d + at_ty : nullptr;
    uint64_t* d_out_off = static_cast<uint64_t*>(c->d_off.p);
    uint32_t* d_crc = static_cast<uint32_t*>(c->d_len.p);
    uint64_t got = 0;
    TRY(nkv_encode_records_dev(c, &dp, log.p, total, d_out_off, d_crc, &got));
    if (crc_out) HIPTRY(hipMemcpyAsync(crc_out, d_crc, 4 * n, hipMemcpyDeviceToHost, c->stream));
    return download_table(c, log.p, total, d_out_off, n, out, out_rec_size);  // the call's synchronize
} NKV_CATCH

}  // extern "C"
