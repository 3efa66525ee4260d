// index.hip -- the SSTable writer's Index and Summary tables on the device
// (core/sstable/sstable.go:76-139 makeIndexAndSummary): nkv_index_summary_dev /
// nkv_index_summary_from_records / nkv_summary_entries.
//
// Index entry i   = KeySize u64 | Offset i64 (of record i in the Data table) | Key
// Summary         = MinKeySize u64 | MaxKeySize u64 | Payload u64 | MinKey | MaxKey,
//                   then one entry KeySize | Offset (of Index entry i in the
//                   Index) | Key for record 0, every record i with i % page == 0,
//                   and the last record (each once).
//
// Stages, all on the context's stream:
//   k_index_measure   one lane per record: the header lies in the stream and so
//                     does the key (record_dev.hpp key_span_in); writes 16 + KeySize as the Index entry's
//                     size and, for a selected record, as its Summary entry's.
//                     Selected entry e is record e * page, the last entry the
//                     last record: a closed form, so no compaction pass.
//   scans             exclusive sums of the two size arrays = entry offsets;
//                     k_index_totals leaves the lengths next to the error word.
//                     The host reads both before any writer is launched.
//   k_index_write     tiles the OUTPUT bytes, once per image: a workgroup owns
//                     16 KiB of the image, keeps the entries overlapping it in
//                     LDS, and every lane puts 16 destination-aligned bytes
//                     together in registers (the two fields from their values,
//                     key bytes funnel-shifted out of aligned 16-byte loads of
//                     the stream) and stores them at once.
//   k_summary_header  the Summary's five header fields, byte by byte.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bytes_dev.hpp"  // sel4, first_at_least
#include "context.hpp"

using namespace nkv;

namespace {

constexpr uint32_t kEnt = 16;           // KeySize + Offset in front of every entry's key
constexpr uint32_t kWriteTile = 16384;  // image bytes per workgroup
constexpr uint32_t kWriteChunk = 16;    // image bytes per lane and step
// entries that can overlap one tile: at most kWriteTile / kEnt + 2 = 1026
constexpr uint32_t kWriteList = 1032;

// Selected record of Summary entry e (m entries over n records): e * page, the
// last entry the last record.  The Index is the same with page = 1, m = n.
__device__ __forceinline__ uint64_t record_of(uint64_t e, uint64_t m, uint64_t n, uint64_t page) {
    return e + 1 == m ? n - 1 : e * page;
}

__global__ __launch_bounds__(kBlock) void k_index_measure(const uint8_t* __restrict__ s, uint64_t L,
                                                          const uint64_t* __restrict__ off, uint64_t n, uint64_t page,
                                                          uint64_t m, uint64_t* __restrict__ isz,
                                                          uint64_t* __restrict__ ssz, unsigned int* err) {
    const uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= n) return;
    uint64_t ks = 0;
    const bool bad = !key_span_in(s, L, off[i], &ks);  // ks stays 0
    isz[i] = kEnt + ks;
    if (i == n - 1) ssz[m - 1] = kEnt + ks;
    else if (i % page == 0) ssz[i / page] = kEnt + ks;
    if (bad) atomicOr(err, 1u);
}

// totals: [0] index_len, [1] Payload, [2] MinKeySize, [3] MaxKeySize
__global__ void k_index_totals(const uint64_t* __restrict__ isz, const uint64_t* __restrict__ ioff, uint64_t n,
                               const uint64_t* __restrict__ ssz, const uint64_t* __restrict__ soff, uint64_t m,
                               uint64_t* __restrict__ totals) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    totals[0] = ioff[n - 1] + isz[n - 1];
    totals[1] = soff[m - 1] + ssz[m - 1];
    totals[2] = isz[0] - kEnt;
    totals[3] = isz[n - 1] - kEnt;
}

struct Image {  // the entries of one image
    uint8_t* out;           // where entry 0 starts (any alignment)
    const uint64_t* eoff;   // m entry offsets (exclusive sums of the sizes)
    uint64_t m, len;        // entries, and the bytes of all of them
    const uint64_t* field;  // the Offset field of record i's entry
    uint64_t n, page;       // record_of
};

// Image byte o is byte o - eoff[e] of entry e, for the e with eoff[e] <= o <
// eoff[e + 1]: bytes 0..7 KeySize, 8..15 the Offset field, then the key, which
// lies at stream + rec_off[i] + 30.  Chunks lie on the 16-byte grid of the
// output's address, so every full chunk is one aligned 16-byte store; a chunk
// of key bytes of one entry is read as the one or two aligned 16-byte words of
// the stream that hold it (an aligned word with one key byte in it cannot
// cross a page) and funnel-shifted; a chunk that is exactly an entry's two
// fields is put together from their values; any other chunk byte by byte, and
// at the ends of the image only the bytes inside it are stored.
__global__ __launch_bounds__(kBlock) void k_index_write(Image g, const uint8_t* __restrict__ stream,
                                                        const uint64_t* __restrict__ rec_off) {
    __shared__ uint64_t l_off[kWriteList + 1];
    __shared__ uint64_t l_fld[kWriteList];
    __shared__ uint64_t l_key[kWriteList];
    uint8_t* __restrict__ out = g.out;
    const uint64_t head = uint64_t(reinterpret_cast<uintptr_t>(out)) & 15;  // grid position p = o + head
    const uint64_t p0 = uint64_t(blockIdx.x) * kWriteTile, pend = head + g.len;
    if (g.m == 0 || p0 >= pend) return;
    const uint64_t o_lo = p0 > head ? p0 - head : 0;
    const uint64_t o_hi = p0 + kWriteTile < pend ? p0 + kWriteTile - head : g.len;
    // entries overlapping [o_lo, o_hi): jlo = the last with eoff <= o_lo, up to
    // the first with eoff >= o_hi, which is at most kWriteTile / kEnt + 1
    // entries on (entries are at least kEnt bytes apart)
    uint64_t lo = first_at_least(g.eoff, 0, g.m, o_lo + 1);
    const uint64_t jlo = lo - 1;  // eoff[0] = 0 <= o_lo
    const uint64_t far = jlo + kWriteTile / kEnt + 2;
    lo = first_at_least(g.eoff, lo, far < g.m ? far : g.m, o_hi);
    const uint32_t cnt = uint32_t(lo - jlo < kWriteList ? lo - jlo : kWriteList);
    for (uint32_t e = threadIdx.x; e < cnt; e += kBlock) {
        const uint64_t i = record_of(jlo + e, g.m, g.n, g.page);
        l_off[e] = g.eoff[jlo + e];
        l_fld[e] = g.field[i];
        l_key[e] = uint64_t(reinterpret_cast<uintptr_t>(stream + rec_off[i] + kHdr));
    }
    if (threadIdx.x == 0) l_off[cnt] = jlo + cnt < g.m ? g.eoff[jlo + cnt] : g.len;
    __syncthreads();
#pragma unroll 1
    for (uint32_t it = 0; it < kWriteTile / (kWriteChunk * kBlock); ++it) {
        const uint64_t p = p0 + uint64_t(it * kBlock + threadIdx.x) * kWriteChunk;
        if (p + kWriteChunk <= head || p >= pend) continue;
        const uint64_t ob = p > head ? p - head : 0;  // first image byte of the chunk
        uint32_t a = 0, b = cnt;                      // e = the last list entry with eoff <= ob
        while (b - a > 1) {
            const uint32_t mid = (a + b) / 2;
            if (l_off[mid] <= ob) a = mid;
            else b = mid;
        }
        uint32_t e = a;
        const bool whole = p >= head && p + kWriteChunk <= pend;
        const bool inside = whole && ob + kWriteChunk <= l_off[e + 1];
        const uint64_t r = ob - l_off[e];  // the chunk's place in its entry
        if (inside && r >= kEnt) {
            const uint64_t S = l_key[e] + (r - kEnt);
            const uint32_t sh = uint32_t(S & 15);
            const uint4* q = reinterpret_cast<const uint4*>(uintptr_t(S - sh));
            uint4 v = q[0];
            if (sh) {
                const uint4 w = q[1];
                const uint32_t d = sh >> 2, bs = sh & 3;
                const uint32_t x0 = sel4(d, v.x, v.y, v.z, v.w), x1 = sel4(d, v.y, v.z, v.w, w.x),
                               x2 = sel4(d, v.z, v.w, w.x, w.y), x3 = sel4(d, v.w, w.x, w.y, w.z),
                               x4 = sel4(d, w.x, w.y, w.z, w.w);
                v.x = __builtin_amdgcn_alignbyte(x1, x0, bs);
                v.y = __builtin_amdgcn_alignbyte(x2, x1, bs);
                v.z = __builtin_amdgcn_alignbyte(x3, x2, bs);
                v.w = __builtin_amdgcn_alignbyte(x4, x3, bs);
            }
            *reinterpret_cast<uint4*>(out + ob) = v;
        } else if (inside && r == 0) {
            const uint64_t ks = l_off[e + 1] - l_off[e] - kEnt, f = l_fld[e];
            *reinterpret_cast<uint4*>(out + ob) = make_uint4(uint32_t(ks), uint32_t(ks >> 32), uint32_t(f), uint32_t(f >> 32));
        } else {
            uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
            for (uint32_t k = 0; k < kWriteChunk; ++k) {
                const uint64_t pb = p + k;
                if (pb < head || pb >= pend) continue;
                const uint64_t o = pb - head;
                while (e + 1 < cnt && o >= l_off[e + 1]) ++e;
                const uint64_t rb = o - l_off[e];
                uint8_t byte;
                if (rb < 8) byte = uint8_t((l_off[e + 1] - l_off[e] - kEnt) >> (8 * rb));
                else if (rb < kEnt) byte = uint8_t(l_fld[e] >> (8 * (rb - 8)));
                else byte = *reinterpret_cast<const uint8_t*>(uintptr_t(l_key[e] + (rb - kEnt)));
                if (whole) w[k >> 2] |= uint32_t(byte) << (8 * (k & 3));
                else out[o] = byte;
            }
            if (whole) *reinterpret_cast<uint4*>(out + ob) = make_uint4(w[0], w[1], w[2], w[3]);
        }
    }
}

// MinKeySize | MaxKeySize | Payload | MinKey | MaxKey: 24 bytes and two keys,
// in front of an entry region that starts wherever they end.
__global__ __launch_bounds__(kBlock) void k_summary_header(uint8_t* __restrict__ out,
                                                           const uint8_t* __restrict__ stream,
                                                           const uint64_t* __restrict__ rec_off, uint64_t n,
                                                           const uint64_t* __restrict__ totals) {
    const uint64_t payload = totals[1], ks0 = totals[2], ks1 = totals[3];
    const uint8_t* k0 = stream + rec_off[0] + kHdr;
    const uint8_t* k1 = stream + rec_off[n - 1] + kHdr;
    const uint64_t H = 24 + ks0 + ks1;
    for (uint64_t b = uint64_t(blockIdx.x) * kBlock + threadIdx.x; b < H; b += uint64_t(gridDim.x) * kBlock) {
        uint8_t v;
        if (b < 8) v = uint8_t(ks0 >> (8 * b));
        else if (b < 16) v = uint8_t(ks1 >> (8 * (b - 8)));
        else if (b < 24) v = uint8_t(payload >> (8 * (b - 16)));
        else if (b < 24 + ks0) v = k0[b - 24];
        else v = k1[b - 24 - ks0];
        out[b] = v;
    }
}

uint64_t summary_entries(uint64_t n, uint64_t page) {
    if (n <= 1) return n;
    if (page == 0) return 0;
    return 1 + (n - 1) / page + ((n - 1) % page ? 1 : 0);
}

inline uint64_t tiles_of(const void* out, uint64_t len) {
    return ((uint64_t(reinterpret_cast<uintptr_t>(out)) & 15) + len + kWriteTile - 1) / kWriteTile;
}

// own: the images go to the context's d_nodes (Index) and d_img (Summary),
// grown once the lengths are known, instead of d_index / d_summary.
int index_summary(nkv_ctx* c, const uint8_t* d_stream, uint64_t stream_len, const uint64_t* d_rec_off, uint64_t n,
                  uint64_t page, uint8_t* d_index, uint64_t index_cap, uint8_t* d_summary, uint64_t summary_cap,
                  bool own, bool query, uint64_t* index_len, uint64_t* summary_len) {
    *index_len = 0;
    *summary_len = 0;
    if (n > kMaxN || (page == 0 && n >= 2)) return NKV_ERR_INVALID;
    if (n == 0) {  // what the reference's loop leaves of an empty slice: no entry, a header of zeros
        *summary_len = 24;
        if (query) return NKV_OK;
        if (summary_cap < 24) return NKV_ERR_INVALID;
        if (own) {
            TRY(grow(c->d_img, 24));
            d_summary = static_cast<uint8_t*>(c->d_img.p);
        }
        if (!d_summary) return NKV_ERR_INVALID;
        return st(hipMemsetAsync(d_summary, 0, 24, c->stream));
    }
    if (!d_stream || !d_rec_off) return NKV_ERR_INVALID;
    // every entry is at most 16 + stream_len bytes: the lengths fit 64 bits
    if (stream_len > UINT64_MAX / n - kEnt) return NKV_ERR_INVALID;
    if (page == 0) page = 1;  // n = 1: never divided by in the reference (sstable.go:111)
    const uint64_t m = summary_entries(n, page);

    // scratch in d_stmp, which carries nothing from call to call: the Index
    // entries' sizes and offsets (n each), the Summary entries' (m each)
    uint64_t *isz, *ioff, *ssz, *soff;
    const auto carve = [&](Carver k) {
        isz = k.take<uint64_t>(n);
        ioff = k.take<uint64_t>(n);
        ssz = k.take<uint64_t>(m);
        soff = k.take<uint64_t>(m);
        return k.bytes();
    };
    TRY(grow(c->d_stmp, carve(Carver())));
    carve(Carver(c->d_stmp.p));
    size_t tb = 0;
    HIPTRY(scan_exclusive_u64(isz, ioff, n, nullptr, &tb, c->stream));
    TRY(grow(c->d_tmp, tb));
    TRY(grow(c->d_stats, 40));  // [err | index_len, Payload, MinKeySize, MaxKeySize]
    unsigned int* err = static_cast<unsigned int*>(c->d_stats.p);
    uint64_t* totals = static_cast<uint64_t*>(c->d_stats.p) + 1;

    // with NKV_TIMING_EVENTS: "leaf" = measure + scans, "reduce" = the writers
    TRY(mark(c, 0));
    HIPTRY(hipMemsetAsync(err, 0, 40, c->stream));
    hipLaunchKernelGGL(k_index_measure, dim3(blocks_for(n)), dim3(kBlock), 0, c->stream, d_stream, stream_len,
                       d_rec_off, n, page, m, isz, ssz, err);
    HIPTRY(hipGetLastError());
    HIPTRY(scan_exclusive_u64(isz, ioff, n, c->d_tmp.p, &tb, c->stream));
    HIPTRY(scan_exclusive_u64(ssz, soff, m, c->d_tmp.p, &tb, c->stream));
    hipLaunchKernelGGL(k_index_totals, dim3(1), dim3(1), 0, c->stream, isz, ioff, n, ssz, soff, m, totals);
    HIPTRY(hipGetLastError());
    TRY(mark(c, 1));
    // the verdict and the lengths, before any writer is launched
    uint64_t h[5] = {0, 0, 0, 0, 0};
    HIPTRY(hipMemcpyAsync(h, err, 40, hipMemcpyDeviceToHost, c->stream));
    HIPTRY(hipStreamSynchronize(c->stream));
    if (uint32_t(h[0])) {
        TRY(mark(c, 2));
        return NKV_ERR_INVALID;
    }
    const uint64_t ilen = h[1], hdr = 24 + h[3] + h[4], slen = hdr + h[2];
    *index_len = ilen;
    *summary_len = slen;
    if (query) return mark(c, 2);
    if (own) {  // the host form: the Index image in d_nodes, the Summary in d_img
        if (index_cap >= ilen && summary_cap >= slen) {
            TRY(grow(c->d_nodes, ilen));
            TRY(grow(c->d_img, slen));
            d_index = static_cast<uint8_t*>(c->d_nodes.p);
            d_summary = static_cast<uint8_t*>(c->d_img.p);
        }
    }
    // nothing is written unless both images fit
    bool fits = index_cap >= ilen && summary_cap >= slen && d_index && d_summary;
    uint64_t itiles = 0, stiles = 0;
    if (fits) {
        itiles = tiles_of(d_index, ilen);
        stiles = tiles_of(d_summary + hdr, h[2]);
        fits = itiles <= 0x7fffffffull && stiles <= 0x7fffffffull;
    }
    if (!fits) {
        TRY(mark(c, 2));
        return NKV_ERR_INVALID;
    }
    const Image index{d_index, ioff, n, ilen, d_rec_off, n, 1};
    hipLaunchKernelGGL(k_index_write, dim3(unsigned(itiles)), dim3(kBlock), 0, c->stream, index, d_stream, d_rec_off);
    HIPTRY(hipGetLastError());
    const unsigned hb = unsigned(std::min<uint64_t>(blocks_for(hdr), 1024));
    hipLaunchKernelGGL(k_summary_header, dim3(hb), dim3(kBlock), 0, c->stream, d_summary, d_stream, d_rec_off, n,
                       totals);
    HIPTRY(hipGetLastError());
    const Image summary{d_summary + hdr, soff, m, h[2], ioff, n, page};
    hipLaunchKernelGGL(k_index_write, dim3(unsigned(stiles)), dim3(kBlock), 0, c->stream, summary, d_stream,
                       d_rec_off);
    HIPTRY(hipGetLastError());
    return mark(c, 2);
}

}  // namespace

extern "C" {

uint64_t nkv_summary_entries(uint64_t n, uint64_t page_size) { return summary_entries(n, page_size); }

int nkv_index_summary_dev(nkv_ctx* c, const void* d_stream, uint64_t stream_len, const uint64_t* d_rec_off,
                          uint64_t n, uint64_t page_size, void* d_index, uint64_t index_cap, void* d_summary,
                          uint64_t summary_cap, uint64_t* index_len, uint64_t* summary_len) try {
    TRY(bind(c));
    if (!index_len || !summary_len) return NKV_ERR_INVALID;
    return index_summary(c, static_cast<const uint8_t*>(d_stream), stream_len, d_rec_off, n, page_size,
                         static_cast<uint8_t*>(d_index), index_cap, static_cast<uint8_t*>(d_summary), summary_cap,
                         false, !d_index && !d_summary, index_len, summary_len);
} NKV_CATCH

int nkv_index_summary_from_records(nkv_ctx* c, const uint8_t* stream, uint64_t stream_len, const uint64_t* rec_size,
                                   uint64_t n, uint64_t page_size, uint8_t* index_out, uint64_t index_cap,
                                   uint8_t* summary_out, uint64_t summary_cap, uint64_t* index_len,
                                   uint64_t* summary_len) try {
    TRY(bind(c));
    if (!index_len || !summary_len) return NKV_ERR_INVALID;
    *index_len = 0;
    *summary_len = 0;
    if (n > kMaxN || (n && (!stream || !rec_size))) return NKV_ERR_INVALID;
    if (!records_fill(rec_size, n, stream_len)) return NKV_ERR_INVALID;
    const bool query = !index_out && !summary_out;
    const uint8_t* d_stream = nullptr;
    const uint64_t* d_off = nullptr;
    if (n) {
        TRY(grow(c->d_data, stream_len));
        TRY(grow(c->d_len, 8 * n));
        TRY(grow(c->d_off, 8 * n));
        TRY(upload_records(c, stream, stream_len, rec_size, n, c->d_data.p, static_cast<uint64_t*>(c->d_len.p),
                           static_cast<uint64_t*>(c->d_off.p)));
        d_stream = static_cast<const uint8_t*>(c->d_data.p);
        d_off = static_cast<const uint64_t*>(c->d_off.p);
    }
    TRY(index_summary(c, d_stream, stream_len, d_off, n, page_size, nullptr, index_cap, nullptr, summary_cap, true,
                      query, index_len, summary_len));
    if (query) return NKV_OK;
    if (*index_len && !index_out) return NKV_ERR_INVALID;
    if (!summary_out) return NKV_ERR_INVALID;
    if (*index_len) HIPTRY(hipMemcpyAsync(index_out, c->d_nodes.p, *index_len, hipMemcpyDeviceToHost, c->stream));
    HIPTRY(hipMemcpyAsync(summary_out, c->d_img.p, *summary_len, hipMemcpyDeviceToHost, c->stream));
    return st(hipStreamSynchronize(c->stream));
} NKV_CATCH

}  // extern "C"
