// locate.hip -- the readers of the Index and Summary tables on the device, for
// tables whose Data file stays on disk: nkv_index_open_dev / nkv_locate_dev.
//
// The reference's get (engine/coreeng/coreeng.go:99-160) names one Data offset
// per key through Filter.Query, FindSummaryTableEntry (summarytable.go:129-178)
// and FindIndexTableEntry (indextable.go:64-92).  On a canonical pair (the six
// conditions in include/nkv_merkle.h, "index lookup") the two Find steps have a
// closed form over the Index keys alone, so a table is opened once -- its Index
// entries' offsets found and the pair validated -- and then searched by offset.
//
// Both images are chains of KeySize u64 | Offset i64 | Key entries with no
// offsets beside them.  Open, in order (the host reads a verdict between the
// steps; the call is synchronous because it hands n to the host):
//   header            24 bytes to the host: MinKeySize, MaxKeySize, Payload.
//   Summary chain     k_chain_walk: one lane follows the payload (path 1), or
//                     k_summary_chunks: one lane per kChunk payload bytes starts
//                     at the first position of its chunk that passes the link
//                     test (the Index at Offset holds the same KeySize and Key)
//                     and walks to the first chain position past its chunk.  The
//                     host stitches the (start, landing, count) triples from
//                     lane 0 on: a chunk the chain enters must have started
//                     exactly at the previous used lane's landing, so every
//                     accepted entry is on the true chain.  A mismatch (a decoy
//                     in front of the true position, a broken chain) falls back
//                     to the one-lane walk: same bytes, slower.
//                     k_summary_write then writes the entries' positions.
//   Index chain       k_links holds every Summary entry to the link test and
//                     the named offsets to strict ascent from 0; k_pages walks
//                     one lane per page from its entry's Offset and must land
//                     exactly on the next one's (the last page: one entry, ending
//                     at index_len).  Any failure falls back to the one-lane walk
//                     of the Index from 0 and k_links_exact over its offsets,
//                     which alone tell a broken Index chain from a bad link.
//   order and range   k_order: one lane per entry compares K_i with K_(i+1) by
//                     the 8-byte prefix first (record_dev.hpp cmp_prefixed); the
//                     two ends against MinKey and MaxKey.
// Every chain loop advances at least 16 bytes and never past its image; the
// start search of a chunk looks at no more than kChunk positions.  No
// workgroup waits on another.
//
// Locate: k_locate, the search layer's kernel (search_dev.hpp) over the entry
// format: the key lies behind the two fields, and a found entry answers LOCATED
// with its stored Offset.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "bytes_dev.hpp"
#include "context.hpp"
#include "search_dev.hpp"

using namespace nkv;

namespace {

constexpr uint64_t kNone = ~uint64_t(0);
constexpr uint64_t kEnt = 16;  // KeySize + Offset in front of every entry's key
// verdict bits raised on the device before the host names the stage
constexpr uint32_t kFlagLink = 1, kFlagPage = 2;

__device__ __forceinline__ bool same_bytes(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b, uint64_t n) {
    for (uint64_t i = 0; i < n; ++i)
        if (a[i] != b[i]) return false;
    return true;
}

// The link test of payload position p: an entry lies there, its Offset (read as
// unsigned, so a negative one is out of range) names an Index entry with the
// same KeySize, and the key bytes are the same.
__device__ __forceinline__ bool link_ok(const uint8_t* __restrict__ P, uint64_t PL, uint64_t p,
                                        const uint8_t* __restrict__ I, uint64_t IL, uint64_t* at) {
    uint64_t ks, iks;
    if (!entry_in(P, PL, p, &ks)) return false;
    const uint64_t o = ld_le64(P + p + 8);
    if (!entry_in(I, IL, o, &iks) || iks != ks) return false;
    *at = o;
    return same_bytes(P + p + kEnt, I + o + kEnt, ks);
}

// Follow the chain of img from pos to the first position >= limit (<= L);
// out (nullable) receives the positions.  *land = kNone: an entry on the way
// does not fit the image.  At least 16 bytes per step.
__device__ __forceinline__ void walk(const uint8_t* __restrict__ img, uint64_t L, uint64_t pos, uint64_t limit,
                                     uint64_t* __restrict__ out, uint64_t* land, uint64_t* count) {
    uint64_t c = 0;
    while (pos < limit) {
        uint64_t ks;
        if (!entry_in(img, L, pos, &ks)) {
            pos = kNone;
            break;
        }
        if (out) out[c] = pos;
        ++c;
        pos += kEnt + ks;
    }
    *land = pos;
    *count = c;
}

// The whole chain by one lane: res[0] = landing (L, or kNone), res[1] = entries.
__global__ void k_chain_walk(const uint8_t* __restrict__ img, uint64_t L, uint64_t* __restrict__ out,
                             uint64_t* __restrict__ res) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    walk(img, L, 0, L, out, &res[0], &res[1]);
}

struct Triple {
    uint64_t start, land, count;  // start kNone: no candidate in the chunk; land kNone: the walk broke
};

__global__ __launch_bounds__(kBlock) void k_summary_chunks(const uint8_t* __restrict__ P, uint64_t PL,
                                                           const uint8_t* __restrict__ I, uint64_t IL, uint64_t K,
                                                           uint64_t W, Triple* __restrict__ tr) {
    const uint64_t w = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (w >= W) return;
    const uint64_t lo = w * K, hi = PL - lo > K ? lo + K : PL;
    uint64_t start = w == 0 ? 0 : kNone, at;
    for (uint64_t p = lo; w != 0 && p < hi; ++p) {  // at most K positions
        if (link_ok(P, PL, p, I, IL, &at)) {
            start = p;
            break;
        }
    }
    Triple t{start, kNone, 0};
    if (start != kNone) walk(P, PL, start, hi, nullptr, &t.land, &t.count);
    tr[w] = t;
}

// base[w] != kNone: the stitch uses lane w, whose entries are base[w] .. of the chain
__global__ __launch_bounds__(kBlock) void k_summary_write(const uint8_t* __restrict__ P, uint64_t PL, uint64_t K,
                                                          uint64_t W, const Triple* __restrict__ tr,
                                                          const uint64_t* __restrict__ base,
                                                          uint64_t* __restrict__ soff) {
    const uint64_t w = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (w >= W || base[w] == kNone) return;
    const uint64_t lo = w * K, hi = PL - lo > K ? lo + K : PL;
    uint64_t land, count;
    walk(P, PL, tr[w].start, hi, soff + base[w], &land, &count);
}

// Summary entry e against the Index: the link test, entry 0 at offset 0, the
// named offsets strictly ascending.  ioff[e] = the named offset (0 where the
// entry fails, so that the page walk stays defined).
__global__ __launch_bounds__(kBlock) void k_links(const uint8_t* __restrict__ P, uint64_t PL,
                                                  const uint64_t* __restrict__ soff, uint64_t s,
                                                  const uint8_t* __restrict__ I, uint64_t IL,
                                                  uint64_t* __restrict__ ioff, unsigned int* __restrict__ err) {
    const uint64_t e = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (e >= s) return;
    uint64_t at = 0;
    bool ok = link_ok(P, PL, soff[e], I, IL, &at);
    if (!ok) at = 0;
    if (e == 0 && at != 0) ok = false;
    if (e + 1 < s && ld_le64(P + soff[e + 1] + 8) <= at) ok = false;  // soff[e + 1] is a chain position: in the payload
    ioff[e] = at;
    if (!ok) atomicOr(err, kFlagLink);
}

// Page e: the Index entries from ioff[e] up to ioff[e + 1] (the last page: to
// the end of the image, and exactly one entry).  pcount[e] = its entries.
__global__ __launch_bounds__(kBlock) void k_pages(const uint8_t* __restrict__ I, uint64_t IL,
                                                  const uint64_t* __restrict__ ioff, uint64_t s,
                                                  uint64_t* __restrict__ pcount, uint64_t* __restrict__ pbase,
                                                  uint64_t* __restrict__ ent, unsigned int* __restrict__ err) {
    const uint64_t e = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (e >= s) return;
    uint64_t target = e + 1 < s ? ioff[e + 1] : IL;
    bool ok = target <= IL;
    if (!ok) target = IL;
    uint64_t land, count;
    walk(I, IL, ioff[e], target, ent ? ent + pbase[e] : nullptr, &land, &count);
    if (land != target || (e + 1 == s && count != 1)) ok = false;
    if (!ent) {
        pcount[e] = count;
        if (!ok) atomicOr(err, kFlagPage);
    }
}

// The exact form of k_links, over the offsets ent[0..n) of a whole Index chain:
// the named offset is entry j's, entry 0 names j = 0, the last names n - 1.
__global__ __launch_bounds__(kBlock) void k_links_exact(const uint8_t* __restrict__ P, uint64_t PL,
                                                        const uint64_t* __restrict__ soff, uint64_t s,
                                                        const uint8_t* __restrict__ I, uint64_t IL,
                                                        const uint64_t* __restrict__ ent, uint64_t n,
                                                        unsigned int* __restrict__ err) {
    const uint64_t e = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (e >= s) return;
    uint64_t at = 0;
    bool ok = link_ok(P, PL, soff[e], I, IL, &at);
    if (ok) {
        const uint64_t j = last_at_most(ent, uint64_t(0), n, at);  // ent[0] = 0 <= at
        ok = ent[j] == at && (e != 0 || j == 0) && (e + 1 != s || j == n - 1);
        if (e + 1 < s && ld_le64(P + soff[e + 1] + 8) <= at) ok = false;
    }
    if (!ok) atomicOr(err, kFlagLink);
}

__device__ __forceinline__ int cmp_keys(const uint8_t* a, uint64_t la, const uint8_t* b, uint64_t lb) {
    return cmp_prefixed(key_prefix(a, la), la, a + 8, key_prefix(b, lb), lb, b + 8);
}

// K_i < K_(i+1) for every i, MinKey = K_0, MaxKey = K_(n-1).  ent holds the
// offsets of a validated chain: every entry lies in the image.  hdr = the
// Summary image, whose two keys lie behind its 24-byte header.
__global__ __launch_bounds__(kBlock) void k_order(const uint8_t* __restrict__ I, const uint64_t* __restrict__ ent,
                                                  uint64_t n, const uint8_t* __restrict__ hdr, uint64_t minks,
                                                  uint64_t maxks, unsigned int* __restrict__ err) {
    const uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint8_t* a = I + ent[i];
    const uint64_t la = ld_le64(a);
    unsigned int bad = 0;
    if (i + 1 < n) {
        const uint8_t* b = I + ent[i + 1];
        if (cmp_keys(a + kEnt, la, b + kEnt, ld_le64(b)) >= 0) bad |= NKV_INDEX_BAD_ORDER;
    }
    if (i == 0 && (la != minks || !same_bytes(a + kEnt, hdr + 24, la))) bad |= NKV_INDEX_BAD_RANGE;
    if (i == n - 1 && (la != maxks || !same_bytes(a + kEnt, hdr + 24 + minks, la))) bad |= NKV_INDEX_BAD_RANGE;
    if (bad) atomicOr(err, bad);
}

// ---------------------------------------------------------------------------
// locate

// The entry format of an Index table: KeySize | Offset | Key; a found entry
// answers LOCATED and its stored Offset.  An entry whose file says -1 reads as a
// miss (coreeng.go:138 tests the stored field).
struct IndexFormat {
    static constexpr uint64_t kKeyAt = kEntryHdr;
    static constexpr bool kOverlay = true;
    NKV_HD static bool key_in(const uint8_t* img, uint64_t L, uint64_t o, uint64_t* ks) {
        return entry_in(img, L, o, ks);
    }
    int overlay;        // the call's: answered queries are left as they are
    int64_t* data_off;  // the call's output
    int64_t d = -1;     // this query's
    __device__ bool answer(const uint8_t* ent, uint8_t* st) {
        const int64_t stored = int64_t(ld_le64(ent + 8));
        if (stored == -1) return false;
        d = stored;
        *st = NKV_GET_LOCATED;
        return true;
    }
    __device__ void store(uint64_t i) const { data_off[i] = d; }
};

__global__ __launch_bounds__(kBlock) void k_locate(Tables R, const uint8_t* __restrict__ keys,
                                                   const uint64_t* __restrict__ koff,
                                                   const uint64_t* __restrict__ klen, uint64_t q, int overlay,
                                                   uint64_t* __restrict__ hit, int64_t* __restrict__ data_off,
                                                   uint8_t* __restrict__ status, uint8_t* __restrict__ stage,
                                                   unsigned int* __restrict__ err) {
    search_tables(R, IndexFormat{overlay, data_off}, keys, koff, klen, q, hit, status, stage, err);
}

// nkv_index_table as the search layer reads it
TableView view_of(const nkv_index_table& u) {
    return {u.index, u.index_len, u.ent_off, u.n, u.bits, u.m, u.k, u.seed0};
}

// ---------------------------------------------------------------------------
// open, host side

// Payload bytes from which NKV_OPT_INDEX_OPEN_PATH 0 takes the chunked walk,
// and its default bytes per lane.  Measured (DESIGN.md "Index lookup"): at
// page size 3 the two paths cost the same at an 11 KB payload (0.19 / 0.20 ms,
// launches and the host's reads) and the walk loses from 44 KB on (0.38 / 0.20
// ms); 1 KiB and 4 KiB per lane are within 5 % of each other, 256 B and
// 16 KiB slower.
constexpr uint64_t kAutoChunkedFrom = uint64_t(16) << 10;
constexpr uint64_t kChunkDefault = 4096;

struct Flags {  // c->d_stats: the device's words for the host
    unsigned int* err;
    uint64_t* res;  // behind it: [0] landing, [1] count of k_chain_walk; [2] the scan's total
};

// h[0] = the error word, h[1..3] = res[0..2]
int read_flags(nkv_ctx* c, const Flags& f, uint64_t h[4]) {
    HIPTRY(hipMemcpyAsync(h, f.err, 32, hipMemcpyDeviceToHost, c->stream));
    return st(hipStreamSynchronize(c->stream));
}

// The Summary chain's s positions into soff.  *s = 0: the chain is not whole.
int summary_chain(nkv_ctx* c, const uint8_t* P, uint64_t PL, const uint8_t* I, uint64_t IL, bool chunked, uint64_t K,
                  uint64_t W, Triple* tr, uint64_t* base, uint64_t* soff, const Flags& f, uint64_t* s) {
    uint64_t h[4];
    *s = 0;
    if (chunked) {
        hipLaunchKernelGGL(k_summary_chunks, dim3(blocks_for(W)), dim3(kBlock), 0, c->stream, P, PL, I, IL, K, W, tr);
        HIPTRY(hipGetLastError());
        std::vector<Triple> t(W);
        HIPTRY(hipMemcpyAsync(t.data(), tr, W * sizeof(Triple), hipMemcpyDeviceToHost, c->stream));
        HIPTRY(hipStreamSynchronize(c->stream));
        // the stitch: from lane 0, every chunk the chain enters must have
        // started at the landing of the lane before
        std::vector<uint64_t> b(W, kNone);
        uint64_t pos = 0, total = 0;
        bool ok = true;
        while (pos < PL) {
            const uint64_t w = pos / K;
            if (t[w].start != pos || t[w].land == kNone) {
                ok = false;
                break;
            }
            b[w] = total;
            total += t[w].count;
            pos = t[w].land;  // >= (w + 1) K: the loop takes every lane at most once
        }
        if (ok) {
            HIPTRY(hipMemcpyAsync(base, b.data(), W * 8, hipMemcpyHostToDevice, c->stream));
            hipLaunchKernelGGL(k_summary_write, dim3(blocks_for(W)), dim3(kBlock), 0, c->stream, P, PL, K, W, tr, base,
                               soff);
            HIPTRY(hipGetLastError());
            HIPTRY(hipStreamSynchronize(c->stream));  // b leaves scope
            *s = total;
            return NKV_OK;
        }
    }
    hipLaunchKernelGGL(k_chain_walk, dim3(1), dim3(1), 0, c->stream, P, PL, soff, f.res);
    HIPTRY(hipGetLastError());
    TRY(read_flags(c, f, h));
    if (h[1] == PL) *s = h[2];
    return NKV_OK;
}

}  // namespace

extern "C" {

int nkv_index_open_dev(nkv_ctx* c, const void* d_index, uint64_t index_len, const void* d_summary,
                       uint64_t summary_len, uint64_t* d_ent_off, uint64_t ent_cap, uint64_t* n_out, uint64_t* s_out,
                       uint32_t* verdict) try {
    TRY(bind(c));
    if (!d_index || !d_summary || !n_out || !s_out || !verdict || index_len == 0 || summary_len == 0)
        return NKV_ERR_INVALID;
    *n_out = 0;
    *s_out = 0;
    *verdict = 0;
    const uint8_t* I = static_cast<const uint8_t*>(d_index);
    const uint8_t* S = static_cast<const uint8_t*>(d_summary);
    const uint64_t IL = index_len;
    const auto refuse = [&](uint32_t bit) {
        *verdict = bit;
        return NKV_OK;
    };

    // 1: the header, MinKey, MaxKey and Payload bytes lie in the image
    if (summary_len < 24) return refuse(NKV_INDEX_BAD_HEADER);
    uint64_t hd[3];
    HIPTRY(hipMemcpyAsync(hd, S, 24, hipMemcpyDeviceToHost, c->stream));
    HIPTRY(hipStreamSynchronize(c->stream));
    const uint64_t minks = hd[0], maxks = hd[1], PL = hd[2];
    uint64_t room = summary_len - 24;
    if (minks > room || maxks > room - minks || PL > room - minks - maxks) return refuse(NKV_INDEX_BAD_HEADER);
    const uint8_t* P = S + 24 + minks + maxks;
    if (PL < kEnt) return refuse(NKV_INDEX_BAD_SUMMARY_CHAIN);  // s = 0, or less than one entry

    // scratch in d_stmp, which carries nothing from call to call
    const uint64_t K = c->index_open_chunk ? uint64_t(c->index_open_chunk) : kChunkDefault;
    const bool chunked = c->index_open_path == 2 || (c->index_open_path == 0 && PL >= kAutoChunkedFrom);
    const uint64_t W = (PL + K - 1) / K;
    const uint64_t smax = PL / kEnt, nmax = IL / kEnt + 1;
    Triple* tr;
    uint64_t *base, *soff, *ioff, *pcount, *pbase, *ent;
    const auto carve = [&](Carver k) {
        tr = k.take<Triple>(chunked ? W : 0);
        base = k.take<uint64_t>(chunked ? W : 0);
        soff = k.take<uint64_t>(smax);
        ioff = k.take<uint64_t>(smax);
        pcount = k.take<uint64_t>(smax);
        pbase = k.take<uint64_t>(smax + 1);
        ent = k.take<uint64_t>(nmax);
        return k.bytes();
    };
    TRY(grow(c->d_stmp, carve(Carver())));
    carve(Carver(c->d_stmp.p));
    TRY(grow(c->d_stats, 32));
    const Flags f{static_cast<unsigned int*>(c->d_stats.p), static_cast<uint64_t*>(c->d_stats.p) + 1};
    uint64_t h[4];
    HIPTRY(hipMemsetAsync(f.err, 0, 32, c->stream));

    // 2: the payload is a whole chain of s >= 1 entries
    uint64_t s = 0;
    TRY(summary_chain(c, P, PL, I, IL, chunked, K, W, tr, base, soff, f, &s));
    if (s == 0) return refuse(NKV_INDEX_BAD_SUMMARY_CHAIN);
    if (s > kMaxN) return NKV_ERR_INVALID;

    // 3 and 4, page-parallel: the links, then one lane per page
    size_t tb = 0;
    HIPTRY(scan_exclusive_u64(pcount, pbase, s, nullptr, &tb, c->stream));
    TRY(grow(c->d_tmp, tb));
    HIPTRY(hipMemsetAsync(f.err, 0, 32, c->stream));
    hipLaunchKernelGGL(k_links, dim3(blocks_for(s)), dim3(kBlock), 0, c->stream, P, PL, soff, s, I, IL, ioff, f.err);
    HIPTRY(hipGetLastError());
    hipLaunchKernelGGL(k_pages, dim3(blocks_for(s)), dim3(kBlock), 0, c->stream, I, IL, ioff, s, pcount, pbase,
                       static_cast<uint64_t*>(nullptr), f.err);
    HIPTRY(hipGetLastError());
    HIPTRY(scan_exclusive_u64(pcount, pbase, s, c->d_tmp.p, &tb, c->stream));
    hipLaunchKernelGGL(k_scan_total<uint64_t>, dim3(1), dim3(1), 0, c->stream, pcount, pbase, s, f.res + 2);
    HIPTRY(hipGetLastError());
    TRY(read_flags(c, f, h));
    uint64_t n = 0;
    if (uint32_t(h[0]) == 0) {
        n = h[3];  // <= index_len / 16: the pages are disjoint
        hipLaunchKernelGGL(k_pages, dim3(blocks_for(s)), dim3(kBlock), 0, c->stream, I, IL, ioff, s, pcount, pbase,
                           ent, f.err);
        HIPTRY(hipGetLastError());
    } else {  // the exact path: the Index chain from 0 by one lane, then the links over its offsets
        HIPTRY(hipMemsetAsync(f.err, 0, 32, c->stream));
        hipLaunchKernelGGL(k_chain_walk, dim3(1), dim3(1), 0, c->stream, I, IL, ent, f.res);
        HIPTRY(hipGetLastError());
        TRY(read_flags(c, f, h));
        if (h[1] != IL) return refuse(NKV_INDEX_BAD_INDEX_CHAIN);
        n = h[2];
        hipLaunchKernelGGL(k_links_exact, dim3(blocks_for(s)), dim3(kBlock), 0, c->stream, P, PL, soff, s, I, IL, ent,
                           n, f.err);
        HIPTRY(hipGetLastError());
        TRY(read_flags(c, f, h));
        if (uint32_t(h[0])) return refuse(NKV_INDEX_BAD_LINK);
    }
    if (n > kMaxN) return NKV_ERR_INVALID;

    // 5 and 6: the key order, MinKey and MaxKey
    HIPTRY(hipMemsetAsync(f.err, 0, 32, c->stream));
    hipLaunchKernelGGL(k_order, dim3(blocks_for(n)), dim3(kBlock), 0, c->stream, I, ent, n, S, minks, maxks, f.err);
    HIPTRY(hipGetLastError());
    TRY(read_flags(c, f, h));
    if (uint32_t(h[0])) return refuse(uint32_t(h[0]));

    *n_out = n;
    *s_out = s;
    if (!d_ent_off) return NKV_OK;  // size query
    if (ent_cap < n) return NKV_ERR_INVALID;
    HIPTRY(hipMemcpyAsync(d_ent_off, ent, 8 * n, hipMemcpyDeviceToDevice, c->stream));
    return st(hipStreamSynchronize(c->stream));
} NKV_CATCH

int nkv_locate_dev(nkv_ctx* c, const nkv_index_table* tables, int T, uint32_t table_base, const void* d_keys,
                   const uint64_t* d_koff, const uint64_t* d_klen, uint64_t q, int overlay, uint64_t* d_hit,
                   int64_t* d_data_off, uint8_t* d_status, uint8_t* d_stage, uint32_t* d_err) try {
    TRY(bind(c));
    Tables R;
    TRY(pack_tables(tables, T, table_base, view_of, &R));
    if (q > kMaxN) return NKV_ERR_INVALID;
    if (q == 0) return NKV_OK;
    if (!d_keys || !d_koff || !d_klen || !d_hit || !d_data_off || !d_status) return NKV_ERR_INVALID;
    unsigned int* err;
    TRY(verdict_word(c, d_err, &err));
    hipLaunchKernelGGL(k_locate, dim3(blocks_for(q)), dim3(kBlock), 0, c->stream, R,
                       static_cast<const uint8_t*>(d_keys), d_koff, d_klen, q, overlay ? 1 : 0, d_hit, d_data_off,
                       d_status, d_stage, err);
    HIPTRY(hipGetLastError());
    return finish_verdict(c, d_err, err);
} NKV_CATCH

}  // extern "C"
