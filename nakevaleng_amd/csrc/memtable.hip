// memtable.hip -- the memtable flush on the device (core/memtable/memtable.go:93-116
// over core/skiplist/skiplist.go:62-120): nkv_sort_records_dev / nkv_sort_records.
// A write log in arrival order in, the flushed Data table out: one record per
// distinct key in ascending bytes.Compare order, the last arrival of each key
// kept, every record copied byte for byte.
//
// The order sorted by is total: (key ascending, arrival index ascending).  No
// two entries compare equal, so the result does not depend on the algorithm.
//
// Stages, all on the context's stream:
//   k_sort_validate  one lane per record: header bounds, the record ends where
//                    the next starts; writes the dense entries (first 8 key
//                    bytes big-endian zero-padded, KeySize, TotalSize).  The
//                    host reads its error word before anything else is launched.
//   k_sort_tile      one workgroup sorts a tile of T = 1024 records in LDS as
//                    (prefix u64, arrival index u32) pairs, 12 KiB, by a bitonic
//                    network of 55 steps; a lane owns two compare-exchanges per
//                    step.  Slots past n hold a sentinel that sorts last and is
//                    not stored.  T = 1024: the largest tile at which a 256-lane
//                    workgroup still keeps 2 exchanges per lane and step, and
//                    at 12 KiB per workgroup LDS never bounds the occupancy.
//                    LDS layout: element e lies at slot e ^ 31 when bit 5 of e
//                    is set, else at e.  The 32 lanes of a half-wave work on 64
//                    consecutive elements; for a compare distance j < 32 the
//                    "low" elements of the two 32-element blocks would meet in
//                    the same banks, and reversing every second block puts them
//                    on the complementary ones (8-byte reads: bank pair = slot
//                    mod 32; 4-byte reads: bank = slot mod 32).
//   k_sort_merge     ceil(log2(ceil(n / T))) passes, one lane per record: runs
//                    of L = T 2^p are merged pairwise by rank.  The record at
//                    local index i of a run finds by binary search how many
//                    records of the sibling run are smaller (strictly: the
//                    order is total, both sides use the same bound) and stores
//                    its pair at i + that count in the other buffer; a run with
//                    no sibling is copied through.  The prefix travels with the
//                    index, so a probe reads one dense array and touches the
//                    log only when two keys longer than 8 bytes share 8 bytes.
//   k_sort_survive   one lane per sorted position s: it survives iff s = n - 1
//                    or the key at s + 1 differs; flag, TotalSize (0 for the
//                    shadowed) and arrival index at slot s.
//   scans            exclusive sums of the flags (output index) and the sizes
//                    (output offset), then k_sort_scatter writes d_out_off /
//                    d_out_src / source addresses and the totals.
//   k_merge_copy     the merge's copy kernel (merge_copy_dev.hpp), unchanged.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "bytes_dev.hpp"  // ld_le64, cmp_bytes
#include "context.hpp"
#include "merge_copy_dev.hpp"  // k_merge_copy, kCopyTile

using namespace nkv;

namespace {

constexpr int kHdr = 30;  // record.go:191-199: Crc 4 | Timestamp 8 | Status 1 | TypeInfo 1 | KeySize 8 | ValueSize 8
constexpr uint32_t kTile = 1024;              // T: records one workgroup sorts in LDS
constexpr uint32_t kSentinel = 0xFFFFFFFFu;   // arrival index of a slot past n (n <= 2^31 - 1)

struct Log {  // kernel argument: the write log
    const uint8_t* s;
    uint64_t len;
    const uint64_t* off;
};

// Dense arrays over the log's records, by arrival index (Dense of merge.hip
// without the timestamp).
struct Dense {
    uint64_t* pfx;   // first 8 key bytes, big-endian, zero-padded
    uint64_t* klen;  // KeySize
    uint64_t* size;  // TotalSize
};

__global__ __launch_bounds__(kBlock) void k_sort_validate(Log G, uint32_t n, Dense D, unsigned int* err) {
    const uint64_t gg = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (gg >= n) return;
    const uint32_t i = uint32_t(gg);
    const uint64_t o = G.off[i];
    bool bad = (i == 0 && o != 0) || !header_in(o, G.len);
    if (!bad) {
        const uint64_t ks = ld_le64(G.s + o + 14), vs = ld_le64(G.s + o + 22);
        const uint64_t room = G.len - o - kHdr;
        if (ks > room || vs > room - ks) {
            bad = true;
        } else {
            const uint64_t end = o + kHdr + ks + vs;  // <= len: no overflow
            const uint64_t next = i + 1 < n ? G.off[i + 1] : G.len;
            if (end != next) bad = true;
            const uint8_t* key = G.s + o + kHdr;
            uint64_t p = 0;
            for (uint32_t b = 0; b < 8 && b < ks; ++b) p |= uint64_t(key[b]) << (56 - 8 * b);
            D.pfx[i] = p;
            D.klen[i] = ks;
            D.size[i] = kHdr + ks + vs;
        }
    }
    if (bad) atomicOr(err, 1u);
}

// Keys of the validated records at arrival indices a and b, whose prefixes are
// pa and pb: cmp_key of merge.hip.  The log is read only when both keys are
// longer than 8 bytes and share their first 8.
__device__ inline int cmp_key(const Log& G, const Dense& D, uint64_t pa, uint32_t a, uint64_t pb, uint32_t b) {
    if (pa != pb) return pa < pb ? -1 : 1;
    const uint64_t la = D.klen[a], lb = D.klen[b];
    if (la <= 8 || lb <= 8) return la < lb ? -1 : (la > lb ? 1 : 0);
    return cmp_bytes(G.s + G.off[a] + kHdr + 8, la - 8, G.s + G.off[b] + kHdr + 8, lb - 8);
}

// The total order: key ascending, then arrival index ascending.
__device__ inline bool before(const Log& G, const Dense& D, uint64_t pa, uint32_t a, uint64_t pb, uint32_t b) {
    const int c = cmp_key(G, D, pa, a, pb, b);
    return c < 0 || (c == 0 && a < b);
}

// The same with sentinels, which carry prefix ~0 and sort behind every record
// (two sentinels are equal: neither is before the other).
__device__ inline bool tile_before(const Log& G, const Dense& D, uint64_t pa, uint32_t a, uint64_t pb, uint32_t b) {
    if (pa != pb) return pa < pb;
    if (a == kSentinel || b == kSentinel) return a != kSentinel;
    return before(G, D, pa, a, pb, b);
}

__device__ __forceinline__ uint32_t slot_of(uint32_t e) { return (e & 32) ? e ^ 31 : e; }

__global__ __launch_bounds__(kBlock) void k_sort_tile(Log G, uint32_t n, Dense D, uint64_t* __restrict__ opfx,
                                                      uint32_t* __restrict__ oidx) {
    __shared__ uint64_t l_pfx[kTile];
    __shared__ uint32_t l_idx[kTile];
    const uint64_t base = uint64_t(blockIdx.x) * kTile;
    for (uint32_t e = threadIdx.x; e < kTile; e += kBlock) {
        const uint64_t g = base + e;
        const uint32_t w = slot_of(e);
        l_pfx[w] = g < n ? D.pfx[g] : ~uint64_t(0);
        l_idx[w] = g < n ? uint32_t(g) : kSentinel;
    }
    __syncthreads();
#pragma unroll 1
    for (uint32_t k = 2; k <= kTile; k <<= 1) {
#pragma unroll 1
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = threadIdx.x; t < kTile / 2; t += kBlock) {
                const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
                const uint32_t wi = slot_of(i), wp = slot_of(p);
                const uint64_t pa = l_pfx[wi], pb = l_pfx[wp];
                const uint32_t a = l_idx[wi], b = l_idx[wp];
                const bool up = (i & k) == 0;  // this block of k ascends
                const bool swap = up ? tile_before(G, D, pb, b, pa, a) : tile_before(G, D, pa, a, pb, b);
                if (swap) {
                    l_pfx[wi] = pb;
                    l_pfx[wp] = pa;
                    l_idx[wi] = b;
                    l_idx[wp] = a;
                }
            }
            __syncthreads();
        }
    }
    for (uint32_t e = threadIdx.x; e < kTile; e += kBlock) {
        const uint64_t g = base + e;
        if (g >= n) break;  // the sentinels sorted behind the tile's records
        const uint32_t w = slot_of(e);
        opfx[g] = l_pfx[w];
        oidx[g] = l_idx[w];
    }
}

__global__ __launch_bounds__(kBlock) void k_sort_merge(Log G, uint32_t n, Dense D, uint64_t L,
                                                       const uint64_t* __restrict__ ipfx,
                                                       const uint32_t* __restrict__ iidx,
                                                       uint64_t* __restrict__ opfx, uint32_t* __restrict__ oidx) {
    const uint64_t g = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (g >= n) return;
    const uint64_t r = g / L;             // this record's run
    const uint64_t sb = (r ^ 1) * L;      // where the sibling run starts
    const uint64_t pa = ipfx[g];
    const uint32_t a = iidx[g];
    uint64_t dst = g;                     // no sibling: copied through
    if (sb < n) {
        const uint64_t cnt = n - sb < L ? n - sb : L;
        uint64_t lo = 0, hi = cnt;        // records of the sibling before this one
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (before(G, D, ipfx[sb + mid], iidx[sb + mid], pa, a)) lo = mid + 1;
            else hi = mid;
        }
        dst = (r & ~uint64_t(1)) * L + (g - r * L) + lo;
    }
    opfx[dst] = pa;
    oidx[dst] = a;
}

__global__ __launch_bounds__(kBlock) void k_sort_survive(Log G, uint32_t n, Dense D, const uint64_t* __restrict__ pfx,
                                                         const uint32_t* __restrict__ idx, uint64_t* __restrict__ flag,
                                                         uint64_t* __restrict__ osize, uint64_t* __restrict__ osrc) {
    const uint64_t s = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (s >= n) return;
    const uint32_t a = idx[s];
    // equal keys lie in arrival order: the last of them is the record the skiplist holds
    const bool keep = s + 1 == n || cmp_key(G, D, pfx[s], a, pfx[s + 1], idx[s + 1]) != 0;
    flag[s] = keep ? 1 : 0;
    osize[s] = keep ? D.size[a] : 0;
    osrc[s] = a;
}

__global__ __launch_bounds__(kBlock) void k_sort_scatter(Log G, uint32_t n, const uint64_t* __restrict__ flag,
                                                         const uint64_t* __restrict__ idx,
                                                         const uint64_t* __restrict__ osize,
                                                         const uint64_t* __restrict__ ooff,
                                                         const uint64_t* __restrict__ osrc,
                                                         uint64_t* __restrict__ out_off, uint64_t* __restrict__ out_src,
                                                         uint64_t* __restrict__ src_addr, uint64_t* __restrict__ totals) {
    const uint64_t s = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (s >= n) return;
    if (flag[s]) {
        const uint64_t j = idx[s], a = osrc[s];
        out_off[j] = ooff[s];
        if (out_src) out_src[j] = a;
        src_addr[j] = uint64_t(reinterpret_cast<uintptr_t>(G.s + G.off[a]));
    }
    if (s == n - 1) {
        totals[0] = idx[s] + flag[s];
        totals[1] = ooff[s] + osize[s];
    }
}

inline unsigned blocks_for(uint64_t n) { return unsigned((n + kBlock - 1) / kBlock); }

}  // namespace

extern "C" {

int nkv_sort_records_dev(nkv_ctx* c, const void* d_log, uint64_t log_len, const uint64_t* d_rec_off, uint64_t n,
                         void* d_out, uint64_t out_cap, uint64_t* d_out_off, uint64_t* d_out_src, uint64_t* n_out,
                         uint64_t* out_len) try {
    TRY(bind(c));
    if (!n_out || !out_len || n > kMaxN) return NKV_ERR_INVALID;
    if (n ? (!d_log || !d_rec_off || log_len / kHdr < n) : log_len != 0) return NKV_ERR_INVALID;
    const uint64_t tiles = log_len / kCopyTile + 2;  // the copy's grid: d_out's 16-byte grid over at most log_len bytes
    if (out_cap < log_len || tiles > 0x7fffffffull) return NKV_ERR_INVALID;
    *n_out = 0;
    *out_len = 0;
    if (n == 0) return NKV_OK;
    if (!d_out || !d_out_off) return NKV_ERR_INVALID;
    const Log G{static_cast<const uint8_t*>(d_log), log_len, d_rec_off};

    // scratch in d_stmp (nothing in it outlives the call): nine u64 arrays of n,
    // then the two pair buffers (u64 prefixes, u32 arrival indices)
    const uint64_t n2 = (n + 1) & ~uint64_t(1);  // u32 arrays of n2 keep what follows 8-byte aligned
    TRY(grow(c->d_stmp, 9 * 8 * n + 2 * (8 * n + 4 * n2)));
    uint64_t* a = static_cast<uint64_t*>(c->d_stmp.p);
    const Dense D{a, a + n, a + 2 * n};
    uint64_t *flag = a + 3 * n, *osize = a + 4 * n, *osrc = a + 5 * n, *idx = a + 6 * n, *ooff = a + 7 * n,
             *src_addr = a + 8 * n;
    uint64_t* pfx[2] = {a + 9 * n, a + 10 * n};
    uint32_t* arr[2] = {reinterpret_cast<uint32_t*>(a + 11 * n), reinterpret_cast<uint32_t*>(a + 11 * n) + n2};
    size_t tb = 0;
    HIPTRY(scan_exclusive_u64(flag, idx, n, nullptr, &tb, c->stream));
    TRY(grow(c->d_tmp, tb));
    TRY(grow(c->d_stats, 24));
    unsigned int* err = static_cast<unsigned int*>(c->d_stats.p);
    uint64_t* totals = static_cast<uint64_t*>(c->d_stats.p) + 1;
    const uint32_t n32 = uint32_t(n);

    // validation first: nothing that follows an offset or copies a record is
    // launched unless every header and offset checked out
    HIPTRY(hipMemsetAsync(err, 0, 24, c->stream));
    hipLaunchKernelGGL(k_sort_validate, dim3(blocks_for(n)), dim3(kBlock), 0, c->stream, G, n32, D, err);
    HIPTRY(hipGetLastError());
    unsigned int h_err = 0;
    HIPTRY(hipMemcpyAsync(&h_err, err, 4, hipMemcpyDeviceToHost, c->stream));
    HIPTRY(hipStreamSynchronize(c->stream));
    if (h_err) return NKV_ERR_INVALID;

    // with NKV_TIMING_EVENTS: "leaf" = sort + survive + scans + scatter, "reduce" = the copy kernel
    TRY(mark(c, 0));
    const uint64_t ntiles = (n + kTile - 1) / kTile;
    hipLaunchKernelGGL(k_sort_tile, dim3(unsigned(ntiles)), dim3(kBlock), 0, c->stream, G, n32, D, pfx[0], arr[0]);
    HIPTRY(hipGetLastError());
    int cur = 0;
    for (uint64_t L = kTile; L < n; L *= 2) {  // runs of L into runs of 2 L
        hipLaunchKernelGGL(k_sort_merge, dim3(blocks_for(n)), dim3(kBlock), 0, c->stream, G, n32, D, L, pfx[cur],
                           arr[cur], pfx[cur ^ 1], arr[cur ^ 1]);
        HIPTRY(hipGetLastError());
        cur ^= 1;
    }
    hipLaunchKernelGGL(k_sort_survive, dim3(blocks_for(n)), dim3(kBlock), 0, c->stream, G, n32, D, pfx[cur], arr[cur],
                       flag, osize, osrc);
    HIPTRY(hipGetLastError());
    HIPTRY(scan_exclusive_u64(flag, idx, n, c->d_tmp.p, &tb, c->stream));
    HIPTRY(scan_exclusive_u64(osize, ooff, n, c->d_tmp.p, &tb, c->stream));
    hipLaunchKernelGGL(k_sort_scatter, dim3(blocks_for(n)), dim3(kBlock), 0, c->stream, G, n32, flag, idx, osize, ooff,
                       osrc, d_out_off, d_out_src, src_addr, totals);
    HIPTRY(hipGetLastError());
    TRY(mark(c, 1));
    // out_len is known on the device only: the grid covers the bound (log_len),
    // and tiles past out_len leave at once
    hipLaunchKernelGGL(k_merge_copy, dim3(unsigned(tiles)), dim3(kBlock), 0, c->stream, static_cast<uint8_t*>(d_out),
                       d_out_off, src_addr, totals);
    HIPTRY(hipGetLastError());
    TRY(mark(c, 2));
    uint64_t h_tot[2] = {0, 0};
    HIPTRY(hipMemcpyAsync(h_tot, totals, 16, hipMemcpyDeviceToHost, c->stream));
    HIPTRY(hipStreamSynchronize(c->stream));
    *n_out = h_tot[0];
    *out_len = h_tot[1];
    return NKV_OK;
} NKV_CATCH

int nkv_sort_records(nkv_ctx* c, const uint8_t* log, uint64_t log_len, const uint64_t* rec_size, uint64_t n,
                     uint8_t* out, uint64_t out_cap, uint64_t* out_rec_size, uint64_t* n_out, uint64_t* out_len) try {
    TRY(bind(c));
    if (!n_out || !out_len || n > kMaxN || (n && (!log || !rec_size))) return NKV_ERR_INVALID;
    uint64_t left = log_len;  // the sizes add up to the log exactly, term by term (no wrapped sum)
    for (uint64_t i = 0; i < n; ++i) {
        if (rec_size[i] > left) return NKV_ERR_INVALID;
        left -= rec_size[i];
    }
    if (left != 0 || log_len > (uint64_t(1) << 62) || out_cap < log_len) return NKV_ERR_INVALID;
    *n_out = 0;
    *out_len = 0;
    if (n == 0) return NKV_OK;
    if (!out || !out_rec_size) return NKV_ERR_INVALID;
    TRY(grow(c->d_data, (log_len + 15) & ~uint64_t(15)));
    TRY(grow(c->d_len, 8 * n));
    TRY(grow(c->d_off, 8 * n));
    TRY(grow(c->d_nodes, log_len));
    TRY(grow(c->d_tmp2, 8 * n));
    uint64_t* d_size = static_cast<uint64_t*>(c->d_len.p);
    uint64_t* d_off = static_cast<uint64_t*>(c->d_off.p);
    uint64_t* d_out_off = static_cast<uint64_t*>(c->d_tmp2.p);
    HIPTRY(hipMemcpyAsync(c->d_data.p, log, log_len, hipMemcpyHostToDevice, c->stream));
    HIPTRY(hipMemcpyAsync(d_size, rec_size, 8 * n, hipMemcpyHostToDevice, c->stream));
    TRY(nkv_record_offsets_dev(c, d_size, n, d_off));
    TRY(nkv_sort_records_dev(c, c->d_data.p, log_len, d_off, n, c->d_nodes.p, log_len, d_out_off, nullptr, n_out,
                             out_len));
    if (*n_out == 0) return NKV_OK;
    std::vector<uint64_t> off(*n_out);
    HIPTRY(hipMemcpyAsync(out, c->d_nodes.p, *out_len, hipMemcpyDeviceToHost, c->stream));
    HIPTRY(hipMemcpyAsync(off.data(), d_out_off, 8 * *n_out, hipMemcpyDeviceToHost, c->stream));
    HIPTRY(hipStreamSynchronize(c->stream));
    for (uint64_t j = 0; j < *n_out; ++j) out_rec_size[j] = (j + 1 < *n_out ? off[j + 1] : *out_len) - off[j];
    return NKV_OK;
} NKV_CATCH

}  // extern "C"
