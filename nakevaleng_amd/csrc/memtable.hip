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
//   k_sort_validate  one lane per record: its dense entry (record_dev.hpp
//                    dense_entry: the record's span, it ends where the next
//                    starts; the key's prefix, KeySize, TotalSize).  The host
//                    reads its error word before anything else is launched.
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
//   k_merge_copy     the copy kernel.  This tail is the merge's too
//                    (merge_copy_dev.hpp write_table).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "context.hpp"
#include "merge_copy_dev.hpp"  // Slots, scatter_slots, write_table, kCopyTile

using namespace nkv;

namespace {

constexpr uint32_t kTile = 1024;              // T: records one workgroup sorts in LDS
constexpr uint32_t kSentinel = 0xFFFFFFFFu;   // arrival index of a slot past n (n <= 2^31 - 1)

struct Log {  // kernel argument: the write log
    const uint8_t* s;
    uint64_t len;
    const uint64_t* off;
    // source word = arrival index
    __device__ const uint8_t* record_at(uint64_t a) const { return s + off[a]; }
};

// Dense arrays over the log's records, by arrival index (record_dev.hpp DenseEntry).
struct Dense {
    uint64_t* pfx;   // first 8 key bytes, big-endian, zero-padded
    uint64_t* klen;  // KeySize
    uint64_t* size;  // TotalSize
};

__global__ __launch_bounds__(kBlock) void k_sort_validate(Log G, uint32_t n, Dense D, unsigned int* err) {
    const uint64_t gg = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (gg >= n) return;
    const uint32_t i = uint32_t(gg);
    DenseEntry e;
    bool bad;
    if (dense_entry(G.s, G.len, G.off, i, n, &e, &bad)) {
        D.pfx[i] = e.pfx;
        D.klen[i] = e.klen;
        D.size[i] = e.size;
    }
    if (bad) atomicOr(err, 1u);
}

// The rest of the key of the validated record at arrival index a, for
// cmp_prefixed: its length from the dense array, its tail in the log.
struct Rest {
    const Log& G;
    const Dense& D;
    uint32_t a;
    __device__ uint64_t len() const { return D.klen[a]; }
    __device__ const uint8_t* tail() const { return G.s + G.off[a] + kHdr + 8; }
};

// Keys of the validated records at arrival indices a and b, whose prefixes are
// pa and pb.  The log is read only when both keys are longer than 8 bytes and
// share their first 8.
__device__ inline int cmp_key(const Log& G, const Dense& D, uint64_t pa, uint32_t a, uint64_t pb, uint32_t b) {
    return cmp_prefixed(pa, Rest{G, D, a}, pb, Rest{G, D, b});
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
    scatter_slots(G, n, flag, idx, osize, ooff, osrc, out_off, out_src, src_addr, totals);
}

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
    Dense D;
    Slots S;
    uint64_t* pfx[2];
    uint32_t* arr[2];
    const auto carve = [&](Carver k) {
        D = Dense{k.take<uint64_t>(n), k.take<uint64_t>(n), k.take<uint64_t>(n)};
        S = take_slots(k, n);
        for (auto& p : pfx) p = k.take<uint64_t>(n);
        for (auto& p : arr) p = k.take<uint32_t>(n2);
        return k.bytes();
    };
    TRY(grow(c->d_stmp, carve(Carver())));
    carve(Carver(c->d_stmp.p));
    size_t tb = 0;
    HIPTRY(scan_exclusive_u64(S.flag, S.idx, n, nullptr, &tb, c->stream));
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
    TRY(read_verdict(c, err));

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
                       S.flag, S.osize, S.osrc);
    HIPTRY(hipGetLastError());
    return write_table(c, k_sort_scatter, G, n, S, c->d_tmp.p, tb, tiles, d_out, d_out_off, d_out_src, totals, n_out,
                       out_len);
} NKV_CATCH

int nkv_sort_records(nkv_ctx* c, const uint8_t* log, uint64_t log_len, const uint64_t* rec_size, uint64_t n,
                     uint8_t* out, uint64_t out_cap, uint64_t* out_rec_size, uint64_t* n_out, uint64_t* out_len) try {
    TRY(bind(c));
    if (!n_out || !out_len || n > kMaxN || (n && (!log || !rec_size))) return NKV_ERR_INVALID;
    if (!records_fill(rec_size, n, log_len) || log_len > (uint64_t(1) << 62) || out_cap < log_len)
        return NKV_ERR_INVALID;
    *n_out = 0;
    *out_len = 0;
    if (n == 0) return NKV_OK;
    if (!out || !out_rec_size) return NKV_ERR_INVALID;
    TRY(grow(c->d_data, (log_len + 15) & ~uint64_t(15)));
    TRY(grow(c->d_len, 8 * n));
    TRY(grow(c->d_off, 8 * n));
    DevBuf& table = c->d_nodes;  // the flushed Data table
    TRY(grow(table, log_len));
    TRY(grow(c->d_rec_off, 8 * n));
    uint64_t* d_size = static_cast<uint64_t*>(c->d_len.p);
    uint64_t* d_off = static_cast<uint64_t*>(c->d_off.p);
    uint64_t* d_out_off = static_cast<uint64_t*>(c->d_rec_off.p);
    TRY(upload_records(c, log, log_len, rec_size, n, c->d_data.p, d_size, d_off));
    TRY(nkv_sort_records_dev(c, c->d_data.p, log_len, d_off, n, table.p, log_len, d_out_off, nullptr, n_out,
                             out_len));
    if (*n_out == 0) return NKV_OK;
    return download_table(c, table.p, *out_len, d_out_off, *n_out, out, out_rec_size);
} NKV_CATCH

}  // extern "C"
