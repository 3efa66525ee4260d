// merge.hip -- compaction's k-way merge of sorted Data-table runs on the device
// (core/lsmtree/lsmtree.go:137-231): nkv_merge_records_dev / nkv_merge_records.
//
// Stages, all on the context's stream:
//   k_merge_validate  one lane per input record: its dense entry (record_dev.hpp
//                     dense_entry: the record's span, it ends where the next
//                     starts; the key's prefix, KeySize, TotalSize), the
//                     timestamp, and key > predecessor's key.  The host reads
//                     its error word before anything else is launched.
//   k_merge_rank      one lane per input record: a lower bound in every other
//                     run gives rank = records with a smaller key; a record that
//                     meets its key in another run survives only as the winner
//                     (nkv_merkle.h: the tie rule).  Survivors write flag, size
//                     and source at slot `rank`.
//   scans             exclusive sums of the flags (output index) and the sizes
//                     (output offset), then k_merge_scatter compacts them into
//                     d_out_off / d_out_src / source addresses.
//   k_merge_copy      tiles the OUTPUT bytes: a workgroup owns 16 KiB of d_out,
//                     keeps the records overlapping it in LDS, and every lane
//                     writes 16 destination-aligned bytes per step, funnel-
//                     shifted out of aligned 16-byte source loads.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "context.hpp"
#include "merge_copy_dev.hpp"  // Slots, scatter_slots, write_table, kCopyTile

using namespace nkv;

namespace {

struct Runs {  // kernel argument: the k input runs
    const uint8_t* stream[NKV_MERGE_MAX_RUNS];
    uint64_t len[NKV_MERGE_MAX_RUNS];
    const uint64_t* off[NKV_MERGE_MAX_RUNS];
    uint32_t base[NKV_MERGE_MAX_RUNS + 1];  // records before run r (base[k] = all records)
    int k;
    // source word = (run << 32) | index in the run
    __device__ const uint8_t* record_at(uint64_t w) const { return stream[w >> 32] + off[w >> 32][uint32_t(w)]; }
};

__device__ __forceinline__ int run_of(const Runs& R, uint32_t g) {
    int r = 0;
    while (r + 1 < R.k && g >= R.base[r + 1]) ++r;
    return r;
}

// Dense arrays over all input records (index = base[run] + index in the run).
struct Dense {
    uint64_t* pfx;   // first 8 key bytes, big-endian, zero-padded
    uint64_t* klen;  // KeySize
    int64_t* ts;     // Timestamp
    uint64_t* size;  // TotalSize
};

__global__ __launch_bounds__(kBlock) void k_merge_validate(Runs R, uint32_t N, Dense D, unsigned int* err) {
    const uint64_t gg = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (gg >= N) return;
    const uint32_t g = uint32_t(gg);
    const int r = run_of(R, g);
    const uint32_t i = g - R.base[r], n = R.base[r + 1] - R.base[r];
    const uint8_t* s = R.stream[r];
    const uint64_t L = R.len[r];
    const uint64_t* off = R.off[r];
    DenseEntry e;
    bool bad;
    if (dense_entry(s, L, off, i, n, &e, &bad)) {
        const uint64_t o = off[i];
        D.pfx[g] = e.pfx;
        D.klen[g] = e.klen;
        D.ts[g] = int64_t(ld_le64(s + o + kAtTimestamp));
        D.size[g] = e.size;
        if (i > 0) {  // strictly increasing keys; a predecessor out of bounds is its own lane's error
            const uint64_t po = off[i - 1];
            uint64_t pks;
            if (key_span_in(s, L, po, &pks) && cmp_bytes(s + po + kHdr, pks, s + o + kHdr, e.klen) >= 0) bad = true;
        }
    }
    if (bad) atomicOr(err, 1u);
}

// The rest of the key of validated record i of run r, for cmp_prefixed: its
// length from the dense array (or at hand), its tail in the stream.
struct Rest {
    const Runs& R;
    const uint64_t* klen;  // at the record's dense index
    int r;
    uint32_t i;
    __device__ uint64_t len() const { return *klen; }
    __device__ const uint8_t* tail() const { return R.stream[r] + R.off[r][i] + kHdr + 8; }
};

// Keys of two validated records by their dense entries; the streams are read
// only when both keys are longer than 8 bytes and share their first 8.
__device__ inline int cmp_key(const Runs& R, const Dense& D, uint64_t pa, uint64_t la, int ra, uint32_t ia, int rb,
                              uint32_t ib) {
    const uint32_t gb = R.base[rb] + ib;
    return cmp_prefixed(pa, Rest{R, &la, ra, ia}, D.pfx[gb], Rest{R, D.klen + gb, rb, ib});
}

__global__ __launch_bounds__(kBlock) void k_merge_rank(Runs R, uint32_t N, Dense D, uint64_t* __restrict__ flag,
                                                       uint64_t* __restrict__ osize, uint64_t* __restrict__ osrc) {
    const uint64_t gg = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (gg >= N) return;
    const uint32_t g = uint32_t(gg);
    const int r = run_of(R, g);
    const uint32_t i = g - R.base[r];
    const uint64_t p = D.pfx[g], l = D.klen[g];
    const int64_t t = D.ts[g];
    uint64_t rank = i;
    bool lost = false;
    for (int q = 0; q < R.k; ++q) {
        if (q == r) continue;
        const uint32_t nq = R.base[q + 1] - R.base[q];
        uint32_t lo = 0, hi = nq;  // lower bound: records of run q with a smaller key
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (cmp_key(R, D, p, l, r, i, q, mid) > 0) lo = mid + 1;
            else hi = mid;
        }
        rank += lo;
        if (lost || lo == nq || cmp_key(R, D, p, l, r, i, q, lo) != 0) continue;
        // the same key in run q: greatest Timestamp (signed), then the smaller
        // predecessor key ("none" smallest), then the lower run
        const int64_t tq = D.ts[R.base[q] + lo];
        if (tq != t) {
            lost = tq > t;
            continue;
        }
        int c;
        if (i == 0 || lo == 0) {
            c = (i == 0 ? 0 : 1) - (lo == 0 ? 0 : 1);
        } else {
            const uint32_t gp = g - 1;
            c = cmp_key(R, D, D.pfx[gp], D.klen[gp], r, i - 1, q, lo - 1);
        }
        lost = c > 0 || (c == 0 && q < r);
    }
    if (!lost) {  // survivors have distinct ranks
        flag[rank] = 1;
        osize[rank] = D.size[g];
        osrc[rank] = (uint64_t(r) << 32) | i;
    }
}

__global__ __launch_bounds__(kBlock) void k_merge_scatter(Runs R, uint32_t N, const uint64_t* __restrict__ flag,
                                                          const uint64_t* __restrict__ idx,
                                                          const uint64_t* __restrict__ osize,
                                                          const uint64_t* __restrict__ ooff,
                                                          const uint64_t* __restrict__ osrc,
                                                          uint64_t* __restrict__ out_off, uint64_t* __restrict__ out_src,
                                                          uint64_t* __restrict__ src_addr, uint64_t* __restrict__ totals) {
    scatter_slots(R, N, flag, idx, osize, ooff, osrc, out_off, out_src, src_addr, totals);
}

}  // namespace

extern "C" {

int nkv_merge_records_dev(nkv_ctx* c, const nkv_run* runs, int k, void* d_out, uint64_t out_cap,
                          uint64_t* d_out_off, uint64_t* d_out_src, uint64_t* n_out, uint64_t* out_len) try {
    TRY(bind(c));
    if (!runs || k < 1 || k > NKV_MERGE_MAX_RUNS || !n_out || !out_len) return NKV_ERR_INVALID;
    Runs R{};
    R.k = k;
    uint64_t N = 0, total = 0;
    for (int r = 0; r < k; ++r) {
        const nkv_run& u = runs[r];
        if (u.n > kMaxN || N + u.n > kMaxN) return NKV_ERR_INVALID;
        if (u.n ? (!u.stream || !u.rec_off || u.stream_len / kHdr < u.n) : u.stream_len != 0) return NKV_ERR_INVALID;
        if (u.stream_len > UINT64_MAX - total) return NKV_ERR_INVALID;
        R.stream[r] = static_cast<const uint8_t*>(u.stream);
        R.len[r] = u.stream_len;
        R.off[r] = u.rec_off;
        R.base[r] = uint32_t(N);
        N += u.n;
        total += u.stream_len;
    }
    for (int r = k; r <= NKV_MERGE_MAX_RUNS; ++r) R.base[r] = uint32_t(N);
    const uint64_t tiles = total / kCopyTile + 2;  // the copy's grid: d_out's 16-byte grid over at most `total` bytes
    if (out_cap < total || tiles > 0x7fffffffull) return NKV_ERR_INVALID;
    *n_out = 0;
    *out_len = 0;
    if (N == 0) return NKV_OK;
    if (!d_out || !d_out_off) return NKV_ERR_INVALID;

    // scratch: ten u64 arrays of N, the scan's temporary, and [err | n_out, out_len].
    // The arrays live in d_stmp (free scratch, context.hpp).
    Dense D;
    Slots S;
    const auto carve = [&](Carver k) {
        D = Dense{k.take<uint64_t>(N), k.take<uint64_t>(N), k.take<int64_t>(N), k.take<uint64_t>(N)};
        S = take_slots(k, N);
        return k.bytes();
    };
    TRY(grow(c->d_stmp, carve(Carver())));
    carve(Carver(c->d_stmp.p));
    size_t tb = 0;
    HIPTRY(scan_exclusive_u64(S.flag, S.idx, N, nullptr, &tb, c->stream));
    TRY(grow(c->d_tmp, tb));
    TRY(grow(c->d_stats, 24));
    unsigned int* err = static_cast<unsigned int*>(c->d_stats.p);
    uint64_t* totals = static_cast<uint64_t*>(c->d_stats.p) + 1;
    const uint32_t n32 = uint32_t(N);

    // validation first: nothing that follows a key or copies a record is
    // launched unless every header, offset and key order checked out
    HIPTRY(hipMemsetAsync(err, 0, 24, c->stream));
    hipLaunchKernelGGL(k_merge_validate, dim3(blocks_for(N)), dim3(kBlock), 0, c->stream, R, n32, D, err);
    HIPTRY(hipGetLastError());
    TRY(read_verdict(c, err));

    // with NKV_TIMING_EVENTS: "leaf" = rank + scans + scatter, "reduce" = the copy kernel
    TRY(mark(c, 0));
    HIPTRY(hipMemsetAsync(S.flag, 0, 2 * 8 * N, c->stream));  // flag and osize
    hipLaunchKernelGGL(k_merge_rank, dim3(blocks_for(N)), dim3(kBlock), 0, c->stream, R, n32, D, S.flag, S.osize,
                       S.osrc);
    HIPTRY(hipGetLastError());
    return write_table(c, k_merge_scatter, R, N, S, c->d_tmp.p, tb, tiles, d_out, d_out_off, d_out_src, totals, n_out,
                       out_len);
} NKV_CATCH

int nkv_merge_records(nkv_ctx* c, const uint8_t* const* streams, const uint64_t* stream_len,
                      const uint64_t* const* rec_size, const uint64_t* n, int k, uint8_t* out, uint64_t out_cap,
                      uint64_t* out_rec_size, uint64_t* n_out, uint64_t* out_len) try {
    TRY(bind(c));
    if (!streams || !stream_len || !rec_size || !n || k < 1 || k > NKV_MERGE_MAX_RUNS || !n_out || !out_len)
        return NKV_ERR_INVALID;
    uint64_t N = 0, total = 0, padded = 0;
    uint64_t at[NKV_MERGE_MAX_RUNS];
    for (int r = 0; r < k; ++r) {
        if (n[r] > kMaxN || N + n[r] > kMaxN) return NKV_ERR_INVALID;
        if (n[r] && (!streams[r] || !rec_size[r])) return NKV_ERR_INVALID;
        if (!records_fill(rec_size[r], n[r], stream_len[r]) || stream_len[r] > (uint64_t(1) << 62) - total)
            return NKV_ERR_INVALID;
        at[r] = padded;
        N += n[r];
        total += stream_len[r];
        padded += (stream_len[r] + 15) & ~uint64_t(15);
    }
    if (out_cap < total) return NKV_ERR_INVALID;
    *n_out = 0;
    *out_len = 0;
    if (N == 0) return NKV_OK;
    if (!out || !out_rec_size) return NKV_ERR_INVALID;
    TRY(grow(c->d_data, padded));
    TRY(grow(c->d_len, 8 * N));
    TRY(grow(c->d_off, 8 * N));
    DevBuf& table = c->d_nodes;  // the merged Data table
    TRY(grow(table, total));
    TRY(grow(c->d_rec_off, 8 * N));
    uint8_t* d_in = static_cast<uint8_t*>(c->d_data.p);
    uint64_t* d_size = static_cast<uint64_t*>(c->d_len.p);
    uint64_t* d_off = static_cast<uint64_t*>(c->d_off.p);
    uint64_t* d_out_off = static_cast<uint64_t*>(c->d_rec_off.p);
    nkv_run runs[NKV_MERGE_MAX_RUNS];
    uint64_t base = 0;
    for (int r = 0; r < k; ++r) {
        runs[r] = nkv_run{d_in + at[r], stream_len[r], d_off + base, n[r]};
        if (n[r] == 0) continue;
        TRY(upload_records(c, streams[r], stream_len[r], rec_size[r], n[r], d_in + at[r], d_size + base, d_off + base));
        base += n[r];
    }
    TRY(nkv_merge_records_dev(c, runs, k, table.p, total, d_out_off, nullptr, n_out, out_len));
    if (*n_out == 0) return NKV_OK;
    return download_table(c, table.p, *out_len, d_out_off, *n_out, out, out_rec_size);
} NKV_CATCH

}  // extern "C"
