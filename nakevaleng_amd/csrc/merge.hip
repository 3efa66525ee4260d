// merge.hip -- compaction's k-way merge of sorted Data-table runs on the device
// (core/lsmtree/lsmtree.go:137-231): nkv_merge_records_dev / nkv_merge_records.
//
// Stages, all on the context's stream:
//   k_merge_validate  one lane per input record: header bounds, the record ends
//                     where the next starts, key > predecessor's key; writes the
//                     dense sort keys (first 8 key bytes big-endian, key length),
//                     the timestamp and TotalSize.  The host reads its error
//                     word before anything else is launched.
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

#include <vector>

#include "bytes_dev.hpp"  // ld_le64, cmp_bytes, ld16_any
#include "context.hpp"
#include "merge_copy_dev.hpp"  // k_merge_copy, kCopyTile

using namespace nkv;

namespace {

constexpr int kHdr = 30;  // record.go:191-199: Crc 4 | Timestamp 8 | Status 1 | TypeInfo 1 | KeySize 8 | ValueSize 8

struct Runs {  // kernel argument: the k input runs
    const uint8_t* stream[NKV_MERGE_MAX_RUNS];
    uint64_t len[NKV_MERGE_MAX_RUNS];
    const uint64_t* off[NKV_MERGE_MAX_RUNS];
    uint32_t base[NKV_MERGE_MAX_RUNS + 1];  // records before run r (base[k] = all records)
    int k;
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
    const uint64_t o = off[i];
    bool bad = (i == 0 && o != 0) || !header_in(o, L);
    if (!bad) {
        const uint64_t ks = ld_le64(s + o + 14), vs = ld_le64(s + o + 22);
        const uint64_t room = L - o - kHdr;
        if (ks > room || vs > room - ks) {
            bad = true;
        } else {
            const uint64_t end = o + kHdr + ks + vs;  // <= L: no overflow
            const uint64_t next = i + 1 < n ? off[i + 1] : L;
            if (end != next) bad = true;
            const uint8_t* key = s + o + kHdr;
            uint64_t p = 0;
            for (uint32_t b = 0; b < 8 && b < ks; ++b) p |= uint64_t(key[b]) << (56 - 8 * b);
            D.pfx[g] = p;
            D.klen[g] = ks;
            D.ts[g] = int64_t(ld_le64(s + o + 4));
            D.size[g] = kHdr + ks + vs;
            if (i > 0) {  // strictly increasing keys; a predecessor out of bounds is its own lane's error
                const uint64_t po = off[i - 1];
                if (header_in(po, L)) {
                    const uint64_t pks = ld_le64(s + po + 14);
                    if (pks <= L - po - kHdr && cmp_bytes(s + po + kHdr, pks, key, ks) >= 0) bad = true;
                }
            }
        }
    }
    if (bad) atomicOr(err, 1u);
}

// Keys of two validated records by their dense entries; the streams are read
// only when both keys are longer than 8 bytes and share their first 8.
__device__ inline int cmp_key(const Runs& R, const Dense& D, uint64_t pa, uint64_t la, int ra, uint32_t ia, int rb,
                              uint32_t ib) {
    const uint32_t gb = R.base[rb] + ib;
    const uint64_t pb = D.pfx[gb];
    if (pa != pb) return pa < pb ? -1 : 1;
    const uint64_t lb = D.klen[gb];
    if (la <= 8 || lb <= 8) return la < lb ? -1 : (la > lb ? 1 : 0);
    const uint8_t* ka = R.stream[ra] + R.off[ra][ia] + kHdr;
    const uint8_t* kb = R.stream[rb] + R.off[rb][ib] + kHdr;
    return cmp_bytes(ka + 8, la - 8, kb + 8, lb - 8);
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
    const uint64_t s = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (s >= N) return;
    if (flag[s]) {
        const uint64_t j = idx[s], w = osrc[s];
        const int r = int(w >> 32);
        out_off[j] = ooff[s];
        if (out_src) out_src[j] = w;
        src_addr[j] = uint64_t(reinterpret_cast<uintptr_t>(R.stream[r] + R.off[r][uint32_t(w)]));
    }
    if (s == N - 1) {
        totals[0] = idx[s] + flag[s];
        totals[1] = ooff[s] + osize[s];
    }
}

inline unsigned blocks_for(uint64_t n) { return unsigned((n + kBlock - 1) / kBlock); }

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
    // The arrays live in d_stmp, which carries nothing from call to call (d_keys
    // does: the length sort expects its head words left at zero).
    TRY(grow(c->d_stmp, 10 * 8 * N));
    uint64_t* a = static_cast<uint64_t*>(c->d_stmp.p);
    Dense D{a, a + N, reinterpret_cast<int64_t*>(a + 2 * N), a + 3 * N};
    uint64_t *flag = a + 4 * N, *osize = a + 5 * N, *osrc = a + 6 * N, *idx = a + 7 * N, *ooff = a + 8 * N,
             *src_addr = a + 9 * N;
    size_t tb = 0;
    HIPTRY(scan_exclusive_u64(flag, idx, N, nullptr, &tb, c->stream));
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
    unsigned int h_err = 0;
    HIPTRY(hipMemcpyAsync(&h_err, err, 4, hipMemcpyDeviceToHost, c->stream));
    HIPTRY(hipStreamSynchronize(c->stream));
    if (h_err) return NKV_ERR_INVALID;

    // with NKV_TIMING_EVENTS: "leaf" = rank + scans + scatter, "reduce" = the copy kernel
    TRY(mark(c, 0));
    HIPTRY(hipMemsetAsync(flag, 0, 2 * 8 * N, c->stream));  // flag and osize
    hipLaunchKernelGGL(k_merge_rank, dim3(blocks_for(N)), dim3(kBlock), 0, c->stream, R, n32, D, flag, osize, osrc);
    HIPTRY(hipGetLastError());
    HIPTRY(scan_exclusive_u64(flag, idx, N, c->d_tmp.p, &tb, c->stream));
    HIPTRY(scan_exclusive_u64(osize, ooff, N, c->d_tmp.p, &tb, c->stream));
    hipLaunchKernelGGL(k_merge_scatter, dim3(blocks_for(N)), dim3(kBlock), 0, c->stream, R, n32, flag, idx, osize,
                       ooff, osrc, d_out_off, d_out_src, src_addr, totals);
    HIPTRY(hipGetLastError());
    TRY(mark(c, 1));
    // out_len is known on the device only: the grid covers the bound (the sum
    // of the inputs), and tiles past out_len leave at once
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
        uint64_t left = stream_len[r];  // the sizes add up to the stream exactly, term by term (no wrapped sum)
        for (uint64_t i = 0; i < n[r]; ++i) {
            if (rec_size[r][i] > left) return NKV_ERR_INVALID;
            left -= rec_size[r][i];
        }
        if (left != 0 || stream_len[r] > (uint64_t(1) << 62) - total) return NKV_ERR_INVALID;
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
    TRY(grow(c->d_nodes, total));
    TRY(grow(c->d_tmp2, 8 * N));
    uint8_t* d_in = static_cast<uint8_t*>(c->d_data.p);
    uint64_t* d_size = static_cast<uint64_t*>(c->d_len.p);
    uint64_t* d_off = static_cast<uint64_t*>(c->d_off.p);
    uint64_t* d_out_off = static_cast<uint64_t*>(c->d_tmp2.p);
    nkv_run runs[NKV_MERGE_MAX_RUNS];
    uint64_t base = 0;
    for (int r = 0; r < k; ++r) {
        runs[r] = nkv_run{d_in + at[r], stream_len[r], d_off + base, n[r]};
        if (n[r] == 0) continue;
        HIPTRY(hipMemcpyAsync(d_in + at[r], streams[r], stream_len[r], hipMemcpyHostToDevice, c->stream));
        HIPTRY(hipMemcpyAsync(d_size + base, rec_size[r], 8 * n[r], hipMemcpyHostToDevice, c->stream));
        TRY(nkv_record_offsets_dev(c, d_size + base, n[r], d_off + base));
        base += n[r];
    }
    TRY(nkv_merge_records_dev(c, runs, k, c->d_nodes.p, total, d_out_off, nullptr, n_out, out_len));
    if (*n_out == 0) return NKV_OK;
    std::vector<uint64_t> off(*n_out);
    HIPTRY(hipMemcpyAsync(out, c->d_nodes.p, *out_len, hipMemcpyDeviceToHost, c->stream));
    HIPTRY(hipMemcpyAsync(off.data(), d_out_off, 8 * *n_out, hipMemcpyDeviceToHost, c->stream));
    HIPTRY(hipStreamSynchronize(c->stream));
    for (uint64_t j = 0; j < *n_out; ++j) out_rec_size[j] = (j + 1 < *n_out ? off[j + 1] : *out_len) - off[j];
    return NKV_OK;
} NKV_CATCH

}  // extern "C"
