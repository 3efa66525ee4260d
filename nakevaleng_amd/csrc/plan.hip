// plan.hip -- what decides and prepares a leaf pass on gfx950 (the leaf kernels
// themselves are leaf.hip).
//
//   K0  k_locate      value offset/length of each serialized core/record
//                     (record.go:191-199): value = rec + 30 + KeySize.
//       k_len_range   min / max full-block count of a batch (the Gate's range).
//       k_len_*_alloc the length sort and the work queue's header.
//       k_scan_*      in-place exclusive scan of u32; the u64 one is hipcub's.
//       k_fill        splitmix64 synthetic bytes (bench/test input only).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdint.h>

#include "bytes_dev.hpp"
#include "internal.hpp"
#include "sha1_feed_dev.hpp"

namespace nkv {

// ---------------------------------------------------------------------------
// Block fold: leaves the workgroup's min / max / or / sum in thread 0.  Grid
// results go through per-workgroup partials and a fold launch (k_locate_fold)
// or, in the records entries, the pass flags (leaf.hip).
__device__ __forceinline__ void block_fold(uint32_t& lo, uint32_t& hi, uint32_t& flag, unsigned long long& sum) {
    __shared__ uint32_t s_lo[kBlock / 64], s_hi[kBlock / 64], s_fl[kBlock / 64];
    __shared__ unsigned long long s_sum[kBlock / 64];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = min(lo, uint32_t(__shfl_xor(int(lo), o)));
        hi = max(hi, uint32_t(__shfl_xor(int(hi), o)));
        flag |= uint32_t(__shfl_xor(int(flag), o));
        sum += __shfl_xor(sum, o);
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        s_lo[w] = lo;
        s_hi[w] = hi;
        s_fl[w] = flag;
        s_sum[w] = sum;
    }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int k = 1; k < kBlock / 64; ++k) {
            lo = min(lo, s_lo[k]);
            hi = max(hi, s_hi[k]);
            flag |= s_fl[k];
            sum += s_sum[k];
        }
}

constexpr uint32_t kLenBuckets = 640;  // counting-sort buckets (len_bucket_desc)
constexpr int kSortItems = 16;         // values per thread of a sort tile
constexpr uint64_t kSortTile = uint64_t(kBlock) * kSortItems;

// ---------------------------------------------------------------------------
// Length bucketing for ragged values: one lane per value means a wavefront
// runs for its longest value, so values are ordered by compression count,
// longest first (longest-processing-time order for the dispatcher), and the
// leaf kernel reads them through the permutation.  A counting sort over 640
// buckets (exact below 256 compressions, 16 buckets per octave above, so a
// bucket spans at most 1/16 of its length) in two gated kernels (below).
// Order inside a bucket is arbitrary (digests are written by leaf index, so
// results do not depend on it).
__device__ __forceinline__ uint32_t len_bucket_desc(uint64_t len) {
    const uint64_t c64 = compressions(len);
    const uint32_t c = c64 > 0xFFFFFFFFull ? 0xFFFFFFFFu : uint32_t(c64);
    uint32_t k = c;
    if (c >= 256) {
        const uint32_t e = 31u - uint32_t(__clz(c));
        k = 256u + (e - 8u) * 16u + ((c >> (e - 4u)) & 15u);
    }
    return kLenBuckets - 1u - k;
}

// Smallest compression count of a bucket (exact below 256 compressions).
__device__ __forceinline__ uint64_t bucket_compressions(uint32_t bucket) {
    const uint32_t k = kLenBuckets - 1u - bucket;
    if (k < 256u) return k;
    const uint32_t e = 8u + (k - 256u) / 16u;
    return uint64_t(16u + (k - 256u) % 16u) << (e - 4u);
}

// The work queue's header from the sorted order's bucket starts (start[b] =
// first sorted position of bucket b, total = values sorted), by one workgroup,
// so no separate launch sets the queue up: tickets 0; q[2] = the first group
// (64 sorted values, longest first) whose first value is short, i.e. has at
// most split + 1 compressions (0xFFFFFFFF if none); q[4..5] = the batch's work,
// the sum over groups of their first value's compressions (each bucket's
// smallest count: exact below 256 compressions, within 1/16 above -- it only
// feeds k_leaf_queue's throughput-bound test).
__device__ void queue_header(const uint32_t* start, uint32_t total, const QueueInit& qi) {
    uint32_t first = 0xFFFFFFFFu, none_hi = 0u, none_fl = 0u;
    unsigned long long work = 0;
    for (uint32_t b = threadIdx.x; b < kLenBuckets; b += kBlock) {
        const uint64_t s0 = start[b], s1 = b + 1u < kLenBuckets ? start[b + 1] : total;
        const uint64_t comp = bucket_compressions(b);
        work += (((s1 + 63) >> 6) - ((s0 + 63) >> 6)) * comp;  // groups whose first value is in the bucket
        if (s1 > s0 && comp <= uint64_t(qi.split) + 1u) first = min(first, uint32_t(s0));
    }
    block_fold(first, none_hi, none_fl, work);
    if (threadIdx.x == 0) {
        uint32_t* q = qi.q;
        q[0] = 0u;
        q[1] = 0u;
        q[2] = first == 0xFFFFFFFFu ? first : uint32_t((uint64_t(first) + 63) >> 6);
        q[3] = 0u;
        reinterpret_cast<unsigned long long*>(q)[2] = work;
        q[6] = 0u;
        q[7] = 0u;
    }
}

// Two-launch form: k_len_hist_alloc reserves each (bucket, tile) run inside
// its bucket with one device atomic per nonzero bucket (bucket totals at the
// head of the scratch), and k_len_scatter_alloc scans the 640 totals itself,
// so the three column-scan launches go away.  Runs of one bucket land in the
// order the tiles' atomics arrive (order inside a bucket is free).  The last
// workgroup of the scatter (a ticket after every workgroup has read the
// totals) restores the totals to zero for the next sort.
constexpr uint32_t kSortHead = 1024;  // [0, 640) bucket totals, [640] ticket
__global__ __launch_bounds__(kBlock) void k_len_hist_alloc(const uint64_t* __restrict__ len, uint64_t n,
                                                            uint32_t* __restrict__ scratch, uint32_t tiles,
                                                            Gate gate, QueueInit qi, CopyWords cw) {
    __shared__ uint32_t h[kLenBuckets];
    if (blockIdx.x == 0 && threadIdx.x < cw.n) cw.dst[threadIdx.x] = cw.src[threadIdx.x];
    if (!gate.open()) return;
    for (uint32_t i = threadIdx.x; i < kLenBuckets; i += kBlock) h[i] = 0u;
    if (qi.q)  // the work queue's per-SIMD arrivals and claim flags (its header: k_len_scatter_alloc)
        for (uint64_t i = kQueueHeader + uint64_t(blockIdx.x) * kBlock + threadIdx.x; i < qi.nq;
             i += uint64_t(tiles) * kBlock)
            qi.q[i] = 0u;
    __syncthreads();
    const uint64_t base = uint64_t(blockIdx.x) * kSortTile;
    uint32_t bk[kSortItems];
#pragma unroll
    for (int j = 0; j < kSortItems; ++j) {
        const uint64_t i = base + uint64_t(j) * kBlock + threadIdx.x;
        bk[j] = i < n ? len_bucket_desc(len[i]) : kLenBuckets;
    }
#pragma unroll
    for (int j = 0; j < kSortItems; ++j)
        if (bk[j] < kLenBuckets) atomicAdd(&h[bk[j]], 1u);
    __syncthreads();
    uint32_t* hist = scratch + kSortHead;
    for (uint32_t i = threadIdx.x; i < kLenBuckets; i += kBlock) {
        const uint32_t c = h[i];
        hist[uint64_t(i) * tiles + blockIdx.x] = c ? atomicAdd(scratch + i, c) : 0u;
    }
}

__global__ __launch_bounds__(kBlock) void k_len_scatter_alloc(const uint64_t* __restrict__ len, uint64_t n,
                                                               uint32_t* __restrict__ scratch, uint32_t tiles,
                                                               uint32_t* __restrict__ perm, Gate gate,
                                                               QueueInit qi) {
    __shared__ uint32_t cur[kLenBuckets];
    __shared__ uint32_t last, total;
    if (!gate.open()) return;
    if (threadIdx.x < 64) {  // exclusive scan of the bucket totals, 64 at a time
        const int lane = threadIdx.x;
        uint32_t carry = 0u;
        for (uint32_t c0 = 0; c0 < kLenBuckets; c0 += 64) {
            const uint32_t v = scratch[c0 + lane];
            uint32_t x = v;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t y = uint32_t(__shfl_up(int(x), o));
                if (lane >= o) x += y;
            }
            cur[c0 + lane] = carry + x - v;
            carry += uint32_t(__shfl(int(x), 63));
        }
        if (lane == 0) total = carry;
    }
    __syncthreads();
    if (qi.q && blockIdx.x == 0) queue_header(cur, total, qi);
    const uint32_t* hist = scratch + kSortHead;
    for (uint32_t i = threadIdx.x; i < kLenBuckets; i += kBlock) cur[i] += hist[uint64_t(i) * tiles + blockIdx.x];
    __syncthreads();  // every read of the totals is done
    if (threadIdx.x == 0) {
        __threadfence();
        last = atomicAdd(scratch + kLenBuckets, 1u) == tiles - 1u ? 1u : 0u;
    }
    __syncthreads();
    if (last) {  // every workgroup has read the totals: restore them for the next sort
        for (uint32_t i = threadIdx.x; i < kLenBuckets; i += kBlock) scratch[i] = 0u;
        if (threadIdx.x == 0) scratch[kLenBuckets] = 0u;
    }
    const uint64_t base = uint64_t(blockIdx.x) * kSortTile;
    uint32_t bk[kSortItems];
#pragma unroll
    for (int j = 0; j < kSortItems; ++j) {
        const uint64_t i = base + uint64_t(j) * kBlock + threadIdx.x;
        bk[j] = i < n ? len_bucket_desc(len[i]) : kLenBuckets;
    }
#pragma unroll
    for (int j = 0; j < kSortItems; ++j)
        if (bk[j] < kLenBuckets)
            perm[atomicAdd(&cur[bk[j]], 1u)] = uint32_t(base + uint64_t(j) * kBlock + threadIdx.x);
}

// ---------------------------------------------------------------------------
// K0: locate values inside a serialized Data-table stream.
// Record layout (record.go:191-199, little endian): Crc u32 @0, Timestamp i64
// @4, Status u8 @12, TypeInfo u8 @13, KeySize u64 @14, ValueSize u64 @22,
// Key @30, Value @30+KeySize.  rec_off[i] = start of record i.

// One record per thread; each workgroup leaves its range and error flag in
// part[3 b .. 3 b + 2] (plain stores: no same-address atomics across 4096
// blocks), and k_locate_fold combines them in a one-workgroup launch.
__global__ __launch_bounds__(kBlock) void k_locate(const uint8_t* __restrict__ stream,
                                                    uint64_t stream_len,
                                                    const uint64_t* __restrict__ rec_off, uint64_t n,
                                                    uint64_t* __restrict__ voff,
                                                    uint64_t* __restrict__ vlen, uint32_t* __restrict__ part) {
    const uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    uint32_t lo = 0xFFFFFFFFu, hi = 0u, bad = 0u;
    unsigned long long none = 0;
    if (i < n) {
        const uint64_t r = rec_off[i];
        uint64_t o = 0, l = 0;
        if (header_in(r, stream_len)) {
            uint64_t ks, vs;
            ld_header_sizes(stream + r, ks, vs);
            o = r + 30 + ks;
            l = vs;
            if (ks > stream_len || vs > stream_len || o + l > stream_len) {
                bad = 1u;
                o = 0;
                l = 0;
            }
        } else {
            bad = 1u;
        }
        voff[i] = o;
        vlen[i] = l;
        const uint64_t b = l >> 6;
        lo = hi = b > 0xFFFFFFFFull ? 0xFFFFFFFFu : uint32_t(b);
    }
    block_fold(lo, hi, bad, none);
    if (threadIdx.x == 0) {
        part[3 * blockIdx.x] = lo;
        part[3 * blockIdx.x + 1] = hi;
        part[3 * blockIdx.x + 2] = bad;
    }
}

__global__ __launch_bounds__(kBlock) void k_locate_fold(const uint32_t* __restrict__ part, uint32_t nb,
                                                         unsigned int* __restrict__ err,
                                                         unsigned int* __restrict__ range) {
    uint32_t lo = 0xFFFFFFFFu, hi = 0u, bad = 0u;
    unsigned long long none = 0;
    // coalesced, independent loads over the flat triples (one per workgroup)
    const uint32_t words = 3u * nb;
#pragma unroll 8
    for (uint32_t x = threadIdx.x; x < words; x += kBlock) {
        const uint32_t v = part[x];
        const uint32_t kind = x % 3u;
        if (kind == 0u) lo = min(lo, v);
        else if (kind == 1u) hi = max(hi, v);
        else bad |= v;
    }
    block_fold(lo, hi, bad, none);
    if (threadIdx.x == 0) {
        if (err) *err = bad;
        if (range) {
            range[0] = lo;
            range[1] = hi;
        }
    }
}

// Range of full-block counts of a batch: out[0] = min, out[1] = max.  Lets
// the leaf level choose input order (narrow range: no sort) or the
// length-sorted work queue, on the device (Gate).
__global__ __launch_bounds__(kBlock) void k_len_range(const uint64_t* __restrict__ len, uint64_t n,
                                                       uint32_t* __restrict__ part, unsigned int* __restrict__ out,
                                                       unsigned int* __restrict__ ticket) {
    // eight values per thread, loads first; one (lo, hi, 0) partial per
    // workgroup, and the last workgroup to finish (a ticket) folds them into
    // out (no same-address min/max atomics: a grid fold over 256 workgroups
    // serialised them for 12.6 us at 453 K values; and no fold launch)
    uint32_t lo = 0xFFFFFFFFu, hi = 0u, none = 0u;
    unsigned long long zero = 0;
    const uint64_t base = uint64_t(blockIdx.x) * (kBlock * 8) + threadIdx.x;
    uint64_t v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        const uint64_t i = base + uint64_t(u) * kBlock;
        v[u] = i < n ? len[i] : 0u;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        if (base + uint64_t(u) * kBlock >= n) continue;
        const uint64_t b = v[u] >> 6;
        const uint32_t bb = b > 0xFFFFFFFFull ? 0xFFFFFFFFu : uint32_t(b);
        lo = min(lo, bb);
        hi = max(hi, bb);
    }
    block_fold(lo, hi, none, zero);
    __shared__ uint32_t is_last;
    if (threadIdx.x == 0) {
        part[3 * blockIdx.x] = lo;
        part[3 * blockIdx.x + 1] = hi;
        part[3 * blockIdx.x + 2] = 0u;
        __threadfence();
        is_last = atomicAdd(ticket, 1u) == gridDim.x - 1 ? 1u : 0u;
    }
    __syncthreads();
    if (!is_last) return;
    __threadfence();
    lo = 0xFFFFFFFFu;
    hi = 0u;
    for (uint32_t b = threadIdx.x; b < gridDim.x; b += kBlock) {
        lo = min(lo, __atomic_load_n(part + 3 * b, __ATOMIC_RELAXED));
        hi = max(hi, __atomic_load_n(part + 3 * b + 1, __ATOMIC_RELAXED));
    }
    block_fold(lo, hi, none, zero);
    if (threadIdx.x == 0) {
        out[0] = lo;
        out[1] = hi;
        atomicExch(ticket, 0u);  // the next launch counts from 0
    }
}

hipError_t launch_len_range(const uint64_t* len, uint64_t n, unsigned int* out, uint32_t* part, unsigned int* ticket,
                            hipStream_t s) {
    const unsigned nb = unsigned((n + kBlock * 8 - 1) / (kBlock * 8));
    hipLaunchKernelGGL(k_len_range, dim3(nb), dim3(kBlock), 0, s, len, n, part, out, ticket);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------
// synthetic input: byte j = byte (j % 8) of splitmix64(seed, j / 8), LE.
__device__ __forceinline__ uint64_t splitmix64_at(uint64_t seed, uint64_t k) {
    uint64_t z = seed + (k + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__global__ __launch_bounds__(kBlock) void k_fill(uint8_t* __restrict__ buf, uint64_t nbytes,
                                                  uint64_t seed) {
    const uint64_t stride = uint64_t(gridDim.x) * kBlock;
    // a byte string, at any address (nkv_merkle.h, device outputs): 16-byte
    // stores only into a 16-byte aligned buffer.  (Established by reading: the
    // hardware also accepts misaligned 16-byte stores, so the placement tests
    // pin the bytes and the extent, not this check.)
    const bool al = (reinterpret_cast<uintptr_t>(buf) & 15u) == 0;
    for (uint64_t t = uint64_t(blockIdx.x) * kBlock + threadIdx.x; 16 * t < nbytes; t += stride) {
        const uint64_t a = splitmix64_at(seed, 2 * t), b = splitmix64_at(seed, 2 * t + 1);
        if (al && 16 * t + 16 <= nbytes) {
            *reinterpret_cast<uint4*>(buf + 16 * t) =
                make_uint4(uint32_t(a), uint32_t(a >> 32), uint32_t(b), uint32_t(b >> 32));
        } else {
            const uint64_t j1 = min(16 * t + 16, nbytes);
            for (uint64_t j = 16 * t; j < j1; ++j) {
                const uint64_t v = (j - 16 * t) < 8 ? a : b;
                buf[j] = uint8_t(v >> (8 * (j & 7)));
            }
        }
    }
}

// ---------------------------------------------------------------------------
// host-side launchers

uint64_t queue_words(uint64_t n) { return kQueueHeader + kSimdKeys + (n + 63) / 64; }

// one (lo, hi, flag) triple per workgroup (k_locate, k_leaf_records)
uint64_t locate_part_words(uint64_t n) { return 3 * uint64_t(blocks_for(n)); }

void launch_locate_fold(const uint32_t* part, uint32_t nb, unsigned int* err, unsigned int* range, hipStream_t s) {
    hipLaunchKernelGGL(k_locate_fold, dim3(1), dim3(kBlock), 0, s, part, nb, err, range);
}

hipError_t launch_locate(const uint8_t* stream, uint64_t stream_len, const uint64_t* rec_off,
                         uint64_t n, uint64_t* voff, uint64_t* vlen, unsigned int* err, unsigned int* range,
                         uint32_t* part, hipStream_t s) {
    const unsigned nb = blocks_for(n);
    hipLaunchKernelGGL(k_locate, dim3(nb), dim3(kBlock), 0, s, stream, stream_len, rec_off, n, voff, vlen, part);
    launch_locate_fold(part, nb, err, range, s);
    return hipGetLastError();
}

hipError_t scan_exclusive_u64(const uint64_t* in, uint64_t* out, uint64_t n, void* tmp,
                              size_t* tmp_bytes, hipStream_t s) {
    return hipcub::DeviceScan::ExclusiveSum(tmp, *tmp_bytes, in, out, int(n), s);
}

// ---------------------------------------------------------------------------
// In-place exclusive scan of u32 (gated): per-tile sums, one block scans the
// sums, each tile scans itself plus its offset.  a holds n + 1 words when the
// total is wanted (a zero appended).
constexpr int kScanItems = 8;
constexpr uint64_t kScanTile = uint64_t(kBlock) * kScanItems;

// exclusive scan of v over the workgroup (thread order); returns the total
__device__ __forceinline__ uint32_t block_exclusive(uint32_t& v) {
    __shared__ uint32_t wsum[kBlock / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = uint32_t(__shfl_up(int(x), o));
        if (lane >= o) x += y;
    }
    if (lane == 63) wsum[wave] = x;
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) {
        if (w < wave) before += wsum[w];
        total += wsum[w];
    }
    __syncthreads();
    v = before + x - v;
    return total;
}

__global__ __launch_bounds__(kBlock) void k_scan_sums(const uint32_t* __restrict__ a, uint64_t n,
                                                       uint32_t* __restrict__ sums, Gate gate) {
    if (!gate.open()) return;
    const uint64_t base = uint64_t(blockIdx.x) * kScanTile + uint64_t(threadIdx.x) * kScanItems;
    uint32_t s = 0;
#pragma unroll
    for (int j = 0; j < kScanItems; ++j)
        if (base + j < n) s += a[base + j];
    uint32_t v = s;
    const uint32_t tot = block_exclusive(v);
    if (threadIdx.x == 0) sums[blockIdx.x] = tot;
}

__global__ __launch_bounds__(kBlock) void k_scan_top(uint32_t* __restrict__ sums, uint32_t nt, Gate gate) {
    if (!gate.open()) return;
    uint32_t carry = 0;
    for (uint32_t b = 0; b < nt; b += kBlock) {  // one workgroup, kBlock sums per round
        uint32_t v = b + threadIdx.x < nt ? sums[b + threadIdx.x] : 0u;
        const uint32_t tot = block_exclusive(v);
        if (b + threadIdx.x < nt) sums[b + threadIdx.x] = carry + v;
        carry += tot;
    }
}

__global__ __launch_bounds__(kBlock) void k_scan_down(uint32_t* __restrict__ a, uint64_t n,
                                                       const uint32_t* __restrict__ sums, Gate gate) {
    if (!gate.open()) return;
    const uint64_t base = uint64_t(blockIdx.x) * kScanTile + uint64_t(threadIdx.x) * kScanItems;
    uint32_t x[kScanItems];
    uint32_t s = 0;
#pragma unroll
    for (int j = 0; j < kScanItems; ++j) {
        x[j] = base + j < n ? a[base + j] : 0u;
        s += x[j];
    }
    uint32_t v = s;
    (void)block_exclusive(v);
    uint32_t run = sums[blockIdx.x] + v;
#pragma unroll
    for (int j = 0; j < kScanItems; ++j) {
        if (base + j < n) a[base + j] = run;
        run += x[j];
    }
}

uint64_t scan_sums_words(uint64_t n) { return (n + kScanTile - 1) / kScanTile; }

hipError_t scan_exclusive_u32(uint32_t* a, uint64_t n, uint32_t* sums, hipStream_t s, Gate gate) {
    const uint64_t nt = scan_sums_words(n);
    if (nt == 0) return hipSuccess;
    if (nt > 0xFFFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_scan_sums, dim3(uint32_t(nt)), dim3(kBlock), 0, s, a, n, sums, gate);
    hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(kBlock), 0, s, sums, uint32_t(nt), gate);
    hipLaunchKernelGGL(k_scan_down, dim3(uint32_t(nt)), dim3(kBlock), 0, s, a, n, sums, gate);
    return hipGetLastError();
}

uint64_t sort_hist_words(uint64_t n) { return kSortHead + ((n + kSortTile - 1) / kSortTile) * kLenBuckets; }
uint64_t sort_head_words() { return kSortHead; }

// scratch: sort_hist_words(n) u32 whose first sort_head_words() are zero
// (the two-launch form keeps them zero between calls)
hipError_t sort_by_length_desc(const uint64_t* len, uint64_t n, uint32_t* perm, uint32_t* scratch, hipStream_t s,
                               Gate gate, QueueInit qi, CopyWords cw) {
    const uint64_t tiles = (n + kSortTile - 1) / kSortTile;
    if (tiles == 0) return hipSuccess;
    hipLaunchKernelGGL(k_len_hist_alloc, dim3(uint32_t(tiles)), dim3(kBlock), 0, s, len, n, scratch,
                       uint32_t(tiles), gate, qi, cw);
    hipLaunchKernelGGL(k_len_scatter_alloc, dim3(uint32_t(tiles)), dim3(kBlock), 0, s, len, n, scratch,
                       uint32_t(tiles), perm, gate, qi);
    return hipGetLastError();
}

hipError_t launch_fill(uint8_t* buf, uint64_t nbytes, uint64_t seed, hipStream_t s) {
    uint64_t threads = (nbytes + 15) / 16;
    uint64_t blocks = (threads + kBlock - 1) / kBlock;
    if (blocks > 65536) blocks = 65536;
    if (blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(k_fill, dim3(unsigned(blocks)), dim3(kBlock), 0, s, buf, nbytes, seed);
    return hipGetLastError();
}

}  // namespace nkv
