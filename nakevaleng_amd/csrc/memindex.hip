// memindex.hip -- the live memtable on the device (core/memtable/memtable.go:40-90
// over core/skiplist/skiplist.go:62-120): nkv_memtable_clear_dev / _add_dev /
// _find_dev.  A hash index over the resident write log, the one
// nkv_encode_records_dev leaves and nkv_sort_records_dev (memtable.hip, the
// flush) takes, with the reference's Add / Find / Count / ShouldFlush answers.
//
// The index: `slots` (a power of two) 8-byte entries, open addressing, linear
// probing from murmur3(key) (murmur_dev.hpp, a fixed seed).  An entry holds two
// arrival indices of writes of its key: the first (low word, the minimum) and
// the latest (high word, the maximum); all ones = empty.  A slot's key never
// changes once the slot is claimed, and either word always names a record of
// that key, so a reader that sees an older value of a slot still compares with
// the right key, and one that sees "empty" where the slot is taken learns the
// truth from its compare-and-swap.  Every answer is a min or a max over the
// writes of a key: it does not depend on the order the lanes arrive in.  The
// bytes of the index do (which of two colliding keys got the earlier slot).
//
// Add, all on the context's stream (every kernel behind the first reads the
// error word and leaves when it is set):
//   k_mem_validate  one lane per new record: its dense entry (record_dev.hpp;
//                   the log must be dense, as the flush requires), its size;
//                   lane 0: the state's indexed count is n_done and record
//                   n_done starts where record n_done - 1 ends.
//   k_mem_insert    one lane per new record: probe; an empty slot is claimed by
//                   one 64-bit compare-and-swap from empty to (i, i); in a taken
//                   one the key is compared in place in the log and, if equal,
//                   atomicMin on the first word and atomicMax on the latest (each
//                   skipped when the value read already makes it a no-op: the
//                   words only move one way; and the lanes of a wave that share
//                   a slot send one of each, from their lowest and their highest
//                   lane).  The slot found goes to scratch.
//   k_mem_flags     write i is new iff its slot's first word is i; its size
//                   counts iff it is new (Memtable.Add adds nothing on an
//                   overwrite: oldNode aliases the node).
//   scans           exclusive sums of the flags and of the sizes in arrival
//                   order = Count and memusage in front of every write.
//   k_mem_flush     Add's return values; the first write of the batch after
//                   which ShouldFlush holds (only a write where it starts to
//                   hold, or the batch's first, takes the atomicMin).
//   k_mem_state     one lane: Count, memusage, the indexed count, flush_at.
// Find: one lane per query (search_dev.hpp's Query) probes and compares with
// the record at the slot's latest word; that record's Status and the hit word
// are the search layer's answers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "context.hpp"
#include "search_dev.hpp"

using namespace nkv;

namespace {

constexpr uint64_t kEmpty = ~uint64_t(0);
constexpr uint32_t kSeed = 0x6d656d74u;  // the index's murmur3 seed
constexpr unsigned kErrRecord = 1;  // a record's span, or where it ends
constexpr unsigned kErrCount = 2;   // the indexed count is not n_done
constexpr unsigned kErrProbe = 4;   // a probe ran out of slots or met an index past n: the index is not this log's

struct Log {  // kernel argument: the write log
    const uint8_t* s;
    uint64_t len;
    const uint64_t* off;
};

__device__ __forceinline__ uint32_t hash_key(const uint8_t* key, uint64_t len) {
    uint32_t h[kBloomMaxK];
    mm_states(key, len, kSeed, 1, h);
    return mm_fmix(h[0] ^ uint32_t(len));
}

// Key a (prefix pa, la bytes) equals the lb bytes at b.
__device__ __forceinline__ bool same_key(uint64_t pa, uint64_t la, const uint8_t* a, const uint8_t* b, uint64_t lb) {
    if (la != lb || pa != key_prefix(b, lb)) return false;
    return la <= 8 || cmp_bytes(a + 8, la - 8, b + 8, lb - 8) == 0;
}

__global__ __launch_bounds__(kBlock) void k_mem_validate(Log G, uint32_t n_done, uint32_t n,
                                                         const uint64_t* __restrict__ state,
                                                         uint64_t* __restrict__ size, unsigned int* err) {
    const uint64_t g = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (g >= n - n_done) return;
    const uint32_t i = n_done + uint32_t(g);
    DenseEntry e;
    bool bad;
    if (dense_entry(G.s, G.len, G.off, i, n, &e, &bad)) size[g] = e.size;
    if (g == 0 && n_done) {  // the batch starts where the indexed records end
        uint64_t ks, vs;
        const uint64_t o = G.off[n_done - 1];
        bad = bad || !record_span_in(G.s, G.len, o, &ks, &vs) || o + kHdr + ks + vs != G.off[n_done];
    }
    if (bad) atomicOr(err, kErrRecord);
    if (g == 0 && state[2] != n_done) atomicOr(err, kErrCount);
}

__global__ __launch_bounds__(kBlock) void k_mem_insert(Log G, uint32_t n_done, uint32_t n,
                                                       unsigned long long* slots, uint32_t mask,
                                                       uint32_t* __restrict__ slot_of, unsigned int* err) {
    if (*err) return;
    const uint64_t g = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (g >= n - n_done) return;
    const uint32_t i = n_done + uint32_t(g);
    const uint64_t at = G.off[i];  // validated
    const uint64_t kl = ld_le64(G.s + at + kAtKeySize);
    const uint8_t* key = G.s + at + kHdr;
    const uint64_t pfx = key_prefix(key, kl);
    uint32_t s = hash_key(key, kl) & mask;
    bool done = false, joined = false;  // joined: the slot was taken by this key already
    uint32_t first = 0, latest = 0;
    for (uint64_t step = 0; step <= mask; ++step, s = (s + 1) & mask) {
        unsigned long long v = __hip_atomic_load(slots + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (v == kEmpty) {
            v = atomicCAS(slots + s, kEmpty, (uint64_t(i) << 32) | i);
            if (v == kEmpty) {
                done = true;
                break;
            }
        }
        first = uint32_t(v), latest = uint32_t(v >> 32);
        if (first >= n) break;  // not an index of this log
        const uint64_t o = G.off[first];
        uint64_t ks;
        if (!key_span_in(G.s, G.len, o, &ks)) break;
        if (same_key(pfx, kl, key, G.s + o + kHdr, ks)) {
            done = joined = true;
            break;
        }
    }
    if (!done) atomicOr(err, kErrProbe);
    slot_of[g] = s;
    // Hot keys: the lanes of a wave that joined one slot are combined before the
    // atomics.  Lane order is arrival order, so of each such group the lowest
    // lane carries the minimum and the highest the maximum; the others are
    // covered by them.  One round per distinct slot among the joined lanes.
    const uint32_t lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(joined);
    while (todo) {
        const int lead = __ffsll((long long)todo) - 1;
        const unsigned long long group = __ballot(joined && s == uint32_t(__shfl(int(s), lead)));
        if ((group >> lane) & 1) {
            unsigned int* w = reinterpret_cast<unsigned int*>(slots + s);
            if (lane == uint32_t(__ffsll((long long)group) - 1) && i < first) atomicMin(w, i);
            if (lane == 63u - uint32_t(__clzll((long long)group)) && i > latest) atomicMax(w + 1, i);
        }
        todo &= ~group;
    }
}

__global__ __launch_bounds__(kBlock) void k_mem_flags(uint32_t n_done, uint32_t n, const uint64_t* __restrict__ slots,
                                                      const uint32_t* __restrict__ slot_of,
                                                      uint64_t* __restrict__ size, uint64_t* __restrict__ flag,
                                                      const unsigned int* __restrict__ err) {
    if (*err) return;
    const uint64_t g = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (g >= n - n_done) return;
    const bool is_new = uint32_t(slots[slot_of[g]]) == n_done + uint32_t(g);
    flag[g] = is_new ? 1 : 0;
    if (!is_new) size[g] = 0;
}

struct FlushRule {  // memtable.go:70-73
    int strategy;
    uint64_t capacity, threshold;
    __device__ bool holds(uint64_t count, uint64_t memusage) const {
        return ((strategy & NKV_FLUSH_BY_CAPACITY) && count == capacity) ||
               ((strategy & NKV_FLUSH_BY_THRESHOLD) && memusage >= threshold);
    }
};

__global__ __launch_bounds__(kBlock) void k_mem_flush(uint32_t n_done, uint32_t n, const uint64_t* __restrict__ flag,
                                                      const uint64_t* __restrict__ size,
                                                      const uint64_t* __restrict__ xflag,
                                                      const uint64_t* __restrict__ xsize,
                                                      const uint64_t* __restrict__ state, FlushRule rule,
                                                      uint8_t* __restrict__ is_new, unsigned long long* flush_at,
                                                      const unsigned int* __restrict__ err) {
    if (*err) return;
    const uint64_t g = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (g >= n - n_done) return;
    // Count and memusage in front of write n_done + g and behind it
    const uint64_t cb = state[0] + xflag[g], mb = state[1] + xsize[g];
    const uint64_t ca = cb + flag[g], ma = mb + size[g];
    if (is_new) is_new[g] = uint8_t(flag[g]);
    if (rule.holds(ca, ma) && (g == 0 || !rule.holds(cb, mb))) atomicMin(flush_at, (unsigned long long)(n_done + g));
}

__global__ void k_mem_state(uint32_t n_done, uint32_t n, const uint64_t* __restrict__ flag,
                            const uint64_t* __restrict__ size, const uint64_t* __restrict__ xflag,
                            const uint64_t* __restrict__ xsize, uint64_t* __restrict__ state,
                            const unsigned long long* __restrict__ flush_at, const unsigned int* __restrict__ err) {
    if (*err) return;
    const uint64_t last = uint64_t(n - n_done) - 1;
    state[0] += xflag[last] + flag[last];
    state[1] += xsize[last] + size[last];
    state[2] = n;
    state[3] = *flush_at;
}

__global__ __launch_bounds__(kBlock) void k_mem_find(Log G, uint32_t n, const uint64_t* __restrict__ slots,
                                                     uint32_t mask, const uint8_t* __restrict__ keys,
                                                     const uint64_t* __restrict__ koff,
                                                     const uint64_t* __restrict__ klen, uint64_t q, uint32_t table_id,
                                                     int overlay, uint64_t* __restrict__ hit,
                                                     uint8_t* __restrict__ status, unsigned int* err) {
    const uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= q) return;
    const Query Q = query_of(keys, koff, klen, i);
    uint32_t s = hash_key(Q.key, Q.len) & mask;
    uint64_t found = kNoHit;
    uint8_t st = NKV_GET_ABSENT;
    bool bad = false, ended = false;
    for (uint64_t step = 0; step <= mask; ++step, s = (s + 1) & mask) {
        const uint64_t v = slots[s];
        if (v == kEmpty) {
            ended = true;
            break;
        }
        const uint32_t latest = uint32_t(v >> 32);
        uint64_t o = 0, ks = 0;
        if (latest >= n || !key_span_in(G.s, G.len, o = G.off[latest], &ks)) {
            bad = true;  // no match; nothing outside the log is read
            continue;
        }
        if (same_key(Q.pfx, Q.len, Q.key, G.s + o + kHdr, ks)) {
            found = latest;
            st = status_answer(G.s[o + kAtStatus]);
            ended = true;
            break;
        }
    }
    if (bad || !ended) atomicOr(err, 1u);
    if (found != kNoHit) {
        hit[i] = hit_word(table_id, found);
        status[i] = st;
    } else if (!overlay) {
        hit[i] = kNoHit;
        status[i] = NKV_GET_ABSENT;
    }
}

bool slots_ok(uint64_t slots) { return slots >= 2 && slots <= (uint64_t(1) << 32) && (slots & (slots - 1)) == 0; }

}  // namespace

extern "C" {

uint64_t nkv_memtable_index_bytes(uint64_t slots) { return slots_ok(slots) ? 8 * slots : 0; }

int nkv_memtable_clear_dev(nkv_ctx* c, void* d_index, uint64_t slots, uint64_t* d_state) try {
    TRY(bind(c));
    if (!d_index || !d_state || !slots_ok(slots)) return NKV_ERR_INVALID;
    HIPTRY(hipMemsetAsync(d_index, 0xFF, 8 * slots, c->stream));
    HIPTRY(hipMemsetAsync(d_state, 0, 24, c->stream));
    HIPTRY(hipMemsetAsync(d_state + 3, 0xFF, 8, c->stream));
    return NKV_OK;
} NKV_CATCH

int nkv_memtable_add_dev(nkv_ctx* c, const void* d_log, uint64_t log_len, const uint64_t* d_rec_off, uint64_t n_done,
                         uint64_t n, void* d_index, uint64_t slots, int strategy, uint64_t capacity,
                         uint64_t threshold, uint64_t* d_state, uint8_t* d_is_new, uint32_t* d_err) try {
    TRY(bind(c));
    if (!d_index || !d_state || !slots_ok(slots) || n_done > n || n > kMaxN || n > slots / 2) return NKV_ERR_INVALID;
    if (n && (!d_log || !d_rec_off || log_len / kHdr < n)) return NKV_ERR_INVALID;
    const uint64_t m = n - n_done;
    if (m == 0) {  // no write: no point at which to flush, and a clean verdict
        HIPTRY(hipMemsetAsync(d_state + 3, 0xFF, 8, c->stream));
        if (d_err) HIPTRY(hipMemsetAsync(d_err, 0, 4, c->stream));
        return NKV_OK;
    }
    const Log G{static_cast<const uint8_t*>(d_log), log_len, d_rec_off};

    // scratch in d_stmp (nothing in it outlives the call)
    uint64_t *size, *flag, *xsize, *xflag;
    uint32_t* slot_of;
    const auto carve = [&](Carver k) {
        size = k.take<uint64_t>(m);
        flag = k.take<uint64_t>(m);
        xsize = k.take<uint64_t>(m);
        xflag = k.take<uint64_t>(m);
        slot_of = k.take<uint32_t>(m);
        return k.bytes();
    };
    TRY(grow(c->d_stmp, carve(Carver())));
    carve(Carver(c->d_stmp.p));
    size_t tb = 0;
    HIPTRY(scan_exclusive_u64(flag, xflag, m, nullptr, &tb, c->stream));
    TRY(grow(c->d_tmp, tb));
    TRY(grow(c->d_stats, 16));  // [err | pad | flush_at]: sized here, before verdict_word takes its word
    unsigned long long* flush_at = static_cast<unsigned long long*>(c->d_stats.p) + 1;
    const uint32_t n0 = uint32_t(n_done), n1 = uint32_t(n), mask = uint32_t(slots - 1);
    const dim3 grid(blocks_for(m)), block(kBlock);

    // with NKV_TIMING_EVENTS: "leaf" = validate + insert + flags, "reduce" = scans + flush point + state
    TRY(mark(c, 0));
    unsigned int* err;
    TRY(verdict_word(c, d_err, &err));
    HIPTRY(hipMemsetAsync(flush_at, 0xFF, 8, c->stream));
    hipLaunchKernelGGL(k_mem_validate, grid, block, 0, c->stream, G, n0, n1, d_state, size, err);
    HIPTRY(hipGetLastError());
    hipLaunchKernelGGL(k_mem_insert, grid, block, 0, c->stream, G, n0, n1, static_cast<unsigned long long*>(d_index),
                       mask, slot_of, err);
    HIPTRY(hipGetLastError());
    hipLaunchKernelGGL(k_mem_flags, grid, block, 0, c->stream, n0, n1, static_cast<const uint64_t*>(d_index), slot_of,
                       size, flag, err);
    HIPTRY(hipGetLastError());
    TRY(mark(c, 1));
    HIPTRY(scan_exclusive_u64(flag, xflag, m, c->d_tmp.p, &tb, c->stream));
    HIPTRY(scan_exclusive_u64(size, xsize, m, c->d_tmp.p, &tb, c->stream));
    hipLaunchKernelGGL(k_mem_flush, grid, block, 0, c->stream, n0, n1, flag, size, xflag, xsize, d_state,
                       FlushRule{strategy, capacity, threshold}, d_is_new, flush_at, err);
    HIPTRY(hipGetLastError());
    hipLaunchKernelGGL(k_mem_state, dim3(1), dim3(1), 0, c->stream, n0, n1, flag, size, xflag, xsize, d_state,
                       flush_at, err);
    HIPTRY(hipGetLastError());
    TRY(mark(c, 2));
    return finish_verdict(c, d_err, err);
} NKV_CATCH

int nkv_memtable_find_dev(nkv_ctx* c, const void* d_log, uint64_t log_len, const uint64_t* d_rec_off, uint64_t n,
                          const void* d_index, uint64_t slots, const void* d_keys, const uint64_t* d_koff,
                          const uint64_t* d_klen, uint64_t q, uint32_t table_id, int overlay, uint64_t* d_hit,
                          uint8_t* d_status, uint32_t* d_err) try {
    TRY(bind(c));
    if (!d_index || !slots_ok(slots) || n > kMaxN || q > kMaxN || table_id >= NKV_LOOKUP_MAX_TABLES)
        return NKV_ERR_INVALID;
    if (n && (!d_log || !d_rec_off)) return NKV_ERR_INVALID;
    if (q == 0) return NKV_OK;
    if (!d_keys || !d_koff || !d_klen || !d_hit || !d_status) return NKV_ERR_INVALID;
    const Log G{static_cast<const uint8_t*>(d_log), log_len, d_rec_off};
    unsigned int* err;
    TRY(verdict_word(c, d_err, &err));
    hipLaunchKernelGGL(k_mem_find, dim3(blocks_for(q)), dim3(kBlock), 0, c->stream, G, uint32_t(n),
                       static_cast<const uint64_t*>(d_index), uint32_t(slots - 1), static_cast<const uint8_t*>(d_keys),
                       d_koff, d_klen, q, table_id, overlay, d_hit, d_status, err);
    HIPTRY(hipGetLastError());
    return finish_verdict(c, d_err, err);
} NKV_CATCH

}  // extern "C"
