// admit.hip -- the engine's admission step on the device (engine/coreeng/
// coreeng.go:63-75, 184-199, 223-234 over ds/tokenbucket/tokenbucket.go:51-83):
// nkv_admit_dev.  For a batch of requests (user, key, now) in arrival order:
// IsLegal of the key, then the per-user token bucket's HasEnoughTokens, and the
// bucket's ToBytes image after every request.  The answers follow a per-user
// sequential recurrence; admit_dev.hpp states its closed form (windows, resets,
// rank inside a window) and holds the arithmetic.  Here the recurrence becomes
// grouping, sorting, window finding and ranking.
//
// Stages, all on the context's stream; every kernel behind the first reads the
// error word and leaves when it is set, and only the last one writes an output:
//   k_adm_validate  one lane per request: the user's and the key's span, the
//                   time's range and its order against request i - 1 (batch-wide
//                   non-decreasing: that makes a user's windows well defined and
//                   lets one array of times serve every search), a key shorter
//                   than `start`, and the IsLegal compare (`start` by value in
//                   the kernel argument).  Writes the legal flag.
//   k_adm_group     one lane per legal request: an open-addressed index of
//                   8-byte slots (first, latest) over the users, as memindex.hip
//                   keeps over keys: murmur3 probing (murmur_dev.hpp), an empty
//                   slot claimed by one 64-bit compare-and-swap, a taken one
//                   compared in place with the user of its first word and
//                   joined by atomicMin / atomicMax, the lanes of a wave on one
//                   slot combined first (their lowest lane carries the minimum,
//                   their highest the maximum).  slots = the power of two >= 2 n,
//                   all empty at the start, so every probe ends.  Every answer
//                   is a min or a max over a user's requests: independent of the
//                   order the lanes arrive in.
//   k_adm_words     group = the slot's first word; the sort word (group << 32) |
//                   i, for an illegal request (2^32 - 1) << 32 | i (behind every
//                   legal one; all words distinct); and for a user's first legal
//                   request the user's bucket in front of the batch: the stored
//                   one (bstatus LIVE, FromBytes at any alignment, checked) or
//                   tokenbucket.New at that request's time.
//   k_adm_tile      one workgroup sorts a tile of 1024 words in LDS by a bitonic
//                   network, a lane owning two compare-exchanges per step; the
//                   LDS layout is memtable.hip's: element e at slot e ^ 31 when
//                   bit 5 of e is set, so the two 32-element blocks a half-wave
//                   compares at distances below 32 fall on complementary bank
//                   pairs.  Slots past n hold all ones and are not stored.
//   k_adm_merge     ceil(log2(ceil(n / 1024))) merge-by-rank passes, one lane
//                   per word: its rank in the sibling run by binary search.
//   k_adm_heads     sorted position p: its time, and head = legal and another
//                   user than p - 1.  A user's requests are now one segment in
//                   arrival order, its times ascending.
//   k_adm_windows   one lane per USER (head) walks its resets, not its requests:
//                   the first reset is the first position of the segment with
//                   t > S0 + R, the next one after a reset at tj the first with
//                   t > tj + R -- an upper bound that looks at the immediate
//                   successor first and then gallops (admit_dev.hpp first_past),
//                   over the predicate "another user, or a later time", which is
//                   monotone from the head to the end of the array, so the
//                   segment's end is never needed.  Each reset is marked.
//                   A user's resets number at most 1 + (t_last - S0) / (R + 1):
//                   now is in seconds and R >= 1, so a batch that spans seconds
//                   has one or two per user whatever the skew.  The adversarial
//                   shape is one user whose every request lies more than R after
//                   the one before: every request is a reset, and one lane
//                   serves them as a chain of n dependent loads
//                   (tools/admit_bench.py measures it).
//   scan + k_adm_starts  an exclusive sum over the "head or reset" marks gives
//                   every position its window's ordinal; the window starts
//                   scatter their position by ordinal.
//   k_adm_apply     each position reads its window's start, forms its rank w,
//                   applies the closed form and scatters to arrival order: the
//                   verdict as a byte store, the 32-byte image as two 16-byte
//                   stores where d_bucket is 16-byte aligned and four 8-byte
//                   stores otherwise (the contract promises 8), wait, group, last.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "admit_dev.hpp"
#include "context.hpp"
#include "murmur_dev.hpp"

using namespace nkv;

namespace {

constexpr uint64_t kEmpty = ~uint64_t(0);
constexpr uint32_t kSeed = 0x61646d74u;  // the index's murmur3 seed
constexpr uint32_t kTile = 1024;         // words one workgroup sorts in LDS
constexpr uint32_t kIllegal = 0xFFFFFFFFu;  // high word of an illegal request's sort word
constexpr unsigned kErrSpan = 1;    // a span outside its blob
constexpr unsigned kErrShort = 2;   // a key shorter than start
constexpr unsigned kErrTime = 4;    // a time out of range or decreasing
constexpr unsigned kErrBucket = 8;  // a stored bucket out of range

struct Start {  // kernel argument: conf.InternalStart
    uint8_t b[64];
    uint32_t len;
};

struct Req {  // kernel argument: the requests
    const uint8_t* users;
    uint64_t users_len;
    const uint64_t *uoff, *ulen;
    const uint8_t* keys;
    uint64_t keys_len;
    const uint64_t *koff, *klen;
    const int64_t* ts;
    int64_t ts_all;
    const uint8_t* buckets;
    const uint64_t* boff;
    const uint8_t* bstatus;
    __device__ int64_t time(uint64_t i) const { return ts ? ts[i] : ts_all; }
};

__device__ __forceinline__ bool span_in(uint64_t off, uint64_t len, uint64_t blob) {
    return off <= blob && len <= blob - off;
}

__device__ __forceinline__ uint32_t hash_user(const uint8_t* u, uint64_t len) {
    uint32_t h[kBloomMaxK];
    mm_states(u, len, kSeed, 1, h);
    return mm_fmix(h[0] ^ uint32_t(len));
}

__global__ __launch_bounds__(kBlock) void k_adm_validate(Req Q, uint32_t n, Start S, uint8_t* __restrict__ legal,
                                                         unsigned int* err) {
    const uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= n) return;
    unsigned bad = 0;
    if (!span_in(Q.uoff[i], Q.ulen[i], Q.users_len)) bad |= kErrSpan;
    const int64_t t = Q.time(i);
    if (!admit_time_ok(t) || (Q.ts && i && Q.ts[i - 1] > t)) bad |= kErrTime;
    bool ok = true;
    if (Q.koff) {
        const uint64_t ko = Q.koff[i], kl = Q.klen[i];
        if (!span_in(ko, kl, Q.keys_len)) bad |= kErrSpan;
        else if (kl < S.len) bad |= kErrShort;
        else ok = !is_internal(Q.keys + ko, S.b, S.len);
    }
    legal[i] = ok ? 1 : 0;
    if (bad) atomicOr(err, bad);
}

__global__ __launch_bounds__(kBlock) void k_adm_group(Req Q, uint32_t n, const uint8_t* __restrict__ legal,
                                                      unsigned long long* slots, uint32_t mask,
                                                      uint32_t* __restrict__ slot_of, unsigned int* err) {
    if (*err) return;
    const uint64_t g = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (g >= n) return;
    const uint32_t i = uint32_t(g);
    const bool live = legal[i] != 0;
    uint32_t s = 0, first = 0, latest = 0;
    bool done = !live, joined = false;  // joined: the slot was taken by this user already
    if (live) {
        const uint8_t* u = Q.users + Q.uoff[i];  // validated
        const uint64_t ul = Q.ulen[i];
        const uint64_t pfx = key_prefix(u, ul);
        s = hash_user(u, ul) & mask;
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
            if (first >= n) break;  // not a request of this batch: cannot happen in an index this call cleared
            const uint64_t ol = Q.ulen[first];
            const uint8_t* o = Q.users + Q.uoff[first];
            if (ol == ul && key_prefix(o, ol) == pfx && (ul <= 8 || cmp_bytes(u + 8, ul - 8, o + 8, ol - 8) == 0)) {
                done = joined = true;
                break;
            }
        }
        slot_of[i] = s;
    }
    if (!done) atomicOr(err, kErrSpan);
    // Hot users: the lanes of a wave that joined one slot are combined before
    // the atomics.  Lane order is arrival order, so of each such group the
    // lowest lane carries the minimum and the highest the maximum.
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

__global__ __launch_bounds__(kBlock) void k_adm_words(Req Q, uint32_t n, const uint8_t* __restrict__ legal,
                                                      const uint64_t* __restrict__ slots,
                                                      const uint32_t* __restrict__ slot_of, int64_t max_tokens,
                                                      int64_t interval, uint64_t* __restrict__ word,
                                                      Bucket* __restrict__ user0, unsigned int* err) {
    if (*err) return;
    const uint64_t g = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (g >= n) return;
    const uint32_t i = uint32_t(g);
    if (!legal[i]) {
        word[i] = (uint64_t(kIllegal) << 32) | i;
        return;
    }
    const uint32_t first = uint32_t(slots[slot_of[i]]);
    word[i] = (uint64_t(first) << 32) | i;
    if (first != i) return;
    // the user's bucket in front of the batch (coreeng.go:165-174)
    Bucket b = bucket_new(max_tokens, interval, Q.time(i));
    if (Q.bstatus && Q.bstatus[i] == NKV_GET_LIVE) {
        b = bucket_from(Q.buckets + Q.boff[i]);
        if (!bucket_ok(b)) atomicOr(err, kErrBucket);
    }
    user0[i] = b;
}

__device__ __forceinline__ uint32_t lds_slot(uint32_t e) { return (e & 32) ? e ^ 31 : e; }

__global__ __launch_bounds__(kBlock) void k_adm_tile(uint64_t* __restrict__ word, uint32_t n,
                                                     const unsigned int* __restrict__ err) {
    __shared__ uint64_t l_w[kTile];
    if (*err) return;
    const uint64_t base = uint64_t(blockIdx.x) * kTile;
    for (uint32_t e = threadIdx.x; e < kTile; e += kBlock) {
        const uint64_t g = base + e;
        l_w[lds_slot(e)] = g < n ? word[g] : ~uint64_t(0);
    }
    __syncthreads();
#pragma unroll 1
    for (uint32_t k = 2; k <= kTile; k <<= 1) {
#pragma unroll 1
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = threadIdx.x; t < kTile / 2; t += kBlock) {
                const uint32_t i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
                const uint32_t wi = lds_slot(i), wp = lds_slot(p);
                const uint64_t a = l_w[wi], b = l_w[wp];
                const bool up = (i & k) == 0;  // this block of k ascends
                if (up ? b < a : a < b) {
                    l_w[wi] = b;
                    l_w[wp] = a;
                }
            }
            __syncthreads();
        }
    }
    for (uint32_t e = threadIdx.x; e < kTile; e += kBlock) {
        const uint64_t g = base + e;
        if (g >= n) break;  // the all-ones words sorted behind the tile's own
        word[g] = l_w[lds_slot(e)];
    }
}

__global__ __launch_bounds__(kBlock) void k_adm_merge(uint32_t n, uint64_t L, const uint64_t* __restrict__ in,
                                                      uint64_t* __restrict__ out,
                                                      const unsigned int* __restrict__ err) {
    if (*err) return;
    const uint64_t g = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (g >= n) return;
    const uint64_t r = g / L;         // this word's run
    const uint64_t sb = (r ^ 1) * L;  // where the sibling run starts
    const uint64_t a = in[g];
    uint64_t dst = g;                 // no sibling: copied through
    if (sb < n) {
        const uint64_t cnt = n - sb < L ? n - sb : L;
        uint64_t lo = 0, hi = cnt;    // words of the sibling below this one (all words differ)
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (in[sb + mid] < a) lo = mid + 1;
            else hi = mid;
        }
        dst = (r & ~uint64_t(1)) * L + (g - r * L) + lo;
    }
    out[dst] = a;
}

__global__ __launch_bounds__(kBlock) void k_adm_heads(Req Q, uint32_t n, const uint64_t* __restrict__ word,
                                                      int64_t* __restrict__ tsort, uint64_t* __restrict__ flag,
                                                      uint8_t* __restrict__ is_reset,
                                                      const unsigned int* __restrict__ err) {
    if (*err) return;
    const uint64_t p = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (p >= n) return;
    const uint64_t w = word[p];
    const uint32_t f = uint32_t(w >> 32);
    tsort[p] = Q.time(uint32_t(w));
    flag[p] = (f != kIllegal && (p == 0 || uint32_t(word[p - 1] >> 32) != f)) ? 1 : 0;
    is_reset[p] = 0;
}

__global__ __launch_bounds__(kBlock) void k_adm_windows(uint32_t n, const uint64_t* __restrict__ word,
                                                        const int64_t* __restrict__ tsort,
                                                        const Bucket* __restrict__ user0, uint64_t* flag,
                                                        uint8_t* is_reset, const unsigned int* __restrict__ err) {
    if (*err) return;
    const uint64_t p = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (p >= n) return;
    const uint32_t f = uint32_t(word[p] >> 32);
    // heads only (no lane has written a mark that is not a head's yet: resets
    // are marked at positions that are heads already or never become one)
    if (f == kIllegal || (p != 0 && uint32_t(word[p - 1] >> 32) == f)) return;
    const Bucket b = user0[f];
    int64_t bound = b.stamp + b.interval;  // the window holds t <= bound
    uint64_t q = p;
    for (;;) {
        q = first_past(q, uint64_t(n), [&](uint64_t j) { return uint32_t(word[j] >> 32) != f || tsort[j] > bound; });
        if (q >= n || uint32_t(word[q] >> 32) != f) break;
        flag[q] = 1;
        is_reset[q] = 1;
        bound = tsort[q] + b.interval;
        ++q;
    }
}

__global__ __launch_bounds__(kBlock) void k_adm_starts(uint32_t n, const uint64_t* __restrict__ flag,
                                                       const uint64_t* __restrict__ xflag,
                                                       uint32_t* __restrict__ wstart,
                                                       const unsigned int* __restrict__ err) {
    if (*err) return;
    const uint64_t p = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (p >= n) return;
    if (flag[p]) wstart[xflag[p]] = uint32_t(p);
}

struct Out {  // kernel argument: the outputs, by request
    uint8_t* verdict;
    uint8_t* bucket;
    int64_t* wait;
    uint64_t* group;
    uint8_t* last;
};

__device__ __forceinline__ void store_bucket(uint8_t* dst, bool wide, const Bucket& b) {
    if (wide) {
        uint4* o = reinterpret_cast<uint4*>(dst);
        o[0] = make_uint4(uint32_t(b.max_tokens), uint32_t(uint64_t(b.max_tokens) >> 32), uint32_t(b.tokens),
                          uint32_t(uint64_t(b.tokens) >> 32));
        o[1] = make_uint4(uint32_t(b.stamp), uint32_t(uint64_t(b.stamp) >> 32), uint32_t(b.interval),
                          uint32_t(uint64_t(b.interval) >> 32));
    } else {
        int64_t* o = reinterpret_cast<int64_t*>(dst);
        o[0] = b.max_tokens, o[1] = b.tokens, o[2] = b.stamp, o[3] = b.interval;
    }
}

__global__ __launch_bounds__(kBlock) void k_adm_apply(uint32_t n, const uint64_t* __restrict__ word,
                                                      const int64_t* __restrict__ tsort,
                                                      const Bucket* __restrict__ user0,
                                                      const uint64_t* __restrict__ flag,
                                                      const uint64_t* __restrict__ xflag,
                                                      const uint32_t* __restrict__ wstart,
                                                      const uint8_t* __restrict__ is_reset, Out O,
                                                      const unsigned int* __restrict__ err) {
    if (*err) return;
    const uint64_t p = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (p >= n) return;
    const uint64_t wd = word[p];
    const uint32_t f = uint32_t(wd >> 32), i = uint32_t(wd);
    const bool wide = (reinterpret_cast<uintptr_t>(O.bucket) & 15) == 0;
    Bucket b{0, 0, 0, 0};
    uint8_t verdict = NKV_ADMIT_ILLEGAL, last = 0;
    int64_t wait = 0;
    uint64_t group = ~uint64_t(0);
    if (f != kIllegal) {
        const uint32_t ws = wstart[xflag[p] + flag[p] - 1];  // this position's window starts there
        const bool allowed = after_rank(user0[f], is_reset[ws] != 0, tsort[ws], p - ws, &b);
        verdict = allowed ? NKV_ADMIT_ALLOWED : NKV_ADMIT_THROTTLED;
        if (!allowed) wait = wait_of(b, tsort[p]);
        group = f;
        last = (p + 1 == n || uint32_t(word[p + 1] >> 32) != f) ? 1 : 0;
    }
    O.verdict[i] = verdict;
    if (O.bucket) store_bucket(O.bucket + 32 * uint64_t(i), wide, b);
    if (O.wait) O.wait[i] = wait;
    if (O.group) O.group[i] = group;
    if (O.last) O.last[i] = last;
}

}  // namespace

extern "C" {

int nkv_admit_dev(nkv_ctx* c, const nkv_requests* req, const void* start, uint64_t start_len, int64_t max_tokens,
                  int64_t reset_interval, uint8_t* d_verdict, void* d_bucket, int64_t* d_wait, uint64_t* d_group,
                  uint8_t* d_last, uint32_t* d_err) try {
    TRY(bind(c));
    if (!req || !start || start_len < 1 || start_len > 64 || req->n > kMaxN) return NKV_ERR_INVALID;
    if (!admit_param_ok(max_tokens) || !admit_param_ok(reset_interval)) return NKV_ERR_INVALID;
    if ((!req->users && req->users_len) || (!req->keys && req->keys_len)) return NKV_ERR_INVALID;
    if (req->koff && !req->klen) return NKV_ERR_INVALID;
    const int stored = (req->buckets != nullptr) + (req->boff != nullptr) + (req->bstatus != nullptr);
    if (stored != 0 && stored != 3) return NKV_ERR_INVALID;
    const uint64_t n = req->n;
    if (n == 0) return NKV_OK;
    if (!req->uoff || !req->ulen || !d_verdict) return NKV_ERR_INVALID;

    Start S{};
    S.len = uint32_t(start_len);
    for (uint32_t j = 0; j < S.len; ++j) S.b[j] = static_cast<const uint8_t*>(start)[j];
    const Req Q{static_cast<const uint8_t*>(req->users), req->users_len, req->uoff, req->ulen,
                static_cast<const uint8_t*>(req->keys), req->keys_len, req->koff, req->klen, req->ts, req->ts_all,
                static_cast<const uint8_t*>(req->buckets), req->boff, req->bstatus};
    uint64_t slots = 2;
    while (slots < 2 * n) slots *= 2;

    // scratch in d_stmp (nothing in it outlives the call)
    unsigned long long* index;
    uint64_t *word[2], *flag, *xflag;
    int64_t* tsort;
    Bucket* user0;
    uint32_t *slot_of, *wstart;
    uint8_t *legal, *is_reset;
    const auto carve = [&](Carver k) {
        index = k.take<unsigned long long>(slots);
        for (auto& w : word) w = k.take<uint64_t>(n);
        flag = k.take<uint64_t>(n);
        xflag = k.take<uint64_t>(n);
        tsort = k.take<int64_t>(n);
        user0 = k.take<Bucket>(n);
        slot_of = k.take<uint32_t>(n);
        wstart = k.take<uint32_t>(n);
        legal = k.take<uint8_t>(n);
        is_reset = k.take<uint8_t>(n);
        return k.bytes();
    };
    TRY(grow(c->d_stmp, carve(Carver())));
    carve(Carver(c->d_stmp.p));
    size_t tb = 0;
    HIPTRY(scan_exclusive_u64(flag, xflag, n, nullptr, &tb, c->stream));
    TRY(grow(c->d_tmp, tb));
    const uint32_t n32 = uint32_t(n), mask = uint32_t(slots - 1);
    const dim3 grid(blocks_for(n)), block(kBlock);

    // with NKV_TIMING_EVENTS: "leaf" = validate, group, words and the sort; "reduce" = windows, ranks and the scatter
    TRY(mark(c, 0));
    unsigned int* err;
    TRY(verdict_word(c, d_err, &err));
    HIPTRY(hipMemsetAsync(index, 0xFF, 8 * slots, c->stream));
    hipLaunchKernelGGL(k_adm_validate, grid, block, 0, c->stream, Q, n32, S, legal, err);
    HIPTRY(hipGetLastError());
    hipLaunchKernelGGL(k_adm_group, grid, block, 0, c->stream, Q, n32, legal, index, mask, slot_of, err);
    HIPTRY(hipGetLastError());
    hipLaunchKernelGGL(k_adm_words, grid, block, 0, c->stream, Q, n32, legal, reinterpret_cast<const uint64_t*>(index),
                       slot_of, max_tokens, reset_interval, word[0], user0, err);
    HIPTRY(hipGetLastError());
    hipLaunchKernelGGL(k_adm_tile, dim3(unsigned((n + kTile - 1) / kTile)), block, 0, c->stream, word[0], n32, err);
    HIPTRY(hipGetLastError());
    int cur = 0;
    for (uint64_t L = kTile; L < n; L *= 2) {  // runs of L into runs of 2 L
        hipLaunchKernelGGL(k_adm_merge, grid, block, 0, c->stream, n32, L, word[cur], word[cur ^ 1], err);
        HIPTRY(hipGetLastError());
        cur ^= 1;
    }
    TRY(mark(c, 1));
    const uint64_t* sorted = word[cur];
    hipLaunchKernelGGL(k_adm_heads, grid, block, 0, c->stream, Q, n32, sorted, tsort, flag, is_reset, err);
    HIPTRY(hipGetLastError());
    hipLaunchKernelGGL(k_adm_windows, grid, block, 0, c->stream, n32, sorted, tsort, user0, flag, is_reset, err);
    HIPTRY(hipGetLastError());
    HIPTRY(scan_exclusive_u64(flag, xflag, n, c->d_tmp.p, &tb, c->stream));
    hipLaunchKernelGGL(k_adm_starts, grid, block, 0, c->stream, n32, flag, xflag, wstart, err);
    HIPTRY(hipGetLastError());
    hipLaunchKernelGGL(k_adm_apply, grid, block, 0, c->stream, n32, sorted, tsort, user0, flag, xflag, wstart, is_reset,
                       Out{d_verdict, static_cast<uint8_t*>(d_bucket), d_wait, d_group, d_last}, err);
    HIPTRY(hipGetLastError());
    TRY(mark(c, 2));
    return finish_verdict(c, d_err, err);
} NKV_CATCH

}  // extern "C"
