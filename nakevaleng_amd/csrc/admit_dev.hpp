// admit_dev.hpp -- the arithmetic of the engine's admission step
// (engine/coreeng/coreeng.go:47-59 IsLegal, ds/tokenbucket/tokenbucket.go:51-83
// HasEnoughTokens / ToBytes / FromBytes), once, for admit.hip: the IsLegal
// compare, the bucket and its validity, the window-membership test, the state
// after rank w in either kind of window, and the upper-bound step of the
// window walk.  The functions are pure and compile as plain host C++
// (tests/cpp/test_admit_layer.cpp), as search_dev.hpp's upper half does.
//
// The closed form.  The legal requests of one user, in arrival order with
// non-decreasing times, fall into windows.  The initial window runs from the
// stored Timestamp S0 (a fresh bucket: the first request's time) up to the
// first request with t > S0 + R.  Every request that opens a new window is a
// reset; the next reset after one at time tj is the first later request with
// t > tj + R.  With w = the request's rank inside its window:
//   reset window    allowed iff w < MaxTokens; Tokens = MaxTokens - 1 - w if
//                   allowed, else 0; Timestamp = the reset's time
//   initial window  allowed iff w < max(0, Tokens0); Tokens = Tokens0 - 1 - w
//                   if allowed, else Tokens0 when Tokens0 <= 0 and 0 otherwise;
//                   Timestamp = S0
// Ranges (nkv_admit_dev's verdicts hold every bucket and time to them):
// MaxTokens and ResetInterval in 1..2^62 - 1, times and Timestamps in
// 0..2^62 - 1, so S0 + R, t - S0 and R - (t - S0) never wrap.  Tokens is any
// int64; w < 2^31.
#pragma once
#include <stdint.h>

#include "record_dev.hpp"  // NKV_HD, ld_le64

namespace nkv {

constexpr int64_t kAdmitMax = (int64_t(1) << 62) - 1;  // largest MaxTokens, ResetInterval, time

struct Bucket {  // tokenbucket.go:11-16, in ToBytes order
    int64_t max_tokens, tokens, stamp, interval;
};

// IsLegal (coreeng.go:47-59) is false: the key's first slen bytes are start's.
// The caller has checked klen >= slen (the reference indexes out of range).
NKV_HD inline bool is_internal(const uint8_t* key, const uint8_t* start, uint32_t slen) {
    uint32_t count = 0;
    for (uint32_t j = 0; j < slen; ++j) count += key[j] == start[j];
    return count == slen;
}

NKV_HD inline bool admit_param_ok(int64_t v) { return v >= 1 && v <= kAdmitMax; }
NKV_HD inline bool admit_time_ok(int64_t t) { return t >= 0 && t <= kAdmitMax; }

// FromBytes (tokenbucket.go:76-83) of 32 bytes at any alignment.
NKV_HD inline Bucket bucket_from(const uint8_t* p) {
    return Bucket{int64_t(ld_le64(p)), int64_t(ld_le64(p + 8)), int64_t(ld_le64(p + 16)), int64_t(ld_le64(p + 24))};
}

// A stored bucket the walk can take (Tokens may be anything).
NKV_HD inline bool bucket_ok(const Bucket& b) {
    return admit_param_ok(b.max_tokens) && admit_param_ok(b.interval) && admit_time_ok(b.stamp);
}

// tokenbucket.New at time now (tokenbucket.go:25-30)
NKV_HD inline Bucket bucket_new(int64_t max_tokens, int64_t interval, int64_t now) {
    return Bucket{max_tokens, max_tokens, now, interval};
}

// A request at time t still belongs to the window stamped `stamp`:
// tokenbucket.go:52's test is false.
NKV_HD inline bool in_window(int64_t t, int64_t stamp, int64_t interval) { return !(t - stamp > interval); }

// The bucket after the request of rank w in a window of user bucket b0 (its
// state in front of the user's first request): a reset window stamped t_reset,
// or (reset = false) the initial one.  Returns HasEnoughTokens' answer.
NKV_HD inline bool after_rank(const Bucket& b0, bool reset, int64_t t_reset, uint64_t w, Bucket* out) {
    const int64_t have = reset ? b0.max_tokens : (b0.tokens > 0 ? b0.tokens : 0);
    const bool allowed = int64_t(w) < have;
    out->max_tokens = b0.max_tokens;
    out->interval = b0.interval;
    out->stamp = reset ? t_reset : b0.stamp;
    if (allowed) out->tokens = have - 1 - int64_t(w);
    else out->tokens = (!reset && b0.tokens <= 0) ? b0.tokens : 0;
    return allowed;
}

// "Slow down, %d seconds to go" (coreeng.go:70) of a throttled request at t.
NKV_HD inline int64_t wait_of(const Bucket& b, int64_t t) { return b.interval - (t - b.stamp); }

// The upper-bound step: the first q in [from, n] with q == n or past(q), for a
// predicate that stays true once it is true.  It looks at `from` itself first,
// then gallops (1, 2, 4, .. ahead) and bisects the last stride, so a target d
// places ahead costs about 2 log2(d) probes whatever n is.
template <class P>
NKV_HD inline uint64_t first_past(uint64_t from, uint64_t n, P past) {
    if (from >= n || past(from)) return from;
    uint64_t lo = from, hi, step = 1;  // past(lo) is false
    for (;;) {
        hi = lo + step;
        if (hi >= n) {
            hi = n;
            break;
        }
        if (past(hi)) break;
        lo = hi;
        step *= 2;
    }
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (past(mid)) hi = mid;
        else lo = mid;
    }
    return hi;
}

}  // namespace nkv
