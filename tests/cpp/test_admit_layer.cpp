// The admission arithmetic of csrc/admit_dev.hpp as plain host C++: a
// stand-alone program (plain, and under ASan + UBSan).  One user's requests at
// non-decreasing times are answered twice: by the literal per-request loop of
// ds/tokenbucket/tokenbucket.go:51-64 (HasEnoughTokens on a bucket carried from
// request to request), and by the header -- the resets found by first_past over
// the times, the rank inside the window, after_rank and wait_of.  Every field
// of every bucket image, every verdict and every wait must agree.  The arrays
// are heap blocks of exactly their sizes, so a probe outside one is caught by
// the sanitizer; first_past's probes are counted and held to its bound.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "admit_dev.hpp"

using namespace nkv;

static int failures = 0;
#define CHECK(x)                                                  \
    do {                                                          \
        if (!(x)) {                                               \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x);   \
            ++failures;                                           \
        }                                                         \
    } while (0)

static uint64_t rng_state = 0x61646d6974ull;
static uint64_t rnd() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// tokenbucket.go:51-64 at time now
static bool has_enough_tokens(Bucket* tb, int64_t now) {
    if (now - tb->stamp > tb->interval) {
        tb->stamp = now;
        tb->tokens = tb->max_tokens - 1;
        return true;
    }
    if (tb->tokens > 0) {
        tb->tokens--;
        return true;
    }
    return false;
}

static bool same(const Bucket& a, const Bucket& b) {
    return a.max_tokens == b.max_tokens && a.tokens == b.tokens && a.stamp == b.stamp && a.interval == b.interval;
}

static void one_sequence(const Bucket& b0, const std::vector<int64_t>& times) {
    const uint64_t n = times.size();
    // the header's way: window starts by upper bound, then the rank
    std::vector<uint64_t> start_of(n);
    std::vector<uint8_t> reset_at(n, 0);
    {
        const int64_t* t = times.data();
        int64_t bound = b0.stamp + b0.interval;
        uint64_t q = 0, open = 0;  // open: where the window of the positions walked so far starts
        std::vector<uint64_t> starts;
        for (;;) {
            uint64_t probes = 0;
            const uint64_t from = q;
            q = first_past(q, n, [&](uint64_t j) {
                ++probes;
                CHECK(j < n);
                return t[j] > bound;
            });
            // about 2 log2(distance) probes: one at `from`, the gallop, the bisection
            uint64_t d = q - from + 1, lg = 0;
            while ((uint64_t(1) << lg) < d) ++lg;
            CHECK(probes <= 2 * lg + 2);
            CHECK(q <= n);
            for (uint64_t j = from; j < q; ++j) CHECK(in_window(t[j], bound - b0.interval, b0.interval));
            if (q >= n) break;
            CHECK(!in_window(t[q], bound - b0.interval, b0.interval));
            reset_at[q] = 1;
            starts.push_back(q);
            bound = t[q] + b0.interval;
            ++q;
        }
        uint64_t k = 0;
        for (uint64_t j = 0; j < n; ++j) {
            if (k < starts.size() && starts[k] == j) open = j, ++k;
            start_of[j] = open;
        }
    }
    Bucket lit = b0;
    for (uint64_t j = 0; j < n; ++j) {
        const bool want = has_enough_tokens(&lit, times[j]);
        const uint64_t ws = start_of[j];
        Bucket got;
        const bool allowed = after_rank(b0, reset_at[ws] != 0, times[ws], j - ws, &got);
        CHECK(allowed == want);
        CHECK(same(got, lit));
        if (!want) {
            CHECK(wait_of(got, times[j]) == lit.interval - (times[j] - lit.stamp));
            CHECK(wait_of(got, times[j]) >= 0);
        }
    }
}

int main() {
    // IsLegal: every byte of start must match; a longer key is judged by its head
    {
        const uint8_t start[3] = {'$', '#', '!'};
        const uint8_t k1[3] = {'$', '#', '!'}, k2[3] = {'$', '#', '?'}, k3[5] = {'$', '#', '!', 'a', 'b'},
                      k4[3] = {'?', '#', '!'};
        CHECK(is_internal(k1, start, 3) && !is_internal(k2, start, 3) && is_internal(k3, start, 3) &&
              !is_internal(k4, start, 3));
        CHECK(is_internal(k2, start, 2) && is_internal(k4 + 1, start + 1, 2));
    }
    // FromBytes at every alignment, the ranges, tokenbucket.New
    {
        std::vector<uint8_t> buf(32 + 7);
        for (int a = 0; a < 8; ++a) {
            uint8_t* p = buf.data() + a;
            const uint64_t v[4] = {100, uint64_t(-5), 1700000000, 60};
            for (int f = 0; f < 4; ++f)
                for (int b = 0; b < 8; ++b) p[8 * f + b] = uint8_t(v[f] >> (8 * b));
            const Bucket b = bucket_from(p);
            CHECK(b.max_tokens == 100 && b.tokens == -5 && b.stamp == 1700000000 && b.interval == 60 && bucket_ok(b));
        }
        CHECK(!bucket_ok(Bucket{0, 1, 0, 1}) && !bucket_ok(Bucket{1, 1, 0, 0}) && !bucket_ok(Bucket{1, 1, -1, 1}));
        CHECK(!bucket_ok(Bucket{kAdmitMax + 1, 1, 0, 1}) && !bucket_ok(Bucket{1, 1, kAdmitMax + 1, 1}));
        CHECK(bucket_ok(Bucket{kAdmitMax, INT64_MIN, kAdmitMax, kAdmitMax}));
        CHECK(admit_time_ok(0) && admit_time_ok(kAdmitMax) && !admit_time_ok(-1) && !admit_time_ok(kAdmitMax + 1));
        CHECK(same(bucket_new(7, 3, 99), Bucket{7, 7, 99, 3}));
        CHECK(in_window(10, 5, 5) && !in_window(11, 5, 5) && in_window(0, kAdmitMax, 1));
    }
    // first_past on hand-made inputs: from == n, true at from, true nowhere, every target in a run of 70
    {
        int never = 0;
        CHECK(first_past(5, 5, [&](uint64_t) { return ++never, true; }) == 5 && never == 0);
        CHECK(first_past(2, 9, [](uint64_t) { return true; }) == 2);
        CHECK(first_past(2, 9, [](uint64_t) { return false; }) == 9);
        for (uint64_t n = 1; n <= 70; ++n)
            for (uint64_t from = 0; from < n; ++from)
                for (uint64_t target = from; target <= n; ++target)
                    CHECK(first_past(from, n, [&](uint64_t j) { return j >= target; }) == target);
    }
    // literal == closed form: stored and fresh buckets, Tokens <= 0 and above Max, a Timestamp in the future,
    // steps of 0, of exactly R and R + 1, and long gaps
    for (int round = 0; round < 4000; ++round) {
        const int64_t R = 1 + int64_t(rnd() % 5), Max = 1 + int64_t(rnd() % 6);
        const int64_t t0 = 1000 + int64_t(rnd() % 50);
        Bucket b0 = bucket_new(Max, R, t0);
        const int kind = int(rnd() % 5);
        if (kind == 1) b0 = Bucket{Max, int64_t(rnd() % 12) - 4, t0 - int64_t(rnd() % 12), R};
        if (kind == 2) b0 = Bucket{Max, Max + int64_t(rnd() % 4), t0 + int64_t(rnd() % 9), R};  // the future
        if (kind == 3) b0 = Bucket{Max, 0, t0 - R - 1 + int64_t(rnd() % 3), R};                  // around the edge
        const uint64_t n = rnd() % 40;
        std::vector<int64_t> times(n);
        int64_t t = t0;
        for (uint64_t j = 0; j < n; ++j) {
            const uint64_t step = rnd() % 8;
            t += step < 4 ? 0 : (step == 4 ? 1 : (step == 5 ? R : (step == 6 ? R + 1 : int64_t(rnd() % 20))));
            times[j] = t;
        }
        one_sequence(b0, times);
    }
    // the extremes of the ranges: nothing wraps
    {
        const std::vector<int64_t> times = {0, 1, kAdmitMax - 1, kAdmitMax, kAdmitMax};
        one_sequence(Bucket{kAdmitMax, INT64_MAX, kAdmitMax, kAdmitMax}, times);
        one_sequence(Bucket{kAdmitMax, INT64_MIN, 0, kAdmitMax}, times);
        one_sequence(Bucket{1, INT64_MIN, 0, 1}, times);
        one_sequence(Bucket{1, INT64_MAX, 0, 1}, times);
    }
    if (failures) return printf("%d failures\n", failures), 1;
    printf("ok\n");
    return 0;
}
