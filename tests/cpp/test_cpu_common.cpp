// The helpers the host comparators share (tools/cpu_common.hpp), as a
// stand-alone program: the key compare against memcmp-then-length, the range
// split covering [0, n) exactly once, the unaligned little-endian load, the
// record accessors.  Built by tests/test_cpu_common.py, once plain and once under
// AddressSanitizer + UndefinedBehaviorSanitizer.  Prints "ok" and exits 0.
#include <stdio.h>
#include <stdlib.h>

#include <atomic>
#include <string>

#include "cpu_common.hpp"

#define CHECK(c)                                                    \
    do {                                                            \
        if (!(c)) {                                                 \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);   \
            exit(1);                                                \
        }                                                           \
    } while (0)

static int sign(int c) { return c < 0 ? -1 : (c > 0 ? 1 : 0); }

static int reference(const std::string& a, const std::string& b) {
    const int c = memcmp(a.data(), b.data(), a.size() < b.size() ? a.size() : b.size());
    if (c) return sign(c);
    return a.size() < b.size() ? -1 : (a.size() > b.size() ? 1 : 0);
}

static void test_compare() {
    // keys of every length, each in three forms: a shared prefix and then a low, a middle or a high last byte
    // (0xff against 0x01: a signed char compare would get it wrong), so pairs share prefixes of every length
    const size_t lens[] = {0, 1, 7, 8, 9, 17};
    std::vector<std::string> keys;
    for (size_t len : lens)
        for (int form = 0; form < 3; ++form) {
            std::string k(len, '\x61');
            if (len) k[len - 1] = form == 0 ? '\x01' : (form == 1 ? '\x61' : '\xff');
            keys.push_back(k);
        }
    for (const auto& a : keys)
        for (const auto& b : keys) {
            // exact-size heap copies, so a read past a key's end is an error under the sanitizer
            uint8_t* pa = static_cast<uint8_t*>(malloc(a.size() ? a.size() : 1));
            uint8_t* pb = static_cast<uint8_t*>(malloc(b.size() ? b.size() : 1));
            memcpy(pa, a.data(), a.size());
            memcpy(pb, b.data(), b.size());
            const int got = cpu::compare(cpu::Key{pa, a.size()}, cpu::Key{pb, b.size()});
            CHECK(got == reference(a, b));
            CHECK(got == -cpu::compare(cpu::Key{pb, b.size()}, cpu::Key{pa, a.size()}));
            CHECK((got == 0) == (a == b));
            free(pa);
            free(pb);
        }
}

static void test_parallel_ranges() {
    for (int threads : {1, 2, 16})
        for (uint64_t n : {uint64_t(0), uint64_t(1), uint64_t(threads - 1), uint64_t(threads), uint64_t(1000)}) {
            std::vector<std::atomic<int>> seen(n);
            for (auto& s : seen) s = 0;
            std::vector<std::atomic<int>> calls(threads);
            for (auto& c : calls) c = 0;
            std::atomic<uint64_t> total{0};
            cpu::parallel_ranges(threads, n, [&](int w, uint64_t lo, uint64_t hi) {
                CHECK(w >= 0 && w < threads && lo <= hi && hi <= n);
                calls[w] += 1;
                for (uint64_t i = lo; i < hi; ++i) seen[i] += 1;
                total += hi - lo;
            });
            for (uint64_t i = 0; i < n; ++i) CHECK(seen[i] == 1);
            for (int w = 0; w < threads; ++w) CHECK(calls[w] == 1);
            CHECK(total == n);
        }
    // ranges ascend with the worker: worker w ends where w + 1 begins
    std::vector<uint64_t> lo(16), hi(16);
    cpu::parallel_ranges(16, 1000, [&](int w, uint64_t a, uint64_t b) { lo[w] = a, hi[w] = b; });
    CHECK(lo[0] == 0 && hi[15] == 1000);
    for (int w = 0; w + 1 < 16; ++w) CHECK(hi[w] == lo[w + 1]);
}

static void test_le64_and_record() {
    // a record of a 3-byte key and a 2-byte value at an odd address
    uint8_t* buf = static_cast<uint8_t*>(malloc(1 + 35));
    uint8_t* rec = buf + 1;
    memset(rec, 0, 35);
    rec[14] = 3;
    rec[22] = 2;
    memcpy(rec + 30, "abc", 3);
    CHECK(cpu::le64(rec + 14) == 3 && cpu::le64(rec + 22) == 2);
    CHECK(cpu::record_size(rec) == 35);
    const cpu::Key k = cpu::record_key(rec);
    CHECK(k.p == rec + 30 && k.len == 3 && memcmp(k.p, "abc", 3) == 0);
    const uint8_t bytes[9] = {0xAA, 0x01, 0x02, 0x03, 0x04, 0x05, 0x06, 0x07, 0x08};
    memcpy(buf, bytes, 9);
    CHECK(cpu::le64(buf + 1) == 0x0807060504030201ull);  // little-endian, unaligned
    free(buf);
}

int main() {
    test_compare();
    test_parallel_ranges();
    test_le64_and_record();
    const auto t0 = cpu::Clock::now();
    const double a = cpu::since(t0), b = cpu::since(t0);
    CHECK(a >= 0 && b >= a && b < 60);
    printf("ok\n");
    return 0;
}
