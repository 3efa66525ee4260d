// The shared record checks and the key order of csrc/record_dev.hpp as plain
// host C++: a stand-alone program (plain, and under ASan + UBSan).  The stream
// is a heap block of exactly L bytes, so a check that read a byte outside it
// before refusing would be caught by the sanitizer.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "record_dev.hpp"

using namespace nkv;

static int failures = 0;
#define CHECK(x)                                                  \
    do {                                                          \
        if (!(x)) {                                               \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x);   \
            ++failures;                                           \
        }                                                         \
    } while (0)

static const uint64_t L = 64;
static const uint64_t kMax = ~uint64_t(0);

static void st_le64(uint8_t* p, uint64_t v) {
    for (int b = 0; b < 8; ++b) p[b] = uint8_t(v >> (8 * b));
}

// A fresh stream of L bytes (0xEE) with one header at o.
static uint8_t* stream_with(uint64_t o, uint64_t ks, uint64_t vs) {
    uint8_t* s = static_cast<uint8_t*>(malloc(L));
    memset(s, 0xEE, L);
    st_le64(s + o + kAtKeySize, ks);
    st_le64(s + o + kAtValueSize, vs);
    return s;
}

static void check_spans(uint64_t o, uint64_t ks, uint64_t vs, bool key_ok, bool rec_ok) {
    uint8_t* s = o <= L - kHdr ? stream_with(o, ks, vs) : stream_with(0, 0, 0);
    uint64_t k = 777, k2 = 777, v = 777;
    CHECK(key_span_in(s, L, o, &k) == key_ok);
    CHECK(k == (key_ok ? ks : 777));  // a refusal yields nothing
    CHECK(record_span_in(s, L, o, &k2, &v) == rec_ok);
    CHECK(k2 == (rec_ok ? ks : 777) && v == (rec_ok ? vs : 777));
    free(s);
}

static void test_checks() {
    // offsets: the header must lie in [0, L)
    const uint64_t in[] = {0, L - 30};
    for (uint64_t o : in) {
        CHECK(header_in(o, L));
        check_spans(o, 0, 0, true, true);
    }
    const uint64_t out[] = {L - 29, L, L + 1, kMax, kMax - 28 /* 2^64 - 29 */};
    for (uint64_t o : out) {
        CHECK(!header_in(o, L));
        check_spans(o, 0, 0, false, false);
    }
    // KeySize against the room behind the header
    const uint64_t offs[] = {0, 7, L - 30};
    for (uint64_t o : offs) {
        const uint64_t room = L - o - kHdr;
        check_spans(o, room, 0, true, true);
        check_spans(o, room + 1, 0, false, false);
        check_spans(o, kMax, 0, false, false);
        check_spans(o, kMax, 1 + room, false, false);  // o + 30 + ks + vs wraps to the stream's end
        if (room < 8) continue;
        // ValueSize against what the key leaves
        const uint64_t ks = 8;
        check_spans(o, ks, room - ks, true, true);
        check_spans(o, ks, room - ks + 1, true, false);
        check_spans(o, ks, kMax - 3, true, false);  // ks + vs wraps to 4
        check_spans(o, ks, kMax, true, false);
    }
}

static void test_dense() {
    // two records of 1-byte key and 1-byte value: 32 + 32 bytes
    uint8_t* s = static_cast<uint8_t*>(malloc(L));
    memset(s, 0, L);
    for (uint64_t o : {uint64_t(0), uint64_t(32)}) {
        st_le64(s + o + kAtKeySize, 1);
        st_le64(s + o + kAtValueSize, 1);
        s[o + kHdr] = uint8_t(0xC0 + o);
    }
    uint64_t off[2] = {0, 32};
    DenseEntry e{};
    bool bad = true;
    CHECK(dense_entry(s, L, off, 0, 2, &e, &bad) && !bad);
    CHECK(e.pfx == uint64_t(0xC0) << 56 && e.klen == 1 && e.size == 32);
    CHECK(dense_entry(s, L, off, 1, 2, &e, &bad) && !bad);
    CHECK(e.pfx == uint64_t(0xE0) << 56 && e.klen == 1 && e.size == 32);
    CHECK(dense_entry(s, L, off, 0, 1, &e, &bad) && bad);  // the last record must end the stream
    off[1] = 33;                                            // a gap: record 0 ends at 32
    CHECK(dense_entry(s, L, off, 0, 2, &e, &bad) && bad);
    off[1] = 31;  // an overlap
    CHECK(dense_entry(s, L, off, 0, 2, &e, &bad) && bad);
    off[0] = 1;  // the first record does not start the stream
    CHECK(!dense_entry(s, L, off, 0, 2, &e, &bad) && bad);
    off[0] = 0;
    for (uint64_t o : {L - 29, L, kMax, kMax - 28, kMax - 15}) {
        off[1] = o;
        CHECK(!dense_entry(s, L, off, 1, 2, &e, &bad) && bad);
    }
    free(s);
}

static int sign(int x) { return (x > 0) - (x < 0); }

// plain lexicographic order: memcmp on the common length, then the lengths
static int ref_cmp(const std::string& a, const std::string& b) {
    const size_t m = a.size() < b.size() ? a.size() : b.size();
    const int c = m ? memcmp(a.data(), b.data(), m) : 0;
    if (c) return sign(c);
    return a.size() < b.size() ? -1 : (a.size() > b.size() ? 1 : 0);
}

static void test_order() {
    std::vector<std::string> keys;
    const size_t lens[] = {0, 1, 7, 8, 9, 16, 17};
    const int fills[] = {0x00, 0x61, 0xFF};
    const int vals[] = {0x00, 0x01, 0x7F, 0x80, 0xFF};
    for (size_t len : lens)
        for (int f : fills) {
            keys.push_back(std::string(len, char(f)));
            const size_t at[] = {0, 3, 7, 8, len ? len - 1 : 0};  // inside the prefix, at byte 8, the last byte
            for (size_t p : at)
                for (int v : vals) {
                    if (p >= len || v == f) continue;
                    std::string k(len, char(f));
                    k[p] = char(v);
                    keys.push_back(k);
                }
        }
    size_t read_tails = 0;
    for (const std::string& a : keys)
        for (const std::string& b : keys) {
            const uint8_t* ka = reinterpret_cast<const uint8_t*>(a.data());
            const uint8_t* kb = reinterpret_cast<const uint8_t*>(b.data());
            const uint64_t pa = key_prefix(ka, a.size()), pb = key_prefix(kb, b.size());
            const int want = ref_cmp(a, b);
            CHECK(cmp_bytes(ka, a.size(), kb, b.size()) == want);
            if (pa != pb) CHECK((pa < pb ? -1 : 1) == want);  // zero padding, unsigned order
            // the tails may be touched only when both keys are longer than 8 and share their first 8
            const bool tails = a.size() > 8 && b.size() > 8 && pa == pb;
            read_tails += tails;
            CHECK(cmp_prefixed(pa, a.size(), tails ? ka + 8 : nullptr, pb, b.size(), tails ? kb + 8 : nullptr) == want);
        }
    CHECK(read_tails > 0 && read_tails < keys.size() * keys.size());
    // the prefix itself
    const uint8_t k9[9] = {1, 2, 3, 4, 5, 6, 7, 8, 9};
    CHECK(key_prefix(k9, 0) == 0);
    CHECK(key_prefix(k9, 1) == 0x0100000000000000ull);
    CHECK(key_prefix(k9, 7) == 0x0102030405060700ull);
    CHECK(key_prefix(k9, 8) == 0x0102030405060708ull);
    CHECK(key_prefix(k9, 9) == 0x0102030405060708ull);
    CHECK(ld_le64(k9) == 0x0807060504030201ull && ld_le64(k9 + 1) == 0x0908070605040302ull);
}

int main() {
    test_checks();
    test_dense();
    test_order();
    if (failures) {
        printf("%d checks failed\n", failures);
        return 1;
    }
    printf("ok\n");
    return 0;
}
