// The sorted search of csrc/search_dev.hpp as plain host C++: a stand-alone
// program (plain, and under ASan + UBSan).  Every table is searched through
// both entry formats -- a small Data stream (key_span_in, the key behind the
// 30-byte header) and the Index built from it (entry_in, the key behind the two
// fields) -- and held to a linear scan: the stage, the index and the number of
// probes.  Images, offset arrays and query batches are heap blocks of exactly
// their sizes, so a read outside one is caught by the sanitizer.
//
// The probe counts in kProbes do not come from the code under test: they were
// recorded from these same inputs run through the two search functions that
// lookup.hip and locate.hip each carried before search_dev.hpp existed.  Both
// gave the same counts, so one table serves both formats.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "search_dev.hpp"

using namespace nkv;

static int failures = 0;
#define CHECK(x)                                                  \
    do {                                                          \
        if (!(x)) {                                               \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #x);   \
            ++failures;                                           \
        }                                                         \
    } while (0)

struct RecordFormat {
    static constexpr uint64_t kKeyAt = kHdr;
    static bool key_in(const uint8_t* s, uint64_t L, uint64_t o, uint64_t* ks) { return key_span_in(s, L, o, ks); }
};
struct IndexFormat {
    static constexpr uint64_t kKeyAt = kEntryHdr;
    static bool key_in(const uint8_t* s, uint64_t L, uint64_t o, uint64_t* ks) { return entry_in(s, L, o, ks); }
};

static void st_le64(uint8_t* p, uint64_t v) {
    for (int b = 0; b < 8; ++b) p[b] = uint8_t(v >> (8 * b));
}

// plain lexicographic order: memcmp on the common length, then the lengths
static int ref_cmp(const std::string& a, const std::string& b) {
    const size_t m = a.size() < b.size() ? a.size() : b.size();
    const int c = m ? memcmp(a.data(), b.data(), m) : 0;
    if (c) return c < 0 ? -1 : 1;
    return a.size() < b.size() ? -1 : (a.size() > b.size() ? 1 : 0);
}

// 129 distinct keys in ascending order, of 0, 1, 7, 8, 9 and 17 bytes.  Per
// byte value c: c, c^7, c^8 (each a proper prefix of the next), c^8 00 and
// c^8 FF (equal 8-byte prefixes, different behind them), c^17 and c^16 FF
// (different in the last byte only); c runs across 0x7F / 0x80.
static std::vector<std::string> key_pool() {
    std::vector<std::string> p;
    p.push_back(std::string());
    for (int i = 0; i < 19; ++i) {
        const char c = char(1 + 13 * i);
        p.push_back(std::string(1, c));
        p.push_back(std::string(7, c));
        p.push_back(std::string(8, c));
        p.push_back(std::string(8, c) + std::string(1, char(0x00)));
        p.push_back(std::string(8, c) + std::string(1, char(0xFF)));
        p.push_back(std::string(17, c));
        p.push_back(std::string(16, c) + std::string(1, char(0xFF)));
    }
    std::sort(p.begin(), p.end(), [](const std::string& a, const std::string& b) { return ref_cmp(a, b) < 0; });
    p.resize(129);
    for (size_t i = 0; i + 1 < p.size(); ++i) CHECK(ref_cmp(p[i], p[i + 1]) < 0);
    return p;
}

struct Image {  // one format's image of a table: heap blocks of exactly len bytes and n offsets
    uint8_t* img = nullptr;
    uint64_t len = 0;
    uint64_t* off = nullptr;
    uint64_t n = 0;
    uint64_t size_at = 0;  // where an entry's KeySize field lies
    Image() = default;
    Image(const Image&) = delete;
    ~Image() {
        free(img);
        free(off);
    }
};

// The Data stream of the held keys (record i: a Value of i % 3 bytes, Status
// i & 1) and the Index over it (entry i: the record's offset).
static void build(const std::vector<std::string>& held, Image* data, Image* index) {
    const uint64_t n = held.size();
    uint64_t dl = 0, il = 0;
    for (uint64_t i = 0; i < n; ++i) {
        dl += kHdr + held[i].size() + i % 3;
        il += kEntryHdr + held[i].size();
    }
    data->img = static_cast<uint8_t*>(malloc(dl));
    index->img = static_cast<uint8_t*>(malloc(il));
    data->off = static_cast<uint64_t*>(malloc(8 * n));
    index->off = static_cast<uint64_t*>(malloc(8 * n));
    memset(data->img, 0xEE, dl);
    data->len = dl, index->len = il, data->n = index->n = n;
    data->size_at = kAtKeySize, index->size_at = 0;
    uint64_t d = 0, e = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t ks = held[i].size();
        data->off[i] = d;
        index->off[i] = e;
        data->img[d + kAtStatus] = uint8_t(i & 1);
        st_le64(data->img + d + kAtKeySize, ks);
        st_le64(data->img + d + kAtValueSize, i % 3);
        memcpy(data->img + d + kHdr, held[i].data(), ks);
        st_le64(index->img + e, ks);
        st_le64(index->img + e + 8, d);
        memcpy(index->img + e + kEntryHdr, held[i].data(), ks);
        d += kHdr + ks + i % 3;
        e += kEntryHdr + ks;
    }
}

struct Batch {  // a query batch as the entries take it, in exact heap blocks
    uint8_t* keys;
    uint64_t *koff, *klen;
    explicit Batch(const std::vector<std::string>& q) {
        uint64_t total = 0;
        for (const std::string& k : q) total += k.size();
        keys = static_cast<uint8_t*>(malloc(total ? total : 1));
        koff = static_cast<uint64_t*>(malloc(8 * q.size()));
        klen = static_cast<uint64_t*>(malloc(8 * q.size()));
        uint64_t at = 0;
        for (size_t i = 0; i < q.size(); ++i) {
            koff[i] = at;
            klen[i] = q[i].size();
            memcpy(keys + at, q[i].data(), q[i].size());
            at += q[i].size();
        }
    }
    Batch(const Batch&) = delete;
    ~Batch() {
        free(keys);
        free(koff);
        free(klen);
    }
};

struct Case {
    int group;       // index into kProbes
    int at;          // the query's place in its group
    bool index_fmt;  // searched through the Index (else the Data stream)
    const Image* image;
    Query Q;
    uint32_t stage;  // what a linear scan says
    uint64_t found;
    bool bad;
};

// The linear scan: SUMMARY outside [K_0, K_(n-1)], FOUND at the equal key, else INDEX.
static void scan(const std::vector<std::string>& held, const std::string& q, uint32_t* stage, uint64_t* found) {
    *found = 0;
    *stage = NKV_STAGE_INDEX;
    if (ref_cmp(q, held.front()) < 0 || ref_cmp(q, held.back()) > 0) *stage = NKV_STAGE_SUMMARY;
    for (uint64_t j = 0; j < held.size(); ++j)
        if (ref_cmp(q, held[j]) == 0) *stage = NKV_STAGE_FOUND, *found = j;
}

static const uint64_t kSizes[] = {1, 2, 3, 4, 7, 64};

// Every case, in a fixed order.  Groups 0..5: per n, the held keys are the
// pool's odd places and the queries its places 0..2n: a key below K_0 (the
// empty key), every held key, a key in every gap, a key above K_(n-1).
// Groups 6..11: per n, the held keys are the even places from the empty key
// on, the queries places 0..2n-1 (nothing sorts below the empty key).
// Groups 12..14: n = 4 with one entry whose KeySize reaches outside the image
// -- entry 0 and entry 2 by 2^64 - 1, entry 3 (the image's last bytes) by one
// byte -- and the queries whose search must probe it: they end at INDEX, bad.
template <class Fn>
static void for_each_case(Fn fn) {
    const std::vector<std::string> pool = key_pool();
    int group = 0;
    for (int phase = 0; phase < 2; ++phase)
        for (uint64_t n : kSizes) {
            std::vector<std::string> held, qs;
            for (uint64_t i = 0; i < n; ++i) held.push_back(pool[2 * i + 1 - phase]);
            for (uint64_t i = 0; i < 2 * n + 1 - phase; ++i) qs.push_back(pool[i]);
            Image data, index;
            build(held, &data, &index);
            const Batch b(qs);
            for (int f = 0; f < 2; ++f)
                for (size_t i = 0; i < qs.size(); ++i) {
                    Case c{group, int(i), f == 1, f ? &index : &data, query_of(b.keys, b.koff, b.klen, i), 0, 0, false};
                    scan(held, qs[i], &c.stage, &c.found);
                    fn(c);
                }
            ++group;
        }
    const struct {
        uint64_t entry, first_query, last_query;
        bool by_one;
    } broken[] = {{0, 0, 8, false}, {2, 2, 6, false}, {3, 2, 8, true}};
    for (const auto& br : broken) {
        std::vector<std::string> held, qs;
        for (uint64_t i = 0; i < 4; ++i) held.push_back(pool[2 * i + 1]);
        for (uint64_t i = br.first_query; i <= br.last_query; ++i) qs.push_back(pool[i]);
        Image data, index;
        build(held, &data, &index);
        for (Image* im : {&data, &index}) {
            uint8_t* field = im->img + im->off[br.entry] + im->size_at;
            st_le64(field, br.by_one ? ld_le64(field) + 1 : ~uint64_t(0));
        }
        const Batch b(qs);
        for (int f = 0; f < 2; ++f)
            for (size_t i = 0; i < qs.size(); ++i)
                fn(Case{group, int(i), f == 1, f ? &index : &data, query_of(b.keys, b.koff, b.klen, i),
                        NKV_STAGE_INDEX, 0, true});
        ++group;
    }
}

// Probes per query, one digit each, in for_each_case's order (see the head of the file).
static const char* const kProbes[] = {
    "111",
    "11222",
    "1133322",
    "114443322",
    "115554435554422",
    "1188878886888788858887888688878884888788868887888588878886888788"
    "83888788868887888588878886888788848887888688878885888788868887722",
    "11",
    "1222",
    "133322",
    "14443322",
    "15554435554422",
    "1888788868887888588878886888788848887888688878885888788868887888"
    "3888788868887888588878886888788848887888688878885888788868887722",
    "111111111",
    "33333",
    "2222222",
};

template <class F>
static uint32_t run(const Image& im, const Query& Q, uint64_t* found, bool* bad, int* probes) {
    return search(im.n, [&](uint64_t j) {
        ++*probes;
        return probe<F>(Q, im.img, im.len, im.off, j);
    }, found, bad);
}

int main() {
    int cases = 0;
    for_each_case([&](const Case& c) {
        uint64_t found = 0;
        bool bad = false;
        int probes = 0;
        const uint32_t stage = c.index_fmt ? run<IndexFormat>(*c.image, c.Q, &found, &bad, &probes)
                                           : run<RecordFormat>(*c.image, c.Q, &found, &bad, &probes);
        const bool known = c.group < int(sizeof(kProbes) / sizeof(kProbes[0])) && c.at < int(strlen(kProbes[c.group]));
        CHECK(known);
        const bool ok = stage == c.stage && bad == c.bad && (stage != NKV_STAGE_FOUND || found == c.found) &&
                        known && probes == kProbes[c.group][c.at] - '0';
        if (!ok) {
            printf("FAIL group %d query %d %s: stage %u (want %u) index %llu (want %llu) bad %d (want %d) probes %d\n",
                   c.group, c.at, c.index_fmt ? "index" : "data", stage, c.stage, (unsigned long long)found,
                   (unsigned long long)c.found, int(bad), int(c.bad), probes);
            ++failures;
        }
        ++cases;
    });
    CHECK(cases == 2 * (168 + 162 + 9 + 5 + 7));
    if (failures) {
        printf("%d checks failed\n", failures);
        return 1;
    }
    printf("ok\n");
    return 0;
}
