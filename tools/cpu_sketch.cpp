// cpu_sketch.cpp -- the host comparator of tools/bench_sketch.py: a plain loop
// of MurmurHash3_x86_32 plus the sketch update (ds/hll/hll.go:43-62,
// ds/cmsketch/cmsketch.go:76-87), on one thread or on several with per-thread
// copies that are merged at the end.  Built by the tool with g++ -O2.
#include <algorithm>

#include "cpu_common.hpp"

namespace {

inline uint32_t rotl(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }

uint32_t murmur3_32(const uint8_t* data, uint64_t len, uint32_t seed) {
    const uint32_t c1 = 0xcc9e2d51u, c2 = 0x1b873593u;
    uint32_t h = seed;
    const uint64_t nblocks = len / 4;
    for (uint64_t i = 0; i < nblocks; ++i) {
        uint32_t k;
        memcpy(&k, data + 4 * i, 4);
        k *= c1;
        k = rotl(k, 15);
        k *= c2;
        h ^= k;
        h = rotl(h, 13);
        h = h * 5 + 0xe6546b64u;
    }
    const uint8_t* tail = data + 4 * nblocks;
    uint32_t k = 0;
    switch (len & 3) {
        case 3: k ^= uint32_t(tail[2]) << 16;  // fall through
        case 2: k ^= uint32_t(tail[1]) << 8;   // fall through
        case 1:
            k ^= tail[0];
            k *= c1;
            k = rotl(k, 15);
            k *= c2;
            h ^= k;
    }
    h ^= uint32_t(len);
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    h ^= h >> 16;
    return h;
}

}  // namespace

// reg (2^p bytes) is max-ed in place; returns the seconds of the loop and the merge
extern "C" double cpu_hll(const uint8_t* base, const uint64_t* off, const uint64_t* len, uint64_t n, int p,
                          int threads, uint8_t* reg) {
    const uint64_t M = uint64_t(1) << p;
    threads = std::max(threads, 1);
    std::vector<std::vector<uint8_t>> part(threads, std::vector<uint8_t>(M, 0));
    const auto t0 = cpu::Clock::now();
    cpu::parallel_ranges(threads, n, [&](int t, uint64_t lo, uint64_t hi) {
        uint8_t* r = part[t].data();
        for (uint64_t i = lo; i < hi; ++i) {
            const uint32_t h = murmur3_32(base + off[i], len[i], 0);
            const uint8_t val = uint8_t(1 + (h ? __builtin_ctz(h) : 32));
            uint8_t& slot = r[h >> (32 - p)];
            if (slot < val) slot = val;
        }
    });
    for (int t = 0; t < threads; ++t)
        for (uint64_t j = 0; j < M; ++j) reg[j] = std::max(reg[j], part[t][j]);
    return cpu::since(t0);
}

// table (k rows of m counters) is added to in place
extern "C" double cpu_cms(const uint8_t* base, const uint64_t* off, const uint64_t* len, uint64_t n, uint32_t m,
                          uint32_t k, uint32_t seed0, int threads, uint32_t* table) {
    const uint64_t T = uint64_t(m) * k;
    threads = std::max(threads, 1);
    std::vector<std::vector<uint32_t>> part(threads, std::vector<uint32_t>(T, 0));
    const auto t0 = cpu::Clock::now();
    cpu::parallel_ranges(threads, n, [&](int t, uint64_t lo, uint64_t hi) {
        uint32_t* c = part[t].data();
        for (uint64_t i = lo; i < hi; ++i)
            for (uint32_t j = 0; j < k; ++j) c[uint64_t(j) * m + murmur3_32(base + off[i], len[i], seed0 + j) % m] += 1;
    });
    for (int t = 0; t < threads; ++t)
        for (uint64_t j = 0; j < T; ++j) table[j] += part[t][j];
    return cpu::since(t0);
}
