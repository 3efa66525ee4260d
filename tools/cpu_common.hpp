// cpu_common.hpp -- what the host comparators tools/cpu_*.cpp share: the
// little-endian load, a record's key and size, bytes.Compare, the seconds since
// a time point, and the split of an index range over std::threads.  Only these
// helpers live here; each comparator's algorithm stays in its own file, because
// the algorithm is the baseline.  Included by path from the same directory, so
// the tools' g++ line needs no -I.
#pragma once
#include <stdint.h>
#include <string.h>

#include <chrono>
#include <thread>
#include <vector>

namespace cpu {

inline uint64_t le64(const uint8_t* p) {
    uint64_t v;
    memcpy(&v, p, 8);
    return v;
}

struct Key {
    const uint8_t* p;
    uint64_t len;
};

// bytes.Compare: memcmp over the shorter length, then the shorter key first; -1, 0 or 1
inline int compare(const Key& a, const Key& b) {
    const int c = memcmp(a.p, b.p, size_t(a.len < b.len ? a.len : b.len));
    if (c) return c < 0 ? -1 : 1;
    return a.len < b.len ? -1 : (a.len > b.len ? 1 : 0);
}

// a serialized record: KeySize at byte 14, ValueSize at byte 22, the key at byte 30
inline Key record_key(const uint8_t* rec) { return Key{rec + 30, le64(rec + 14)}; }
inline uint64_t record_size(const uint8_t* rec) { return 30 + le64(rec + 14) + le64(rec + 22); }

using Clock = std::chrono::steady_clock;
inline double since(Clock::time_point t0) { return std::chrono::duration<double>(Clock::now() - t0).count(); }

// f(w, lo, hi) for w in [0, threads): worker w gets [n * w / threads, n * (w + 1) / threads),
// so the ranges cover [0, n) once.  threads <= 1: one call on the calling thread.
template <class F>
void parallel_ranges(int threads, uint64_t n, F f) {
    if (threads <= 1) {
        f(0, uint64_t(0), n);
        return;
    }
    std::vector<std::thread> pool;
    for (int w = 0; w < threads; ++w)
        pool.emplace_back(f, w, n * uint64_t(w) / uint64_t(threads), n * uint64_t(w + 1) / uint64_t(threads));
    for (auto& th : pool) th.join();
}

}  // namespace cpu
