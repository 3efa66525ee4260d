// cpu_sort.cpp -- the CPU comparator of tools/bench_sort.py: a single-thread
// memtable flush of a write log held in memory.  The records' offsets are found
// by walking the headers, an index array is sorted with std::stable_sort by key
// (memcmp, then length: bytes.Compare), which leaves equal keys in arrival
// order, and one pass keeps the last record of each group of equal keys and
// copies it.  Same semantics as nkv_sort_records.  Built by the tool with
// g++ -O2 -shared.
#include <algorithm>

#include "cpu_common.hpp"

namespace {

inline int cmp_key(const uint8_t* a, const uint8_t* b) { return cpu::compare(cpu::record_key(a), cpu::record_key(b)); }

}  // namespace

// Returns the seconds the flush took; *n_out / *out_len as nkv_sort_records;
// src (nullable, n entries): the arrival index of every output record.
extern "C" double cpu_sort(const uint8_t* log, uint64_t log_len, uint64_t n, uint8_t* out, uint64_t* src,
                           uint64_t* n_out, uint64_t* out_len) {
    const auto t0 = cpu::Clock::now();
    std::vector<const uint8_t*> rec(n);
    uint64_t at = 0;
    for (uint64_t i = 0; i < n && at + 30 <= log_len; ++i) {
        rec[i] = log + at;
        at += cpu::record_size(log + at);
    }
    std::vector<uint32_t> order(n);
    for (uint64_t i = 0; i < n; ++i) order[i] = uint32_t(i);
    std::stable_sort(order.begin(), order.end(),
                     [&](uint32_t a, uint32_t b) { return cmp_key(rec[a], rec[b]) < 0; });
    uint64_t m = 0;
    at = 0;
    for (uint64_t s = 0; s < n; ++s) {
        if (s + 1 < n && cmp_key(rec[order[s]], rec[order[s + 1]]) == 0) continue;  // shadowed by a later write
        const uint8_t* r = rec[order[s]];
        const uint64_t size = cpu::record_size(r);
        memcpy(out + at, r, size);
        if (src) src[m] = order[s];
        at += size;
        ++m;
    }
    *n_out = m;
    *out_len = at;
    return cpu::since(t0);
}
