// cpu_lookup.cpp -- the host comparator of tools/bench_lookup.py: the same
// batch of keys over the same Data tables in host memory, std::lower_bound over
// each table's record offsets (keys compared in place as bytes.Compare does),
// the tables in order until one holds the key, on `threads` threads.  Filters
// are not consulted: a filter only prunes, so the hits are the device's.
//
// hit[i] = (table << 32) | record index, UINT64_MAX if no table holds key i.
// Returns the wall-clock seconds of the search.
#include <algorithm>

#include "cpu_common.hpp"

namespace {

using cpu::Key;
inline int cmp(const Key& a, const Key& b) { return cpu::compare(a, b); }
inline Key key_of(const uint8_t* stream, uint64_t off) { return cpu::record_key(stream + off); }

}  // namespace

extern "C" double cpu_lookup(const uint8_t* const* streams, const uint64_t* const* offs, const uint64_t* ns, int T,
                             const uint8_t* keys, const uint64_t* koff, const uint64_t* klen, uint64_t q,
                             uint64_t* hit, int threads) {
    const auto t0 = cpu::Clock::now();
    cpu::parallel_ranges(threads, q, [&](int, uint64_t lo, uint64_t hi) {
        for (uint64_t i = lo; i < hi; ++i) {
            const Key k{keys + koff[i], klen[i]};
            uint64_t h = UINT64_MAX;
            for (int t = 0; t < T && h == UINT64_MAX; ++t) {
                const uint64_t* b = offs[t];
                const uint64_t* e = b + ns[t];
                const uint64_t* it = std::lower_bound(
                    b, e, k, [&](uint64_t off, const Key& x) { return cmp(key_of(streams[t], off), x) < 0; });
                if (it != e && cmp(key_of(streams[t], *it), k) == 0) h = (uint64_t(t) << 32) | uint64_t(it - b);
            }
            hit[i] = h;
        }
    });
    return cpu::since(t0);
}
