// cpu_locate.cpp -- the host comparators of tools/bench_locate.py.
//
// cpu_index_walk: one thread follows the Summary payload and then the Index,
// entry by entry, writing the Index entries' offsets -- the only honest host
// baseline for a chain, whose next position is known only from the entry before.
// Returns the wall-clock seconds; *n_out / *s_out the entries met.
//
// cpu_locate: the same batch of keys over the same opened Index images in host
// memory, std::lower_bound over each table's entry offsets (keys compared in
// place as bytes.Compare does), the tables in order until one holds the key,
// on `threads` threads.  Filters are not consulted: a filter only prunes, so
// the hits are the device's.  hit[i] = (table << 32) | entry index, UINT64_MAX
// if no table holds key i; data_off[i] the entry's stored Offset, else -1.
#include <algorithm>

#include "cpu_common.hpp"

namespace {

using cpu::Key;
inline int cmp(const Key& a, const Key& b) { return cpu::compare(a, b); }
// an Index entry: KeySize | Offset | Key
inline Key key_of(const uint8_t* index, uint64_t off) { return Key{index + off + 16, cpu::le64(index + off)}; }

// the chain of img[0, len): offsets into out (nullable); entries met, or UINT64_MAX if it breaks
uint64_t walk(const uint8_t* img, uint64_t len, uint64_t* out) {
    uint64_t pos = 0, c = 0;
    while (pos < len) {
        if (len - pos < 16) return UINT64_MAX;
        const uint64_t ks = cpu::le64(img + pos);
        if (ks > len - pos - 16) return UINT64_MAX;
        if (out) out[c] = pos;
        ++c;
        pos += 16 + ks;
    }
    return c;
}

}  // namespace

extern "C" double cpu_index_walk(const uint8_t* index, uint64_t index_len, const uint8_t* summary,
                                 uint64_t summary_len, uint64_t* ent_off, uint64_t* n_out, uint64_t* s_out) {
    const auto t0 = cpu::Clock::now();
    uint64_t h[3] = {0, 0, 0};
    if (summary_len >= 24) memcpy(h, summary, 24);
    const uint64_t at = 24 + h[0] + h[1];
    *s_out = at + h[2] <= summary_len ? walk(summary + at, h[2], nullptr) : UINT64_MAX;
    *n_out = walk(index, index_len, ent_off);
    return cpu::since(t0);
}

extern "C" double cpu_locate(const uint8_t* const* indexes, const uint64_t* const* offs, const uint64_t* ns, int T,
                             const uint8_t* keys, const uint64_t* koff, const uint64_t* klen, uint64_t q,
                             uint64_t* hit, int64_t* data_off, int threads) {
    const auto t0 = cpu::Clock::now();
    cpu::parallel_ranges(threads, q, [&](int, uint64_t lo, uint64_t hi) {
        for (uint64_t i = lo; i < hi; ++i) {
            const Key k{keys + koff[i], klen[i]};
            uint64_t h = UINT64_MAX;
            int64_t d = -1;
            for (int t = 0; t < T && h == UINT64_MAX; ++t) {
                const uint64_t* b = offs[t];
                const uint64_t* e = b + ns[t];
                const uint64_t* it = std::lower_bound(
                    b, e, k, [&](uint64_t off, const Key& x) { return cmp(key_of(indexes[t], off), x) < 0; });
                if (it != e && cmp(key_of(indexes[t], *it), k) == 0) {
                    memcpy(&d, indexes[t] + *it + 8, 8);
                    if (d != -1) h = (uint64_t(t) << 32) | uint64_t(it - b);
                }
            }
            hit[i] = h;
            data_off[i] = h == UINT64_MAX ? -1 : d;
        }
    });
    return cpu::since(t0);
}
