// cpu_index.cpp -- the CPU comparator of tools/bench_index.py: makeIndexAndSummary
// (core/sstable/sstable.go:76-139) as one single-thread loop over a Data-table
// stream and its record offsets held in memory, writing both images into memory
// (the reference's loop is single-threaded too and goes through two bufio
// writers; this one has no file or buffer layer, so it is the faster of the two
// shapes).  Same inputs and bytes as nkv_index_summary_dev.  Built by the tool
// with g++ -O2 -shared.
#include "cpu_common.hpp"

namespace {

using cpu::le64;

inline uint8_t* put_entry(uint8_t* w, uint64_t ks, uint64_t off, const uint8_t* key) {
    memcpy(w, &ks, 8);
    memcpy(w + 8, &off, 8);
    memcpy(w + 16, key, ks);
    return w + 16 + ks;
}

}  // namespace

// Returns the seconds the loop took.  index / summary must hold the images
// (the tool sizes them from the device call's lengths); n >= 1, page >= 1.
extern "C" double cpu_index(const uint8_t* stream, const uint64_t* rec_off, uint64_t n, uint64_t page,
                            uint8_t* index, uint8_t* summary, uint64_t* index_len, uint64_t* summary_len) {
    const auto t0 = cpu::Clock::now();
    // the two header keys are known up front, so the entries go straight behind them
    const uint8_t *first = stream + rec_off[0], *last = stream + rec_off[n - 1];
    const uint64_t ks0 = le64(first + 14), ks1 = le64(last + 14);
    uint8_t* const entries = summary + 24 + ks0 + ks1;
    uint8_t* wi = index;
    uint8_t* ws = entries;
    for (uint64_t i = 0; i < n; ++i) {
        const uint8_t* r = stream + rec_off[i];
        const uint64_t ks = le64(r + 14);
        const uint64_t ioff = uint64_t(wi - index);
        wi = put_entry(wi, ks, rec_off[i], r + 30);
        if (i == 0 || i % page == 0 || i == n - 1) ws = put_entry(ws, ks, ioff, r + 30);
    }
    const uint64_t payload = uint64_t(ws - entries);
    memcpy(summary, &ks0, 8);
    memcpy(summary + 8, &ks1, 8);
    memcpy(summary + 16, &payload, 8);
    memcpy(summary + 24, first + 30, ks0);
    memcpy(summary + 24 + ks0, last + 30, ks1);
    *index_len = uint64_t(wi - index);
    *summary_len = uint64_t(ws - summary);
    return cpu::since(t0);
}
