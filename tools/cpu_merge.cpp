// cpu_merge.cpp -- the CPU comparator of tools/bench_merge.py: a single-thread
// heap-based k-way merge of sorted Data-table runs held in memory (the
// reference's merge is single-threaded too; it re-sorts a slice per output
// record where this uses a heap, so this is the faster of the two shapes).
// Same semantics as nkv_merge_records: one record per key, newest Timestamp,
// ties by (predecessor key, run).  Built by the tool with g++ -O2 -shared.
#include <queue>

#include "cpu_common.hpp"

namespace {

using cpu::le64;

struct Head {
    const uint8_t* rec;   // the record
    const uint8_t* pred;  // its predecessor in the run, or null
    int run;
};

inline int cmp_key(const uint8_t* a, const uint8_t* b) {  // a null record sorts first ("no predecessor")
    if (!a || !b) return (a ? 1 : 0) - (b ? 1 : 0);
    return cpu::compare(cpu::record_key(a), cpu::record_key(b));
}
// true if a comes out after b
struct After {
    bool operator()(const Head& a, const Head& b) const {
        int c = cmp_key(a.rec, b.rec);
        if (c) return c > 0;
        const int64_t ta = int64_t(le64(a.rec + 4)), tb = int64_t(le64(b.rec + 4));
        if (ta != tb) return ta < tb;
        c = cmp_key(a.pred, b.pred);
        if (c) return c > 0;
        return a.run > b.run;
    }
};

}  // namespace

// Returns the seconds the merge took; *n_out / *out_len as nkv_merge_records.
extern "C" double cpu_merge(const uint8_t* const* streams, const uint64_t* stream_len, int k, uint8_t* out,
                            uint64_t* n_out, uint64_t* out_len) {
    const auto t0 = cpu::Clock::now();
    std::priority_queue<Head, std::vector<Head>, After> pq;
    std::vector<const uint8_t*> end(k);
    for (int r = 0; r < k; ++r) {
        end[r] = streams[r] + stream_len[r];
        if (stream_len[r]) pq.push(Head{streams[r], nullptr, r});
    }
    uint64_t n = 0, at = 0;
    const uint8_t* last = nullptr;  // the latest record written
    while (!pq.empty()) {
        const Head h = pq.top();
        pq.pop();
        const uint64_t size = cpu::record_size(h.rec);
        if (!last || cmp_key(last, h.rec) != 0) {  // the first of its key wins
            memcpy(out + at, h.rec, size);
            last = out + at;
            at += size;
            ++n;
        }
        if (h.rec + size < end[h.run]) pq.push(Head{h.rec + size, h.rec, h.run});
    }
    *n_out = n;
    *out_len = at;
    return cpu::since(t0);
}
