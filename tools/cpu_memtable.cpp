// cpu_memtable.cpp -- the host comparator of tools/bench_memtable.py: the live
// memtable's Add and Find as a hash map over keys read in place in the log,
// std::unordered_map<std::string_view, (first, latest arrival index)>.
//   threads = 1   one map, the writes inserted in arrival order.
//   threads = T   T maps sharded by hash: every thread hashes a slice of the
//                 writes (pass 1), then walks all the hashes and inserts the
//                 writes of its shard in arrival order (pass 2); a find goes to
//                 the shard of its key's hash, the queries split in slices.
// Same answers as nkv_memtable_add_dev / nkv_memtable_find_dev: Add's return
// value per write, Count, memusage (the sizes of the first writes), and per
// query the arrival index of the key's latest write or UINT64_MAX.  Built by
// the tool with g++ -O2 -shared -pthread.
#include <string_view>
#include <unordered_map>

#include "cpu_common.hpp"

namespace {

struct Span {
    uint32_t first, latest;
};
using Map = std::unordered_map<std::string_view, Span>;
using cpu::since;

inline std::string_view key_at(const uint8_t* log, uint64_t off) {
    const cpu::Key k = cpu::record_key(log + off);
    return {reinterpret_cast<const char*>(k.p), size_t(k.len)};
}

}  // namespace

// seconds[0] = the add, seconds[1] = the find.  is_new: n bytes; totals: Count,
// memusage; latest: q entries.
extern "C" void cpu_memtable(const uint8_t* log, const uint64_t* off, uint64_t n, int threads, const uint8_t* keys,
                             const uint64_t* koff, const uint64_t* klen, uint64_t q, uint8_t* is_new,
                             uint64_t* totals, uint64_t* latest, double* seconds) {
    const int T = threads < 1 ? 1 : threads;
    std::vector<Map> maps(T);
    std::vector<uint64_t> count(T, 0), mem(T, 0);
    std::vector<size_t> hash(T > 1 ? n : 0);
    const std::hash<std::string_view> H;
    auto t0 = cpu::Clock::now();
    if (T > 1)
        cpu::parallel_ranges(T, n, [&](int, uint64_t lo, uint64_t hi) {
            for (uint64_t i = lo; i < hi; ++i) hash[i] = H(key_at(log, off[i]));
        });
    cpu::parallel_ranges(T, n, [&](int t, uint64_t, uint64_t) {  // every worker walks all the writes, for its shard
        Map& m = maps[t];
        m.reserve(n / T + 16);
        for (uint64_t i = 0; i < n; ++i) {
            if (T > 1 && int(hash[i] % T) != t) continue;
            auto [it, fresh] = m.try_emplace(key_at(log, off[i]), Span{uint32_t(i), uint32_t(i)});
            it->second.latest = uint32_t(i);
            is_new[i] = fresh;
            if (fresh) {
                ++count[t];
                mem[t] += cpu::record_size(log + off[i]);
            }
        }
    });
    seconds[0] = since(t0);
    totals[0] = totals[1] = 0;
    for (int t = 0; t < T; ++t) totals[0] += count[t], totals[1] += mem[t];
    t0 = cpu::Clock::now();
    cpu::parallel_ranges(T, q, [&](int, uint64_t lo, uint64_t hi) {
        for (uint64_t i = lo; i < hi; ++i) {
            const std::string_view k{reinterpret_cast<const char*>(keys + koff[i]), size_t(klen[i])};
            const Map& m = maps[T > 1 ? H(k) % T : 0];
            const auto it = m.find(k);
            latest[i] = it == m.end() ? ~uint64_t(0) : it->second.latest;
        }
    });
    seconds[1] = since(t0);
}
