// cpu_admit.cpp -- the host comparator of tools/admit_bench.py: the engine's
// admission as the literal per-request loop (coreeng.go:63-73 over
// tokenbucket.go:51-64), the buckets in a std::unordered_map<std::string_view,
// Bucket> keyed by users read in place.
//   threads = 1   one map, the requests served in arrival order.
//   threads = T   T maps sharded by the user's hash: every thread hashes a slice
//                 of the requests (pass 1), then walks all the hashes and serves
//                 the requests of its shard in arrival order (pass 2).
// Same answers as nkv_admit_dev: the verdict byte and the 32-byte bucket image
// per request.  Built by the tool with g++ -O2 -shared -pthread.
#include <string_view>
#include <unordered_map>

#include "../cpu_common.hpp"

namespace {

struct Bucket {
    int64_t max_tokens, tokens, stamp, interval;
};
using Map = std::unordered_map<std::string_view, Bucket>;
using cpu::since;

inline bool is_legal(const uint8_t* key, const uint8_t* start, uint64_t slen) {  // coreeng.go:47-59
    uint64_t count = 0;
    for (uint64_t j = 0; j < slen; ++j) count += key[j] == start[j];
    return count != slen;
}

inline bool has_enough_tokens(Bucket& tb, int64_t now) {  // tokenbucket.go:51-64
    if (now - tb.stamp > tb.interval) {
        tb.stamp = now;
        tb.tokens = tb.max_tokens - 1;
        return true;
    }
    if (tb.tokens > 0) {
        tb.tokens--;
        return true;
    }
    return false;
}

}  // namespace

// ts: n times, or null and ts_all.  verdict: n bytes; image: 32 n bytes (four int64 per request).
extern "C" void cpu_admit(const uint8_t* users, const uint64_t* uoff, const uint64_t* ulen, const uint8_t* keys,
                          const uint64_t* koff, const int64_t* ts, int64_t ts_all, uint64_t n, const uint8_t* start,
                          uint64_t start_len, int64_t max_tokens, int64_t interval, int threads, uint8_t* verdict,
                          int64_t* image, double* seconds) {
    const int T = threads < 1 ? 1 : threads;
    std::vector<Map> maps(T);
    std::vector<size_t> hash(T > 1 ? n : 0);
    const std::hash<std::string_view> H;
    const auto user_at = [&](uint64_t i) {
        return std::string_view{reinterpret_cast<const char*>(users + uoff[i]), size_t(ulen[i])};
    };
    const auto t0 = cpu::Clock::now();
    if (T > 1)
        cpu::parallel_ranges(T, n, [&](int, uint64_t lo, uint64_t hi) {
            for (uint64_t i = lo; i < hi; ++i) hash[i] = H(user_at(i));
        });
    cpu::parallel_ranges(T, n, [&](int t, uint64_t, uint64_t) {  // every worker walks all the requests, for its shard
        Map& m = maps[t];
        for (uint64_t i = 0; i < n; ++i) {
            if (T > 1 && int(hash[i] % T) != t) continue;
            int64_t* out = image + 4 * i;
            if (!is_legal(keys + koff[i], start, start_len)) {
                verdict[i] = 0;
                out[0] = out[1] = out[2] = out[3] = 0;
                continue;
            }
            const int64_t now = ts ? ts[i] : ts_all;
            // getTokenBucket: the stored bucket, or tokenbucket.New at this request's time
            auto it = m.find(user_at(i));
            Bucket tb = it == m.end() ? Bucket{max_tokens, max_tokens, now, interval} : it->second;
            const bool ok = has_enough_tokens(tb, now);
            if (ok) {  // putTokenBucket
                if (it == m.end()) m.emplace(user_at(i), tb);
                else it->second = tb;
            }
            verdict[i] = ok ? 1 : 2;
            out[0] = tb.max_tokens, out[1] = tb.tokens, out[2] = tb.stamp, out[3] = tb.interval;
        }
    });
    seconds[0] = since(t0);
}
