// cpu_encode.cpp -- the CPU comparator of tools/bench_encode.py: record.New +
// ToBytes over a batch of puts held in memory, zlib's crc32 over the key and
// then the value (chained, which is the checksum of Key ++ Value) and memcpy
// into the log.  One pass sums the sizes into the record offsets; the records
// are then encoded by `threads` threads over equal index ranges.  Same output as
// nkv_encode_records.  Built by the tool with g++ -O2 -shared -pthread -lz.
#include <zlib.h>

#include "cpu_common.hpp"

namespace {

inline void put_le(uint8_t* p, uint64_t v, int bytes) {
    for (int b = 0; b < bytes; ++b) p[b] = uint8_t(v >> (8 * b));
}

}  // namespace

// Returns the seconds the encode took; out receives the log, *out_len its
// length.  ts / status / type are nullable (ts_all, 0, 0).
extern "C" double cpu_encode(const uint8_t* keys, const uint64_t* koff, const uint64_t* klen, const uint8_t* vals,
                             const uint64_t* voff, const uint64_t* vlen, const int64_t* ts, int64_t ts_all,
                             const uint8_t* status, const uint8_t* type, uint64_t n, int threads, uint8_t* out,
                             uint64_t* out_len) {
    const auto t0 = cpu::Clock::now();
    std::vector<uint64_t> off(n + 1);
    off[0] = 0;
    for (uint64_t i = 0; i < n; ++i) off[i + 1] = off[i] + 30 + klen[i] + vlen[i];
    cpu::parallel_ranges(threads, n, [&](int, uint64_t lo, uint64_t hi) {
        for (uint64_t i = lo; i < hi; ++i) {
            const uint8_t *k = keys + koff[i], *v = vals + voff[i];
            uint8_t* r = out + off[i];
            uLong crc = crc32(0L, Z_NULL, 0);
            crc = crc32(crc, k, uInt(klen[i]));
            for (uint64_t at = 0; at < vlen[i]; at += 1u << 30)  // uInt lengths
                crc = crc32(crc, v + at, uInt(vlen[i] - at < (1u << 30) ? vlen[i] - at : 1u << 30));
            put_le(r, crc, 4);
            put_le(r + 4, uint64_t(ts ? ts[i] : ts_all), 8);
            r[12] = status ? status[i] : 0;
            r[13] = type ? type[i] : 0;
            put_le(r + 14, klen[i], 8);
            put_le(r + 22, vlen[i], 8);
            memcpy(r + 30, k, klen[i]);
            memcpy(r + 30 + klen[i], v, vlen[i]);
        }
    });
    *out_len = off[n];
    return cpu::since(t0);
}
