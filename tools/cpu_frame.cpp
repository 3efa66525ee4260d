// cpu_frame.cpp -- the host walk tools/bench_frame.py times the device against:
// record.Deserialize's loop (core/record/record.go:119-172) in closed form over
// bytes in host memory, one thread, one dependent load per record.  Built by
// the tool with g++ into build/cpu_frame.so.
#include "cpu_common.hpp"

extern "C" {

// Segment j = [seg[j], seg[j + 1]), the last ends at L; S == 0: the one segment
// [0, L).  off_out receives the accepted offsets; returns their number, the
// seconds taken in *secs and the bytes of whole records in *whole.
uint64_t cpu_frame(const uint8_t* s, uint64_t L, const uint64_t* seg, uint64_t S, uint64_t* off_out, double* secs,
                   uint64_t* whole) {
    const auto t0 = cpu::Clock::now();
    uint64_t n = 0, bytes = 0;
    const uint64_t Se = S ? S : 1;
    for (uint64_t j = 0; j < Se; ++j) {
        const uint64_t a = S ? seg[j] : 0, e = j + 1 < S ? seg[j + 1] : L;
        uint64_t p = a;
        while (e - p >= 30) {
            const uint64_t ks = cpu::le64(s + p + 14), vs = cpu::le64(s + p + 22);
            const uint64_t room = e - p - 30;
            if (ks > room || vs > room - ks) break;
            off_out[n++] = p;
            p += 30 + ks + vs;
        }
        bytes += p - a;
    }
    *secs = cpu::since(t0);
    *whole = bytes;
    return n;
}

}  // extern "C"
