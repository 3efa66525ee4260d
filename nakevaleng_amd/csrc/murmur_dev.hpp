// murmur_dev.hpp -- MurmurHash3_x86_32 (spaolacci/murmur3 v1.1.0 Sum32) on the
// device, several seeds at once, shared by the filter build (bloom.hip) and the
// filter test of the point lookups (search_dev.hpp) and the memtable's hash.
//
// The key's 4-byte little-endian blocks come from aligned dword loads funnelled
// by the key's byte offset (v_alignbyte), so any alignment works and no load
// touches a dword without a key byte.  The block mix (k *= c1, rotl 15, *= c2)
// does not depend on the seed, so it is done once per block and shared by all
// hash states, which are kept in registers (up to kBloomMaxK per pass over the
// key).  idx = h % M by Lemire's fastmod (one 64-bit multiply + one 64x32 high
// multiply, exact for every 32-bit h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nkv {

constexpr int kBloomMaxK = 16;

__device__ __forceinline__ uint32_t mm_rotl(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }

__device__ __forceinline__ uint32_t mm_fmix(uint32_t h) {
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    h ^= h >> 16;
    return h;
}

__device__ __forceinline__ uint32_t mm_block(uint32_t k) {
    k *= 0xcc9e2d51u;
    k = mm_rotl(k, 15);
    return k * 0x1b873593u;
}

// Lemire fastmod: a % d with M = 2^64 / d rounded up (M = 0 for d = 1).
__device__ __forceinline__ uint32_t fastmod_u32(uint32_t a, uint64_t M, uint32_t d) {
    const uint64_t low = M * a;
    return uint32_t(__umul64hi(low, uint64_t(d)));
}

inline uint64_t fastmod_magic(uint32_t d) { return ~uint64_t(0) / d + 1; }

// h[j] = MurmurHash3_x86_32(key, seed0 + j0 + j) before the final length xor
// and fmix, for j < nk (<= kBloomMaxK).
__device__ __forceinline__ void mm_states(const uint8_t* key, uint64_t len, uint32_t seed, int nk,
                                          uint32_t h[kBloomMaxK]) {
#pragma unroll
    for (int j = 0; j < kBloomMaxK; ++j) h[j] = seed + uint32_t(j);
    const uint32_t s = uint32_t(reinterpret_cast<uintptr_t>(key)) & 3u;
    const uint32_t* q = reinterpret_cast<const uint32_t*>(key - s);  // stays a global pointer
    const uint64_t nb = len >> 2;
    const uint32_t nxt = s != 0u;  // the dword after q[i] holds key bytes only when s > 0
    for (uint64_t i = 0; i < nb; ++i) {
        const uint32_t k = mm_block(__builtin_amdgcn_alignbyte(q[i + nxt], q[i], s));
#pragma unroll
        for (int j = 0; j < kBloomMaxK; ++j)
            if (j < nk) h[j] = mm_rotl(h[j] ^ k, 13) * 5u + 0xe6546b64u;
    }
    const uint32_t r = uint32_t(len & 3u);
    if (r) {
        // bytes 4nb .. 4nb+r-1: in q[nb] and, if s + r > 4, q[nb + 1]
        const uint32_t w0 = q[nb];
        const uint32_t w1 = s + r > 4u ? q[nb + 1] : w0;
        const uint32_t t = __builtin_amdgcn_alignbyte(w1, w0, s) & (0xFFFFFFFFu >> (8 * (4 - r)));
        const uint32_t k = mm_block(t);
#pragma unroll
        for (int j = 0; j < kBloomMaxK; ++j)
            if (j < nk) h[j] ^= k;
    }
}

// Filter.Query (bloomfilter.go:93-111) of one key: every one of the k bits set.
// M = fastmod_magic(m).
__device__ __forceinline__ bool filter_query(const uint8_t* key, uint64_t len, const uint32_t* __restrict__ bits,
                                             uint32_t m, uint64_t M, uint32_t k, uint32_t seed0) {
    bool hit = true;
    for (uint32_t j0 = 0; j0 < k && hit; j0 += kBloomMaxK) {
        const int nk = int(min(k - j0, uint32_t(kBloomMaxK)));
        uint32_t h[kBloomMaxK];
        mm_states(key, len, seed0 + j0, nk, h);
#pragma unroll
        for (int j = 0; j < kBloomMaxK; ++j) {
            if (j < nk) {
                const uint32_t idx = fastmod_u32(mm_fmix(h[j] ^ uint32_t(len)), M, m);
                hit = hit && ((bits[idx >> 5] >> (idx & 31u)) & 1u);
            }
        }
    }
    return hit;
}

}  // namespace nkv
