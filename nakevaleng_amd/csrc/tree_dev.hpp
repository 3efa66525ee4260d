// tree_dev.hpp -- the node storage and the in-LDS subtree reduce shared by the
// leaf kernels (leaf.hip), the level kernels (reduce.hip) and the small tree
// (small_tree.hip).
//
// Node storage ("nodes" buffer): every level, bottom-up, level-major; level L
// holds ceil(n / 2^L) 20-byte digests in Go byte order (big-endian words);
// level 0 is the leaves, the last digest is the root.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sha1_dev.hpp"

namespace nkv {

// ---------------------------------------------------------------------------
// tree shape helpers (device side; host side mirrors them in context.hpp)

__device__ __forceinline__ uint64_t lvl_count(uint64_t n, int L) {
    return L == 0 ? n : ((n - 1) >> L) + 1;  // ceil(n / 2^L), n >= 1
}

__device__ __forceinline__ uint64_t lvl_start(uint64_t n, int L) {
    uint64_t s = 0;
    for (int j = 0; j < L; ++j) s += lvl_count(n, j);
    return s;
}

__device__ __forceinline__ void store_digest(uint8_t* nodes, uint64_t idx, const uint32_t h[5]) {
    uint32_t* p = reinterpret_cast<uint32_t*>(nodes + 20ull * idx);
#pragma unroll
    for (int k = 0; k < 5; ++k) p[k] = bswap32(h[k]);
}

__device__ __forceinline__ void load_digest(const uint8_t* nodes, uint64_t idx, uint32_t h[5]) {
    const uint32_t* p = reinterpret_cast<const uint32_t*>(nodes + 20ull * idx);
#pragma unroll
    for (int k = 0; k < 5; ++k) h[k] = bswap32(p[k]);
}

// ---------------------------------------------------------------------------
// Subtree reduce inside one 256-thread workgroup.
//
// lds[k][t] holds word k of the node at index lo + t of level j0 (t < 256).
// Levels j0+1 .. jmax are computed; each level's nodes are written to the
// global nodes buffer.  Node i of level j is SHA-1(c[2i] || c[2i+1]) when
// 2i+1 < n_{j-1}, else SHA-1(c[2i]) (the empty pad, merkletree.go:32-34).
template <int B>
__device__ __forceinline__ void subtree_reduce(uint32_t (*lds)[B], uint64_t n, int j0, int jmax, uint64_t lo,
                               uint8_t* nodes) {
    const int tid = threadIdx.x;
    uint64_t nprev = lvl_count(n, j0);
    uint64_t start_cur = lvl_start(n, j0) + nprev;
    uint64_t lo_prev = lo;
    int span = B;
    for (int j = j0 + 1; j <= jmax; ++j) {
        const uint64_t ncur = ((nprev - 1) >> 1) + 1;
        const uint64_t lo_cur = lo_prev >> 1;
        span >>= 1;
        // lanes [0, live) build this level's parents; every lane of a wave that
        // has one takes part (a lane past live rebuilds the last parent and
        // drops it): a wave with few active lanes computes up to 35 % slower on
        // some CUs, and the narrow top levels are a lone-wave chain
        // (sha1_value_all_lanes, tools/svc_shape.hip)
        const int live = ncur > lo_cur ? int(min<uint64_t>(uint64_t(span), ncur - lo_cur)) : 0;
        const bool act = tid < live;
        uint32_t out[5];
        __syncthreads();
        if ((tid & ~63) < live) {
            const int t = min(tid, live - 1);
            uint32_t l[5], r[5];
            const bool lone = (2 * (lo_cur + uint64_t(t)) + 1) >= nprev;
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                l[k] = lds[k][2 * t];
                r[k] = lone ? 0u : lds[k][2 * t + 1];
            }
            sha1_parent(l, r, lone, out);
        }
        __syncthreads();
        if (act) {
#pragma unroll
            for (int k = 0; k < 5; ++k) lds[k][tid] = out[k];
            store_digest(nodes, start_cur + lo_cur + tid, out);
        }
        nprev = ncur;
        start_cur += ncur;
        lo_prev = lo_cur;
    }
}

}  // namespace nkv
