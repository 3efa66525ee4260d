// reduce.hip -- the levels above the leaves and the Serialize image on gfx950.
//
//   K2w k_reduce2     build() levels (merkletree.go:31-64) two at a time at
//                     full lane use, while a level holds >= 64 Ki nodes.
//   K2x k_reduce_wide the bottom twelve levels in one launch.
//   K2  k_reduce      the rest: a 256-node slab of one level reduced up to 8
//                     levels in LDS per launch.
//   K3  k_bfs_image   Serialize() byte image (merkletree.go:67-92,
//                     merklenode.go:37-63) at closed-form offsets.
//
// The nodes buffer and subtree_reduce are tree_dev.hpp's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "internal.hpp"
#include "sha1_dev.hpp"
#include "tree_dev.hpp"

namespace nkv {

// K2: a B-node slab of level j0 (already in nodes) reduced up to
// min(j0 + log2 B, top) in LDS, one workgroup of B threads per slab: 8 levels
// per launch with B = 256, 10 with B = 1024 (the narrow levels are a chain of
// one compression per level, so fewer launches is a shorter tree).
template <int B>
__global__ __launch_bounds__(B) void k_reduce(uint8_t* __restrict__ nodes, uint64_t n, int j0, int jmax, Gate gate) {
    __shared__ uint32_t lds[5][B];
    if (!gate.open()) return;
    const uint64_t lo = uint64_t(blockIdx.x) * B;
    const uint64_t cnt = lvl_count(n, j0);
    const uint64_t idx = lo + threadIdx.x;
    uint32_t h[5] = {0u, 0u, 0u, 0u, 0u};
    if (idx < cnt) load_digest(nodes, lvl_start(n, j0) + idx, h);
#pragma unroll
    for (int k = 0; k < 5; ++k) lds[k][threadIdx.x] = h[k];
    subtree_reduce<B>(lds, n, j0, jmax, lo, nodes);
}

// K2w: the wide bottom levels at full lane use.  A wavefront takes 256 nodes
// of level j0: their 128 parents (two per lane), then those parents' 64
// parents (one per lane) when jmax >= j0 + 2.  A k_reduce slab runs 8 levels
// but keeps at most half a wave busy past its first two, while the two bottom
// levels hold three quarters of all parents: 3 wave-compressions per 256 nodes
// here against 9 there.
__global__ __launch_bounds__(kBlock) void k_reduce2(uint8_t* __restrict__ nodes, uint64_t n, int j0, int jmax,
                                                     Gate gate) {
    if (!gate.open()) return;
    const int lane = threadIdx.x & 63;
    const uint64_t w = uint64_t(blockIdx.x) * (kBlock / 64) + (threadIdx.x >> 6);
    const uint64_t n0 = lvl_count(n, j0), s0 = lvl_start(n, j0);
    const uint64_t n1 = ((n0 - 1) >> 1) + 1, s1 = s0 + n0;
    uint32_t hp[2][5];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
#pragma unroll
        for (int k = 0; k < 5; ++k) hp[p][k] = 0u;
        const uint64_t i1 = 128 * w + uint64_t(lane) + 64 * p;
        if (i1 < n1) {
            const bool lone = 2 * i1 + 1 >= n0;
            uint32_t l[5], r[5] = {0u, 0u, 0u, 0u, 0u};
            load_digest(nodes, s0 + 2 * i1, l);
            if (!lone) load_digest(nodes, s0 + 2 * i1 + 1, r);
            sha1_parent(l, r, lone, hp[p]);
            store_digest(nodes, s1 + i1, hp[p]);
        }
    }
    if (jmax < j0 + 2) return;
    const uint64_t n2 = ((n1 - 1) >> 1) + 1, s2 = s1 + n1;
    const uint64_t i2 = 64 * w + uint64_t(lane);
    // children 2 lane, 2 lane + 1 of this wave's 128: pass 0 for lane < 32
    const int src = (2 * lane) & 63;
    uint32_t l[5], r[5], h[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const uint32_t l0 = uint32_t(__shfl(int(hp[0][k]), src)), l1 = uint32_t(__shfl(int(hp[1][k]), src));
        const uint32_t r0 = uint32_t(__shfl(int(hp[0][k]), src + 1)), r1 = uint32_t(__shfl(int(hp[1][k]), src + 1));
        l[k] = lane < 32 ? l0 : l1;
        r[k] = lane < 32 ? r0 : r1;
    }
    if (i2 < n2) {
        const bool lone = 2 * i2 + 1 >= n1;
        sha1_parent(l, r, lone, h);
        store_digest(nodes, s2 + i2, h);
    }
}

// K2x: the bottom twelve levels in one launch.  A workgroup of 1024 threads
// (16 waves) takes 4096 nodes of level j0: each wave builds the two levels
// above its 256 nodes at full lane use exactly as k_reduce2 does (128 parents,
// two per lane, then their 64 parents by shuffles), the workgroup's 1024
// level-(j0 + 2) nodes go to LDS, and subtree_reduce<1024> builds ten more
// levels: jmax = min(j0 + 12, top).  Replaces k_reduce2 + one 1024-slab launch
// (the slab part is a chain of one compression per level either way).
__global__ __launch_bounds__(1024) void k_reduce_wide(uint8_t* __restrict__ nodes, uint64_t n, int j0, int jmax,
                                                      Gate gate) {
    __shared__ uint32_t lds[5][1024];
    if (!gate.open()) return;
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const uint64_t w = uint64_t(blockIdx.x) * 16 + uint64_t(wv);
    const uint64_t n0 = lvl_count(n, j0), s0 = lvl_start(n, j0);
    const uint64_t n1 = ((n0 - 1) >> 1) + 1, s1 = s0 + n0;
    uint32_t hp[2][5];
#pragma unroll
    for (int p = 0; p < 2; ++p) {
#pragma unroll
        for (int k = 0; k < 5; ++k) hp[p][k] = 0u;
        const uint64_t i1 = 128 * w + uint64_t(lane) + 64 * p;
        if (i1 < n1) {
            const bool lone = 2 * i1 + 1 >= n0;
            uint32_t l[5], r[5] = {0u, 0u, 0u, 0u, 0u};
            load_digest(nodes, s0 + 2 * i1, l);
            if (!lone) load_digest(nodes, s0 + 2 * i1 + 1, r);
            sha1_parent(l, r, lone, hp[p]);
            store_digest(nodes, s1 + i1, hp[p]);
        }
    }
    const uint64_t n2 = ((n1 - 1) >> 1) + 1, s2 = s1 + n1;
    const uint64_t i2 = 64 * w + uint64_t(lane);
    const int src = (2 * lane) & 63;
    uint32_t l[5], r[5], h[5] = {0u, 0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const uint32_t l0 = uint32_t(__shfl(int(hp[0][k]), src)), l1 = uint32_t(__shfl(int(hp[1][k]), src));
        const uint32_t r0 = uint32_t(__shfl(int(hp[0][k]), src + 1)), r1 = uint32_t(__shfl(int(hp[1][k]), src + 1));
        l[k] = lane < 32 ? l0 : l1;
        r[k] = lane < 32 ? r0 : r1;
    }
    if (i2 < n2) {
        const bool lone = 2 * i2 + 1 >= n1;
        sha1_parent(l, r, lone, h);
        store_digest(nodes, s2 + i2, h);
    }
    // level j0 + 2 of this workgroup's 4096 nodes: 1024 nodes, node 64 wv + lane
#pragma unroll
    for (int k = 0; k < 5; ++k) lds[k][threadIdx.x] = h[k];
    subtree_reduce<1024>(lds, n, j0 + 2, jmax, uint64_t(blockIdx.x) * 1024, nodes);
}

// ---------------------------------------------------------------------------
// K3: BFS image.  Levels are written top-down; level L contributes 21 bytes
// per node (0x00 flag + digest) plus one 0x01 byte for the pad of an odd
// level below the top.  One workgroup builds one 4 KiB segment of the image
// in LDS: for every level that overlaps the segment, each thread takes nodes
// of it (one 64-bit division by 21 per level, not per byte) and writes their
// 21-byte records, clipped to the segment, as byte stores into LDS; then each
// thread stores 16 aligned bytes of the segment.  A record that straddles two
// segments is written, clipped, by both workgroups.
constexpr uint32_t kBfsSeg = kBlock * 16;
__global__ __launch_bounds__(kBlock) void k_bfs_image(const uint8_t* __restrict__ nodes,
                                                       BfsLayout lay, uint8_t* __restrict__ img) {
    __shared__ __attribute__((aligned(16))) uint8_t seg[kBfsSeg];
    const uint64_t s0 = uint64_t(blockIdx.x) * kBfsSeg;
    if (s0 >= lay.total) return;
    const uint64_t s1 = min(s0 + kBfsSeg, lay.total);
    for (int L = 0; L < lay.nlev; ++L) {
        const uint64_t A = lay.img_start[L];
        const uint64_t E = A + 21 * lay.count[L];           // end of the node records
        const uint64_t Z = L + 1 < lay.nlev ? lay.img_start[L + 1] : lay.total;  // E or E + 1 (pad)
        if (Z <= s0 || A >= s1) continue;
        if (E < Z && E >= s0 && E < s1 && threadIdx.x == 0)
            seg[E - s0] = 0x01u;  // MERKLE_NODE_EMPTY pad (merklenode.go:11, merkletree.go:32-34)
        if (E <= s0) continue;
        const uint64_t k0 = s0 > A ? (s0 - A) / 21 : 0;
        const uint64_t k1 = (min(s1, E) - 1 - A) / 21;  // last node with a byte in the segment
        for (uint64_t k = k0 + threadIdx.x; k <= k1; k += kBlock) {
            const uint32_t* d = reinterpret_cast<const uint32_t*>(nodes + 20 * (lay.node_start[L] + k));
            uint32_t w[5];
#pragma unroll
            for (int i = 0; i < 5; ++i) w[i] = d[i];
            const int64_t pos = int64_t(A + 21 * k) - int64_t(s0);  // record start in the segment
            if (pos >= 0 && pos + 21 <= int64_t(kBfsSeg)) {
                uint8_t* o = seg + pos;
                o[0] = 0u;
#pragma unroll
                for (int j = 0; j < 20; ++j) o[1 + j] = uint8_t(w[j >> 2] >> (8 * (j & 3)));
            } else {
#pragma unroll
                for (int j = 0; j < 21; ++j) {
                    const int64_t q = pos + j;
                    if (q >= 0 && q < int64_t(kBfsSeg))
                        seg[q] = j == 0 ? 0u : uint8_t(w[(j - 1) >> 2] >> (8 * ((j - 1) & 3)));
                }
            }
        }
    }
    __syncthreads();
    // The image is a byte string and may lie at any address (nkv_merkle.h,
    // device outputs).  s0 is a multiple of 16, so every segment has the same
    // sh bytes up to the first 16-byte boundary of img: those go out as bytes
    // (as k_merge_copy's head does), then each thread stores the 16 aligned
    // bytes at sh + 16 t, or the clipped rest of the segment as bytes.
    // (Established by reading: the hardware also accepts misaligned 16-byte
    // stores, so the placement tests pin the bytes and the extent, not this
    // alignment handling.  Do not take it for guarded when simplifying.)
    const uint32_t sh = uint32_t(-reinterpret_cast<uintptr_t>(img)) & 15u;
    const uint32_t len = uint32_t(s1 - s0);
    if (threadIdx.x < min(sh, len)) img[s0 + threadIdx.x] = seg[threadIdx.x];
    const uint32_t c = sh + 16 * threadIdx.x;
    if (c + 16 <= len) {
        uint4 v;
        if (sh == 0) {
            v = *reinterpret_cast<const uint4*>(seg + c);
        } else {
            uint32_t w[4];
#pragma unroll
            for (int k = 0; k < 4; ++k)
                w[k] = uint32_t(seg[c + 4 * k]) | uint32_t(seg[c + 4 * k + 1]) << 8 |
                       uint32_t(seg[c + 4 * k + 2]) << 16 | uint32_t(seg[c + 4 * k + 3]) << 24;
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        *reinterpret_cast<uint4*>(img + s0 + c) = v;
    } else {
        for (uint32_t p = c; p < len; ++p) img[s0 + p] = seg[p];
    }
}

// ---------------------------------------------------------------------------
// host-side launchers

hipError_t launch_reduce(uint8_t* nodes, uint64_t n, int from_level, int top, hipStream_t s, Gate gate) {
    int j0 = from_level;
    // The widest levels two at a time at full lane use (k_reduce2, while a
    // level holds >= kReduce2Min = 512 Ki nodes: that launch is
    // compression-bound); then slabs, which are a chain of one compression per
    // level: 1024-node slabs (10 levels per launch) while a level holds more
    // than 256 nodes, then the last <= 8 levels in 256-node slabs.  At
    // n = 2^20: k_reduce2 0 -> 2, 1024-slabs 2 -> 12, 256-slab 12 -> 20: 52.5 us
    // against 60.7 us for r01's three k_reduce2 and two 256-slab launches
    // (tools/ab_reduce.sh, one box).
    // 4096-node workgroups build the bottom twelve levels in one launch
    // (k_reduce_wide) when the tree is that tall and the level between 64 Ki
    // and 2 Mi nodes: at most two 1024-thread workgroups per CU, so beyond
    // that the ten-level chains run in several rounds (at 8 Mi nodes 231 us
    // against 209 us for k_reduce2 + slabs; at 1 Mi 50.5 against 53.9 us)
    for (uint64_t cnt = j0 == 0 ? n : ((n - 1) >> j0) + 1;
         top - j0 >= 12 && cnt >= kReduceWideMin && cnt <= (uint64_t(2) << 20); cnt = ((cnt - 1) >> 12) + 1) {
        hipLaunchKernelGGL(k_reduce_wide, dim3(unsigned((cnt + 4095) / 4096)), dim3(1024), 0, s, nodes, n, j0,
                           j0 + 12, gate);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        j0 += 12;
    }
    for (uint64_t cnt = j0 == 0 ? n : ((n - 1) >> j0) + 1; top - j0 >= 2 && cnt >= kReduce2Min;
         cnt = ((cnt - 1) >> 2) + 1) {
        const uint64_t waves = (cnt + 255) / 256;
        hipLaunchKernelGGL(k_reduce2, dim3(unsigned((waves + 3) / 4)), dim3(kBlock), 0, s, nodes, n, j0, j0 + 2,
                           gate);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        j0 += 2;
    }
    while (j0 < top) {
        const uint64_t cnt = j0 == 0 ? n : ((n - 1) >> j0) + 1;
        if (cnt > 256 && top - j0 > kSlabLevels) {
            const int jmax = (j0 + 10 < top) ? j0 + 10 : top;
            hipLaunchKernelGGL(k_reduce<1024>, dim3(unsigned((cnt + 1023) / 1024)), dim3(1024), 0, s, nodes, n, j0,
                               jmax, gate);
            j0 = jmax;
        } else {
            const int jmax = (j0 + kSlabLevels < top) ? j0 + kSlabLevels : top;
            hipLaunchKernelGGL(k_reduce<kBlock>, dim3(blocks_for(cnt)), dim3(kBlock), 0, s, nodes, n, j0, jmax, gate);
            j0 = jmax;
        }
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_bfs_image(const uint8_t* nodes, const BfsLayout& lay, uint8_t* img,
                            hipStream_t s) {
    const uint64_t segs = (lay.total + kBfsSeg - 1) / kBfsSeg;
    if (segs == 0) return hipSuccess;
    hipLaunchKernelGGL(k_bfs_image, dim3(uint32_t(segs)), dim3(kBlock), 0, s, nodes, lay, img);
    return hipGetLastError();
}

}  // namespace nkv
