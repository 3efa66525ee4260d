// frame.hip -- record boundaries of a raw byte stream on the device: the loop
// of record.Deserialize (core/record/record.go:119-172) that lsmtree.merge runs
// over a Data file (core/lsmtree/lsmtree.go:137-231) and wal.readEntireSegment
// over a WAL segment (core/wal/wal.go:293-328).  nkv_frame_records_dev /
// nkv_frame_records.
//
// Per segment [a, e): p = a; while record_span_in(stream, e, p) holds, p is a
// record and p += 30 + KeySize + ValueSize; the first p that fails ends the
// segment and [p, e) is its tail.
//
// Two paths give the same bytes (NKV_OPT_FRAME_PATH):
//   walk         one lane per segment follows its chain: k_walk_count, the scan
//                of the counts, k_walk_write.  Right for a WAL (five records
//                per segment) and the exact fallback for everything else.
//   speculative  for long segments:
//     k_frame_mark   every byte position is tested with the accept rule against
//                    the end of the segment that holds it; tiles of kMarkTile
//                    positions staged through LDS with a 29-byte halo; a bit
//                    per position, a count per 64.
//     scan, k_frame_pos    M valid starts (nodes) and pos[M], ascending.
//     k_frame_succ   jump[v] = the node at pos[v] + TotalSize if that is a
//                    valid start strictly inside the same segment, else v.
//     k_frame_starts, k_frame_round   the segment starts that are nodes are
//                    marked; ceil(log2(M + 1)) rounds, each a launch of its
//                    own: every marked v marks jump[v], and jump o jump goes to
//                    the other buffer, so round k applies exactly s^(2^k).
//                    Marking in place is safe: a marked node lies on a true
//                    chain, and so does whatever it marks.
//     k_frame_flags, scan, k_frame_last, k_frame_compact, k_frame_seg_out
//                    the marks' ranks are the record indices.
// No workgroup waits on another.  The segment offsets are checked by
// k_frame_segs before any kernel follows one: every later kernel returns at
// once when it refused.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bytes_dev.hpp"  // last_at_most
#include "context.hpp"

using namespace nkv;

namespace {

constexpr uint32_t kMarkTile = 4096;                 // positions per k_frame_mark workgroup
constexpr uint32_t kMarkLds = (kMarkTile + 64) / 4;  // dwords: 15 in front, the tile, the halo, the reader's reach
constexpr uint64_t kNone = ~uint64_t(0);
// auto: segments shorter than this on average are walked.  Measured on 1 Mi
// records of 146 bytes: the walk costs 0.65 us per record
// of the longest segment, the speculative path 0.9 ms for the table, and they
// meet near 650 records per segment.
constexpr uint64_t kAutoMeanSegment = 98304;

// soff[0 .. Se]: the segments' starts and, last, stream_len.  S == 0: the one
// segment [0, L).
__global__ __launch_bounds__(kBlock) void k_frame_segs(const uint64_t* __restrict__ seg_off, uint64_t S, uint64_t L,
                                                       uint64_t* __restrict__ soff, unsigned int* err) {
    const uint64_t j = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    const uint64_t Se = S ? S : 1;
    if (j > Se) return;
    const uint64_t v = S == 0 ? (j == 0 ? 0 : L) : (j < S ? seg_off[j] : L);
    const uint64_t w = j + 1 < S ? seg_off[j + 1] : L;  // the next entry (L behind the last)
    soff[j] = v;
    if (v > L || v > w) atomicOr(err, 1u);
}

// stats: [0] n, [1] bytes of whole records, [2] segments with a tail, [3] the lowest such
__device__ __forceinline__ void note_segment(unsigned long long* stats, uint64_t j, uint64_t cnt, uint64_t len,
                                             bool tail) {
    if (cnt) atomicAdd(&stats[0], (unsigned long long)cnt);
    if (len) atomicAdd(&stats[1], (unsigned long long)len);
    if (tail) {
        atomicAdd(&stats[2], 1ull);
        atomicMin(&stats[3], (unsigned long long)j);
    }
}

__global__ __launch_bounds__(kBlock) void k_walk_count(const uint8_t* __restrict__ s, const uint64_t* __restrict__ soff,
                                                       uint64_t Se, uint64_t* __restrict__ cnt,
                                                       uint64_t* __restrict__ seglen, unsigned long long* stats,
                                                       const unsigned int* err) {
    if (*err) return;
    const uint64_t j = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (j >= Se) return;
    const uint64_t a = soff[j], e = soff[j + 1];
    uint64_t p = a, c = 0, ks, vs;
    while (record_span_in(s, e, p, &ks, &vs)) {
        p += kHdr + ks + vs;  // <= e
        ++c;
    }
    cnt[j] = c;
    seglen[j] = p - a;
    note_segment(stats, j, c, p - a, p != e);
}

__global__ __launch_bounds__(kBlock) void k_walk_write(const uint8_t* __restrict__ s, const uint64_t* __restrict__ soff,
                                                       uint64_t Se, const uint64_t* __restrict__ first,
                                                       uint64_t* __restrict__ rec_off) {
    const uint64_t j = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (j >= Se) return;
    const uint64_t e = soff[j + 1];
    uint64_t p = soff[j], i = first[j], ks, vs;
    while (record_span_in(s, e, p, &ks, &vs)) {
        rec_off[i++] = p;
        p += kHdr + ks + vs;
    }
}

// seg_first (S + 1 entries, nullable) and seg_len (S entries, nullable) from
// the per-segment arrays; n: the records of the call.
__global__ __launch_bounds__(kBlock) void k_seg_out(const uint64_t* __restrict__ first,
                                                    const uint64_t* __restrict__ seglen, uint64_t S, uint64_t n,
                                                    uint64_t* __restrict__ seg_first, uint64_t* __restrict__ seg_len) {
    const uint64_t j = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (j > S) return;
    if (seg_first) seg_first[j] = j < S ? first[j] : n;
    if (seg_len && j < S) seg_len[j] = seglen[j];
}

// ---------------------------------------------------------------------------
// the speculative path

struct Marks {
    uint64_t* mask;  // W words: bit b of word w = position 64 w + b is a valid start
    uint64_t* cnt;   // W: the bits of each word
    uint64_t* coff;  // W + 1: their exclusive sums, coff[W] = M
    uint64_t W, L;
    // nodes in front of position q (q a node: its index); q <= L
    __device__ __forceinline__ uint64_t rank(uint64_t q) const {
        const uint64_t w = q >> 6;
        if (w >= W) return coff[W];
        return coff[w] + uint64_t(__popcll(mask[w] & ((uint64_t(1) << (q & 63)) - 1)));
    }
    __device__ __forceinline__ bool at(uint64_t q) const { return q < L && ((mask[q >> 6] >> (q & 63)) & 1); }
};

// The segment that holds position p (soff[0] <= p < L): the last one that
// starts at or before p, which skips the empty segments in front of it.
__device__ __forceinline__ uint64_t segment_of(const uint64_t* __restrict__ soff, uint64_t Se, uint64_t p) {
    return Se == 1 ? 0 : last_at_most(soff, uint64_t(0), Se + 1, p);
}

__global__ __launch_bounds__(kBlock) void k_frame_mark(const uint8_t* __restrict__ s, uint64_t L,
                                                       const uint64_t* __restrict__ soff, uint64_t Se, Marks m,
                                                       const unsigned int* err) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[kMarkLds];
    if (*err) return;
    const uint64_t p0 = uint64_t(blockIdx.x) * kMarkTile;  // < L
    // the tile and its halo, as the aligned 16-byte words that hold one of its bytes
    const uint8_t* a = s + p0;
    const uint32_t mis = uint32_t(reinterpret_cast<uintptr_t>(a) & 15);
    const uint64_t left = L - p0;
    const uint32_t nb = uint32_t(left < kMarkTile + kHdr - 1 ? left : kMarkTile + kHdr - 1);
    const uint32_t nw = (mis + nb + 15) / 16;  // <= (15 + 4125 + 15) / 16 = 259 words = 4144 bytes <= 4 kMarkLds
    const uint4* q = reinterpret_cast<const uint4*>(a - mis);
    for (uint32_t k = threadIdx.x; k < nw; k += kBlock) reinterpret_cast<uint4*>(lds)[k] = q[k];
    __syncthreads();
    const uint64_t first = soff[0];
#pragma unroll 1
    for (uint32_t it = 0; it < kMarkTile / kBlock; ++it) {
        const uint32_t lp = it * kBlock + threadIdx.x;
        const uint64_t p = p0 + lp;
        bool ok = false;
        if (p >= first && p < L && L - p >= kHdr) {
            // KeySize and ValueSize from bytes 14 .. 29 of the header, at any alignment
            const uint32_t at = mis + lp + kAtKeySize, d = at >> 2, bs = at & 3;  // d + 4 <= 1035 < kMarkLds
            const uint32_t w0 = lds[d], w1 = lds[d + 1], w2 = lds[d + 2], w3 = lds[d + 3], w4 = lds[d + 4];
            const uint64_t ks = uint64_t(__builtin_amdgcn_alignbyte(w1, w0, bs)) |
                                uint64_t(__builtin_amdgcn_alignbyte(w2, w1, bs)) << 32;
            const uint64_t vs = uint64_t(__builtin_amdgcn_alignbyte(w3, w2, bs)) |
                                uint64_t(__builtin_amdgcn_alignbyte(w4, w3, bs)) << 32;
            uint64_t room = L - p - kHdr;
            if (ks <= room && vs <= room - ks) {  // fits the stream: now the segment
                const uint64_t e = soff[segment_of(soff, Se, p) + 1];
                room = e - p;  // > 0
                ok = room >= kHdr && ks <= room - kHdr && vs <= room - kHdr - ks;
            }
        }
        const uint64_t bits = __ballot(ok);
        const uint64_t w = (p0 >> 6) + it * (kBlock / 64) + (threadIdx.x >> 6);
        if ((threadIdx.x & 63) == 0 && w < m.W) {
            m.mask[w] = bits;
            m.cnt[w] = uint64_t(__popcll(bits));
        }
    }
}

// coff[W] = M, and M next to the error word for the host
__global__ void k_frame_total(Marks m, uint64_t* __restrict__ total, const unsigned int* err) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const uint64_t M = *err ? 0 : m.coff[m.W - 1] + m.cnt[m.W - 1];
    m.coff[m.W] = M;
    *total = M;
}

__global__ __launch_bounds__(kBlock) void k_frame_pos(Marks m, uint64_t* __restrict__ pos) {
    const uint64_t w = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (w >= m.W) return;
    uint64_t bits = m.mask[w], v = m.coff[w];
    while (bits) {
        pos[v++] = 64 * w + uint64_t(__builtin_ctzll(bits));
        bits &= bits - 1;
    }
}

// Where the record at node v ends, and the segment that holds it.
__device__ __forceinline__ uint64_t node_end(const uint8_t* __restrict__ s, uint64_t L, uint64_t p) {
    uint64_t ks = 0, vs = 0;
    (void)record_span_in(s, L, p, &ks, &vs);  // holds: p is a node
    return p + kHdr + ks + vs;
}

__global__ __launch_bounds__(kBlock) void k_frame_succ(const uint8_t* __restrict__ s,
                                                       const uint64_t* __restrict__ soff, uint64_t Se, Marks m,
                                                       const uint64_t* __restrict__ pos, uint32_t M,
                                                       uint32_t* __restrict__ jump) {
    const uint64_t v = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (v >= M) return;
    const uint64_t p = pos[v];
    const uint64_t e = soff[segment_of(soff, Se, p) + 1];
    const uint64_t q = node_end(s, m.L, p);  // <= e
    jump[v] = q < e && m.at(q) ? uint32_t(m.rank(q)) : uint32_t(v);
}

// Per segment: mark its start if that is a node; if not, it holds no record,
// and a non-empty one is all tail.
__global__ __launch_bounds__(kBlock) void k_frame_starts(const uint64_t* __restrict__ soff, uint64_t Se, Marks m,
                                                         uint8_t* __restrict__ mark, uint64_t* __restrict__ seglen,
                                                         unsigned long long* stats) {
    const uint64_t j = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (j >= Se) return;
    const uint64_t a = soff[j], e = soff[j + 1];
    seglen[j] = 0;
    if (a == e) return;
    if (m.at(a)) mark[m.rank(a)] = 1;
    else note_segment(stats, j, 0, 0, true);
}

__global__ __launch_bounds__(kBlock) void k_frame_round(const uint32_t* __restrict__ jin, uint32_t* __restrict__ jout,
                                                        uint8_t* mark, uint32_t M) {
    const uint64_t v = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (v >= M) return;
    const uint32_t j = jin[v];
    if (mark[v] && j != v) mark[j] = 1;
    jout[v] = jin[j];
}

// flag[v] = mark[v] for the scan, a zero appended so that flag[M] becomes n
__global__ __launch_bounds__(kBlock) void k_frame_flags(const uint8_t* __restrict__ mark, uint32_t M,
                                                        uint32_t* __restrict__ flag) {
    const uint64_t v = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (v > M) return;
    flag[v] = v < M ? mark[v] : 0u;
}

// The last record of every segment that has one: a marked node whose successor
// is no node of the segment.  It gives the segment's bytes of whole records and
// its tail.  Lane 0 adds n.
__global__ __launch_bounds__(kBlock) void k_frame_last(const uint8_t* __restrict__ s,
                                                       const uint64_t* __restrict__ soff, uint64_t Se, Marks m,
                                                       const uint64_t* __restrict__ pos, uint32_t M,
                                                       const uint8_t* __restrict__ mark,
                                                       const uint32_t* __restrict__ rank, uint64_t* __restrict__ seglen,
                                                       unsigned long long* stats) {
    const uint64_t v = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (v == 0) atomicAdd(&stats[0], (unsigned long long)rank[M]);
    if (v >= M || !mark[v]) return;
    const uint64_t p = pos[v];
    const uint64_t j = segment_of(soff, Se, p);
    const uint64_t a = soff[j], e = soff[j + 1];
    const uint64_t q = node_end(s, m.L, p);
    if (q < e && m.at(q)) return;
    seglen[j] = q - a;
    note_segment(stats, j, 0, q - a, q != e);
}

__global__ __launch_bounds__(kBlock) void k_frame_compact(const uint64_t* __restrict__ pos, uint32_t M,
                                                          const uint8_t* __restrict__ mark,
                                                          const uint32_t* __restrict__ rank,
                                                          uint64_t* __restrict__ rec_off) {
    const uint64_t v = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (v < M && mark[v]) rec_off[rank[v]] = pos[v];
}

// first[j] = the records in front of segment j = the marked nodes in front of its start
__global__ __launch_bounds__(kBlock) void k_frame_first(const uint64_t* __restrict__ soff, uint64_t Se, Marks m,
                                                        const uint32_t* __restrict__ rank,
                                                        uint64_t* __restrict__ first) {
    const uint64_t j = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (j < Se) first[j] = rank[m.rank(soff[j])];
}

// the host form's sizes: TotalSize of the record at each offset
__global__ __launch_bounds__(kBlock) void k_frame_sizes(const uint8_t* __restrict__ s, uint64_t L,
                                                        const uint64_t* __restrict__ off, uint64_t n,
                                                        uint64_t* __restrict__ size) {
    const uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (i < n) size[i] = node_end(s, L, off[i]) - off[i];
}

template <class... A, class... B>
hipError_t launch(void (*k)(A...), uint64_t lanes, hipStream_t s, B... args) {
    hipLaunchKernelGGL(k, dim3(blocks_for(lanes)), dim3(kBlock), 0, s, args...);
    return hipGetLastError();
}

struct Frame {  // one call
    const uint8_t* s;
    uint64_t L;
    uint64_t Se;  // segments walked: S, or 1 for S == 0
    // in d_stmp: the checked offsets, per-segment counts / first records / bytes
    uint64_t *soff, *cnt, *first, *seglen;
    unsigned int* err;          // d_stats: [err | pad | M | stats[4]]
    uint64_t* total;
    unsigned long long* stats;
};

uint64_t marks_bytes(uint64_t W) { return 8 * (3 * W + 1); }
uint64_t nodes_bytes(uint64_t M) {
    return 8 * M + 4 * (M + 1) + 4 * M + M + 4 * scan_sums_words(M + 1) + 64;
}

// err = 0, M = 0, stats = {0, 0, 0, UINT64_MAX}
int reset_stats(nkv_ctx* c, const Frame& f) {
    HIPTRY(hipMemsetAsync(f.err, 0, 40, c->stream));
    return st(hipMemsetAsync(f.stats + 3, 0xFF, 8, c->stream));
}

// The verdict of k_frame_segs, M and the stats: the call's read of the counts.
int read_counts(nkv_ctx* c, const Frame& f, uint64_t h[6]) {
    HIPTRY(hipMemcpyAsync(h, f.err, 48, hipMemcpyDeviceToHost, c->stream));
    return st(hipStreamSynchronize(c->stream));
}

struct Nodes {  // the speculative path's scratch: the marks in d_aux, the rest in d_frame
    Marks m;
    uint64_t* pos;             // M positions, ascending
    uint32_t *ja, *jb, *sums;  // the two jump buffers (ja: M + 1, the marks' ranks in the end), the scan's sums
    uint8_t* mark;
    uint32_t M;
};

// The speculative path up to the stats.  *taken = false: the marks or the nodes
// do not fit the budget, or there is no node; the stats were not touched.
int speculate(nkv_ctx* c, const Frame& f, uint64_t budget, Nodes* nd, bool* taken) {
    *taken = false;
    const uint64_t W = (f.L + 63) / 64, tiles = (f.L + kMarkTile - 1) / kMarkTile;
    if (W > kMaxN || tiles > kMaxN || marks_bytes(W) > budget) return NKV_OK;
    Marks& m = nd->m;
    TRY(grow(c->d_aux, marks_bytes(W)));
    Carver k(c->d_aux.p);
    m.mask = k.take<uint64_t>(W);
    m.cnt = k.take<uint64_t>(W);
    m.coff = k.take<uint64_t>(W + 1);
    m.W = W;
    m.L = f.L;
    size_t tb = 0;
    HIPTRY(scan_exclusive_u64(m.cnt, m.coff, W, nullptr, &tb, c->stream));
    TRY(grow(c->d_tmp, tb));
    hipLaunchKernelGGL(k_frame_mark, dim3(unsigned(tiles)), dim3(kBlock), 0, c->stream, f.s, f.L, f.soff, f.Se, m,
                       f.err);
    HIPTRY(hipGetLastError());
    HIPTRY(scan_exclusive_u64(m.cnt, m.coff, W, c->d_tmp.p, &tb, c->stream));
    hipLaunchKernelGGL(k_frame_total, dim3(1), dim3(1), 0, c->stream, m, f.total, f.err);
    HIPTRY(hipGetLastError());
    uint64_t h[6];
    TRY(read_counts(c, f, h));  // the host sizes the workspace by M
    const uint64_t M = h[1];
    if (uint32_t(h[0]) || M == 0 || M > kMaxN || nodes_bytes(M) > budget - marks_bytes(W)) return NKV_OK;
    TRY(grow(c->d_frame, nodes_bytes(M)));
    Carver kn(c->d_frame.p);
    nd->pos = kn.take<uint64_t>(M);
    nd->ja = kn.take<uint32_t>(M + 1);
    nd->jb = kn.take<uint32_t>(M);
    nd->sums = kn.take<uint32_t>(scan_sums_words(M + 1));
    nd->mark = kn.take<uint8_t>(M);
    nd->M = uint32_t(M);
    HIPTRY(launch(k_frame_pos, W, c->stream, m, nd->pos));
    HIPTRY(launch(k_frame_succ, M, c->stream, f.s, f.soff, f.Se, m, nd->pos, nd->M, nd->ja));
    TRY(mark(c, 1));
    HIPTRY(hipMemsetAsync(nd->mark, 0, M, c->stream));
    HIPTRY(launch(k_frame_starts, f.Se, c->stream, f.soff, f.Se, m, nd->mark, f.seglen, f.stats));
    uint32_t *jin = nd->ja, *jout = nd->jb;
    for (uint64_t reach = 1; reach < M + 1; reach *= 2) {  // ceil(log2(M + 1)) rounds
        HIPTRY(launch(k_frame_round, M, c->stream, jin, jout, nd->mark, nd->M));
        std::swap(jin, jout);
    }
    // the jumps are done with: ja holds the marks' ranks from here on
    HIPTRY(launch(k_frame_flags, M + 1, c->stream, nd->mark, nd->M, nd->ja));
    HIPTRY(scan_exclusive_u32(nd->ja, M + 1, nd->sums, c->stream));
    HIPTRY(launch(k_frame_last, M, c->stream, f.s, f.soff, f.Se, m, nd->pos, nd->M, nd->mark, nd->ja, f.seglen,
                  f.stats));
    *taken = true;
    return NKV_OK;
}

uint64_t auto_budget(uint64_t L) {
    size_t fr = 0, tot = 0;
    if (hipMemGetInfo(&fr, &tot) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    const uint64_t twice = L > kNone / 2 ? kNone : 2 * L;
    return std::min<uint64_t>(twice, fr / 4);
}

// own: the offsets go to the context's d_off, seg_first / seg_len to d_len
// (S + 1 entries, then S), grown once n is known, instead of the caller's.
int frame(nkv_ctx* c, const uint8_t* d_stream, uint64_t L, const uint64_t* d_seg_off, uint64_t S, int flags,
          uint64_t* d_rec_off, uint64_t rec_cap, uint64_t* d_seg_first, uint64_t* d_seg_len, bool own, bool query,
          uint64_t* n_out, uint64_t stats[4]) {
    if ((!d_stream && L) || (S && !d_seg_off) || S > kMaxN) return NKV_ERR_INVALID;
    Frame f{};
    f.s = d_stream;
    f.L = L;
    f.Se = S ? S : 1;
    const auto carve = [&](Carver k) {
        f.soff = k.take<uint64_t>(f.Se + 1);
        f.cnt = k.take<uint64_t>(f.Se);
        f.first = k.take<uint64_t>(f.Se);
        f.seglen = k.take<uint64_t>(f.Se);
        return k.bytes();
    };
    TRY(grow(c->d_stmp, carve(Carver())));
    carve(Carver(c->d_stmp.p));
    TRY(grow(c->d_stats, 48));
    f.err = static_cast<unsigned int*>(c->d_stats.p);
    f.total = static_cast<uint64_t*>(c->d_stats.p) + 1;
    f.stats = static_cast<unsigned long long*>(c->d_stats.p) + 2;
    size_t tb = 0;
    HIPTRY(scan_exclusive_u64(f.cnt, f.first, f.Se, nullptr, &tb, c->stream));
    TRY(grow(c->d_tmp, tb));

    // with NKV_TIMING_EVENTS: "leaf" = mark, scans and successor (walk: count
    // and scan), "reduce" = the rounds and the compaction (walk: the write pass)
    TRY(mark(c, 0));
    TRY(reset_stats(c, f));
    HIPTRY(launch(k_frame_segs, f.Se + 1, c->stream, d_seg_off, S, L, f.soff, f.err));

    bool spec = false;
    Nodes nd{};
    if (L && c->frame_path != 1 && (c->frame_path == 2 || L / f.Se >= kAutoMeanSegment)) {
        const uint64_t budget = c->frame_budget ? c->frame_budget : auto_budget(L);
        TRY(speculate(c, f, budget, &nd, &spec));
    }
    if (!spec) {
        HIPTRY(launch(k_walk_count, f.Se, c->stream, f.s, f.soff, f.Se, f.cnt, f.seglen, f.stats, f.err));
        HIPTRY(scan_exclusive_u64(f.cnt, f.first, f.Se, c->d_tmp.p, &tb, c->stream));
        TRY(mark(c, 1));
    }
    uint64_t h[6];
    TRY(read_counts(c, f, h));
    const auto refuse = [&]() {
        TRY(mark(c, 2));
        return int(NKV_ERR_INVALID);
    };
    if (uint32_t(h[0])) return refuse();  // the segment offsets
    const uint64_t n = h[2];
    *n_out = n;
    for (int i = 0; i < 4; ++i) stats[i] = h[2 + i];
    c->last_path = spec ? NKV_PATH_FRAME_SPECULATIVE : NKV_PATH_FRAME_WALK;
    if (n > kMaxN || ((flags & NKV_FRAME_STRICT) && h[4])) return refuse();
    if (query) return mark(c, 2);
    if (rec_cap < n) return refuse();
    if (own) {
        TRY(grow(c->d_off, 8 * n));
        TRY(grow(c->d_len, 8 * (2 * S + 1)));
        d_rec_off = static_cast<uint64_t*>(c->d_off.p);
        d_seg_first = static_cast<uint64_t*>(c->d_len.p);
        d_seg_len = d_seg_first + S + 1;
    }
    if (spec) {
        HIPTRY(launch(k_frame_compact, nd.M, c->stream, nd.pos, nd.M, nd.mark, nd.ja, d_rec_off));
        if (d_seg_first) HIPTRY(launch(k_frame_first, f.Se, c->stream, f.soff, f.Se, nd.m, nd.ja, f.first));
    } else if (n) {
        HIPTRY(launch(k_walk_write, f.Se, c->stream, f.s, f.soff, f.Se, f.first, d_rec_off));
    }
    if (d_seg_first || d_seg_len)
        HIPTRY(launch(k_seg_out, S + 1, c->stream, f.first, f.seglen, S, n, d_seg_first, d_seg_len));
    return mark(c, 2);
}

}  // namespace

extern "C" {

int nkv_frame_records_dev(nkv_ctx* c, const void* d_stream, uint64_t stream_len, const uint64_t* d_seg_off,
                          uint64_t S, int flags, uint64_t* d_rec_off, uint64_t rec_cap, uint64_t* d_seg_first,
                          uint64_t* d_seg_len, uint64_t* n_out, uint64_t stats[4]) try {
    TRY(bind(c));
    if (!n_out || !stats) return NKV_ERR_INVALID;
    TRY(frame(c, static_cast<const uint8_t*>(d_stream), stream_len, d_seg_off, S, flags, d_rec_off, rec_cap,
              d_seg_first, d_seg_len, false, !d_rec_off, n_out, stats));
    return st(hipStreamSynchronize(c->stream));
} NKV_CATCH

int nkv_frame_records(nkv_ctx* c, const uint8_t* stream, uint64_t stream_len, const uint64_t* seg_off, uint64_t S,
                      int flags, uint64_t* rec_size_out, uint64_t rec_cap, uint64_t* seg_first_out,
                      uint64_t* seg_len_out, uint64_t* n_out, uint64_t stats[4]) try {
    TRY(bind(c));
    if (!n_out || !stats) return NKV_ERR_INVALID;
    if ((!stream && stream_len) || (S && !seg_off) || S > kMaxN) return NKV_ERR_INVALID;
    const uint64_t* d_seg = nullptr;
    if (stream_len) {
        TRY(grow(c->d_data, stream_len));
        HIPTRY(c->stage.upload(stream, stream_len, static_cast<uint8_t*>(c->d_data.p), c->stream));
    }
    if (S) {
        TRY(grow(c->d_perm, 8 * S));
        HIPTRY(hipMemcpyAsync(c->d_perm.p, seg_off, 8 * S, hipMemcpyHostToDevice, c->stream));
        d_seg = static_cast<const uint64_t*>(c->d_perm.p);
    }
    const uint8_t* d_stream = stream_len ? static_cast<const uint8_t*>(c->d_data.p) : nullptr;
    const bool query = !rec_size_out;
    TRY(frame(c, d_stream, stream_len, d_seg, S, flags, nullptr, rec_cap, nullptr, nullptr, true, query, n_out,
              stats));
    if (query) return NKV_OK;
    const uint64_t n = *n_out;
    if (n) {  // the offsets become sizes in place
        uint64_t* d_off = static_cast<uint64_t*>(c->d_off.p);
        HIPTRY(launch(k_frame_sizes, n, c->stream, d_stream, stream_len, d_off, n, d_off));
        HIPTRY(hipMemcpyAsync(rec_size_out, d_off, 8 * n, hipMemcpyDeviceToHost, c->stream));
    }
    const uint64_t* d_first = static_cast<const uint64_t*>(c->d_len.p);
    if (seg_first_out)
        HIPTRY(hipMemcpyAsync(seg_first_out, d_first, 8 * (S + 1), hipMemcpyDeviceToHost, c->stream));
    if (seg_len_out && S)
        HIPTRY(hipMemcpyAsync(seg_len_out, d_first + S + 1, 8 * S, hipMemcpyDeviceToHost, c->stream));
    return st(hipStreamSynchronize(c->stream));
} NKV_CATCH

}  // extern "C"
