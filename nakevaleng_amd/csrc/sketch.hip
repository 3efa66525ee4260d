// sketch.hip -- the reference's two sketches on gfx950: HyperLogLog (ds/hll)
// and Count-Min Sketch (ds/cmsketch), both per-key MurmurHash3_x86_32 loops.
//
// Reference: ds/hll/hll.go:43-62 (Add: h = murmur3 Sum32(key), seed 0; idx =
// h >> (32 - P); val = 1 + TrailingZeros32(h), 33 for h == 0; Reg[idx] =
// max(Reg[idx], val)), :75-92 (Estimate); ds/cmsketch/cmsketch.go:18-24
// (M = ceil(e / epsilon), K = ceil(ln(1 / delta))), :28-38 (row i hashes with
// seed t + i), :76-87 (Insert: Contents[i][h_i % uint32(M)] += 1, uint32, so
// it wraps), :91-111 (Query: the minimum of the K counters).
//
// One lane per key, read as bloom.hip reads it: from a span (base + off[i],
// len[i], any alignment) or from the record at base + off[i] through
// record_dev.hpp's key span (a header or key outside the stream sets the error
// word and contributes nothing).  The hash is murmur_dev.hpp's: one state for
// the HLL, passes of up to kBloomMaxK consecutive seeds for the CMS rows, the
// row index by fastmod.
//
// HLL update.  Once the registers have warmed up almost every Add is a no-op,
// so the register byte is read with a plain load and the atomic path is taken
// only when val exceeds it.  A stale read can only be too low: it costs one
// more attempt, never a wrong result.  There is no byte-wide atomic max, so
// the atomic path is a device-scope compare-and-swap loop on the containing
// dword (d_reg is 4-byte aligned and 2^P >= 16 bytes long).
// CMS update: one no-return device-scope atomicAdd per (key, row).
//
// Two tiers (NKV_OPT_SKETCH_PATH: 0 auto, 1 direct, 2 LDS).
//   direct  one lane per key straight onto the caller's buffer.
//   LDS     a persistent grid strides over the keys; each workgroup keeps a
//           private copy in LDS -- the whole register file (2^P <= 64 KiB), or
//           the K x M table when K M <= 16384 counters, replicated per wave
//           while copies fit (the reference's 28 x 3 gets one copy per wave
//           instead of 256 lanes on 84 counters) -- and merges it into the
//           caller's buffer once at the end: only register bytes that exceed
//           the current value, only non-zero counters.  A table that does not
//           fit LDS takes the direct tier whatever the option says.
// Max and wrapping add commute, so the output is byte-identical for every
// tier, grid size and split of the keys over calls.
//
// Deviations from the reference.  cmsketch.New accepts epsilon = 0, delta = 0
// and delta = 1, which give +Inf conversions or K = 0; nkv_cms_params returns
// NKV_ERR_INVALID unless 0 < epsilon <= 1, 0 < delta < 1 and M <= 2^32 - 1, and
// the insert and query entries need M >= 1, K >= 1 and K M <= 2^31 - 1.  The gob
// encodings (EncodeToBytes / DecodeFromBytes) are host serialization and out of
// scope.  nkv_hll_estimate mode 0 is hll.go:75-92 taken literally, quirk
// included: float64(-val) of a uint8 is 256 - val, so the "harmonic" sum adds
// (256 - val)^2 per non-empty register, and the result is linear counting while
// empty registers remain and a meaningless small number after that; mode 1 sums
// 2^-val with the same alpha and corrections.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <cmath>

#include "context.hpp"
#include "murmur_dev.hpp"  // mm_states, mm_fmix, fastmod_u32, kBloomMaxK

using namespace nkv;

namespace {

constexpr int kSkBlock = 256;
constexpr uint32_t kSkLdsWords = 16384;  // 64 KiB of dynamic LDS per workgroup
constexpr uint32_t kSkWaves = kSkBlock / 64;

// key i: pointer and length (MODE 1: the record's key, span checked)
template <int MODE>
__device__ __forceinline__ bool sketch_key(const uint8_t* base, const uint64_t* off, const uint64_t* len,
                                           uint64_t stream_len, uint64_t i, const uint8_t** key, uint64_t* L) {
    if (MODE == 0) {
        *key = base + off[i];
        *L = len[i];
        return true;
    }
    const uint64_t r = off[i];
    uint64_t ks;
    if (!key_span_in(base, stream_len, r, &ks)) return false;
    *key = base + r + kHdr;
    *L = ks;
    return true;
}

// hll.go:49-55: the register and the value of one key
__device__ __forceinline__ void hll_hash(const uint8_t* key, uint64_t L, int p, uint32_t* idx, uint32_t* val) {
    uint32_t h[kBloomMaxK];
    mm_states(key, L, 0u, 1, h);
    const uint32_t hv = mm_fmix(h[0] ^ uint32_t(L));
    *idx = hv >> (32 - p);
    *val = hv ? 1u + uint32_t(__builtin_ctz(hv)) : 33u;  // TrailingZeros32(0) = 32
}

// reg[idx] = max(reg[idx], val) on bytes inside 32-bit words (global or LDS)
__device__ __forceinline__ void reg_max(uint32_t* words, uint32_t idx, uint32_t val) {
    if (reinterpret_cast<const uint8_t*>(words)[idx] >= val) return;  // plain load: stale = too low = one more try
    uint32_t* w = words + (idx >> 2);
    const uint32_t sh = (idx & 3u) * 8u;
    uint32_t old = *w;
    while (((old >> sh) & 0xFFu) < val) {
        const uint32_t prev = atomicCAS(w, old, (old & ~(0xFFu << sh)) | (val << sh));
        if (prev == old) break;
        old = prev;
    }
}

__device__ __forceinline__ uint32_t bytes_max(uint32_t a, uint32_t b) {
    uint32_t r = 0;
#pragma unroll
    for (int s = 0; s < 32; s += 8) r |= max((a >> s) & 0xFFu, (b >> s) & 0xFFu) << s;
    return r;
}

template <int MODE>
__global__ __launch_bounds__(kSkBlock) void k_hll_direct(const uint8_t* __restrict__ base,
                                                         const uint64_t* __restrict__ off,
                                                         const uint64_t* __restrict__ len, uint64_t stream_len,
                                                         uint64_t n, int p, uint32_t* reg, unsigned int* err) {
    const uint64_t i = uint64_t(blockIdx.x) * kSkBlock + threadIdx.x;
    if (i >= n) return;
    const uint8_t* key;
    uint64_t L;
    if (!sketch_key<MODE>(base, off, len, stream_len, i, &key, &L)) {
        atomicOr(err, 1u);
        return;
    }
    uint32_t idx, val;
    hll_hash(key, L, p, &idx, &val);
    reg_max(reg, idx, val);
}

template <int MODE>
__global__ __launch_bounds__(kSkBlock) void k_hll_lds(const uint8_t* __restrict__ base,
                                                      const uint64_t* __restrict__ off,
                                                      const uint64_t* __restrict__ len, uint64_t stream_len,
                                                      uint64_t n, int p, uint32_t* reg, unsigned int* err) {
    extern __shared__ uint32_t lds[];
    const uint32_t words = (1u << p) >> 2;
    for (uint32_t t = threadIdx.x; t < words; t += kSkBlock) lds[t] = 0u;
    __syncthreads();
    const uint64_t step = uint64_t(gridDim.x) * kSkBlock;
    for (uint64_t i = uint64_t(blockIdx.x) * kSkBlock + threadIdx.x; i < n; i += step) {
        const uint8_t* key;
        uint64_t L;
        if (!sketch_key<MODE>(base, off, len, stream_len, i, &key, &L)) {
            atomicOr(err, 1u);
            continue;
        }
        uint32_t idx, val;
        hll_hash(key, L, p, &idx, &val);
        reg_max(lds, idx, val);
    }
    __syncthreads();
    // merge: only the words with a byte above the caller's current value
    for (uint32_t t = threadIdx.x; t < words; t += kSkBlock) {
        const uint32_t mine = lds[t];
        if (!mine) continue;
        uint32_t old = reg[t];
        for (;;) {
            const uint32_t nw = bytes_max(old, mine);
            if (nw == old) break;
            const uint32_t prev = atomicCAS(reg + t, old, nw);
            if (prev == old) break;
            old = prev;
        }
    }
}

// fn(row, idx) for the k counters of one key
template <class F>
__device__ __forceinline__ void cms_rows(const uint8_t* key, uint64_t L, uint32_t m, uint64_t M, uint32_t k,
                                         uint32_t seed0, F fn) {
    for (uint32_t j0 = 0; j0 < k; j0 += kBloomMaxK) {
        const int nk = int(min(k - j0, uint32_t(kBloomMaxK)));
        uint32_t h[kBloomMaxK];
        mm_states(key, L, seed0 + j0, nk, h);
#pragma unroll
        for (int j = 0; j < kBloomMaxK; ++j)
            if (j < nk) fn(j0 + uint32_t(j), fastmod_u32(mm_fmix(h[j] ^ uint32_t(L)), M, m));
    }
}

template <int MODE>
__global__ __launch_bounds__(kSkBlock) void k_cms_direct(const uint8_t* __restrict__ base,
                                                         const uint64_t* __restrict__ off,
                                                         const uint64_t* __restrict__ len, uint64_t stream_len,
                                                         uint64_t n, uint32_t m, uint64_t M, uint32_t k,
                                                         uint32_t seed0, uint32_t* table, unsigned int* err) {
    const uint64_t i = uint64_t(blockIdx.x) * kSkBlock + threadIdx.x;
    if (i >= n) return;
    const uint8_t* key;
    uint64_t L;
    if (!sketch_key<MODE>(base, off, len, stream_len, i, &key, &L)) {
        atomicOr(err, 1u);
        return;
    }
    cms_rows(key, L, m, M, k, seed0, [&](uint32_t row, uint32_t idx) { atomicAdd(table + (row * m + idx), 1u); });
}

// copies private tables of k * m counters per workgroup, wave w on copy w % copies
template <int MODE>
__global__ __launch_bounds__(kSkBlock) void k_cms_lds(const uint8_t* __restrict__ base,
                                                      const uint64_t* __restrict__ off,
                                                      const uint64_t* __restrict__ len, uint64_t stream_len,
                                                      uint64_t n, uint32_t m, uint64_t M, uint32_t k, uint32_t seed0,
                                                      uint32_t copies, uint32_t* table, unsigned int* err) {
    extern __shared__ uint32_t lds[];
    const uint32_t T = k * m;
    for (uint32_t t = threadIdx.x; t < copies * T; t += kSkBlock) lds[t] = 0u;
    __syncthreads();
    uint32_t* mine = lds + ((threadIdx.x >> 6) % copies) * T;
    const uint64_t step = uint64_t(gridDim.x) * kSkBlock;
    for (uint64_t i = uint64_t(blockIdx.x) * kSkBlock + threadIdx.x; i < n; i += step) {
        const uint8_t* key;
        uint64_t L;
        if (!sketch_key<MODE>(base, off, len, stream_len, i, &key, &L)) {
            atomicOr(err, 1u);
            continue;
        }
        cms_rows(key, L, m, M, k, seed0, [&](uint32_t row, uint32_t idx) { atomicAdd(mine + (row * m + idx), 1u); });
    }
    __syncthreads();
    for (uint32_t t = threadIdx.x; t < T; t += kSkBlock) {
        uint32_t s = 0;
        for (uint32_t c = 0; c < copies; ++c) s += lds[c * T + t];
        if (s) atomicAdd(table + t, s);
    }
}

__global__ __launch_bounds__(kSkBlock) void k_cms_query(const uint8_t* __restrict__ base,
                                                        const uint64_t* __restrict__ off,
                                                        const uint64_t* __restrict__ len, uint64_t n, uint32_t m,
                                                        uint64_t M, uint32_t k, uint32_t seed0,
                                                        const uint32_t* __restrict__ table,
                                                        uint32_t* __restrict__ out) {
    const uint64_t i = uint64_t(blockIdx.x) * kSkBlock + threadIdx.x;
    if (i >= n) return;
    uint32_t lo = 0xFFFFFFFFu;  // cmsketch.go:103-107: the first row's counter, then the minimum
    cms_rows(base + off[i], len[i], m, M, k, seed0,
             [&](uint32_t row, uint32_t idx) { lo = min(lo, table[row * m + idx]); });
    out[i] = lo;
}

uint32_t tiles_of(uint64_t n) { return uint32_t((n + kSkBlock - 1) / kSkBlock); }

// Workgroups of a persistent launch: as many per CU as their LDS copies allow
// (up to 4), and never more than there are tiles of keys.
uint32_t persistent_grid(const nkv_ctx* c, uint64_t n, uint32_t lds_bytes) {
    const uint32_t cus = std::max(1u, c->simds / 4);
    const uint32_t per_cu = std::max(1u, std::min(4u, (kSkLdsWords * 4u) / std::max(lds_bytes, 1u)));
    return std::max(1u, std::min(tiles_of(n), cus * per_cu));
}

// Tier of an HLL add.  Measured ("Sketches"): up to 2^12
// registers the direct tier's compare-and-swaps pile up on a few hundred
// dwords while the registers rise, and the LDS tier wins (4 Ki..16 Mi keys:
// 10-85 x at P = 4, 1.5-6.8 x at P = 10, 1.3-2 x at P = 12 from 256 Ki keys on);
// at P = 13 the tiers are level, and at P = 14 and 16 the merge of 2^P / 4 words
// per workgroup costs more than it saves.
constexpr int kHllLdsMaxP = 12;

bool hll_takes_lds(const nkv_ctx* c, int p) {
    if (c->sketch_path == 1) return false;
    if (c->sketch_path == 2) return true;
    return p <= kHllLdsMaxP;
}

// LDS copies of a K x M table per workgroup; 0 = the direct tier.  Measured
// (DESIGN.md section 4): a table that fits takes the LDS tier from about four
// keys per counter on (28 x 3: 3.6 x at 4 Ki keys, 124 x at 1 Mi; 2719 x 5:
// 0.8 x at 32 Ki, 2.1 x at 256 Ki, 4.1 x at 1 Mi).
constexpr uint64_t kCmsLdsKeysPerCounter = 4;

uint32_t cms_lds_copies(const nkv_ctx* c, uint64_t n, uint32_t m, uint32_t k) {
    const uint64_t T = uint64_t(m) * k;
    if (c->sketch_path == 1 || T > kSkLdsWords) return 0;
    const uint32_t copies = std::min(kSkWaves, uint32_t(kSkLdsWords / T));
    if (c->sketch_path == 2) return copies;
    return n >= kCmsLdsKeysPerCounter * T ? copies : 0;
}

int hll_add(nkv_ctx* c, int mode, const uint8_t* base, const uint64_t* off, const uint64_t* len, uint64_t stream_len,
            uint64_t n, int p, uint32_t* reg, unsigned int* err) {
    const dim3 block(kSkBlock);
    if (hll_takes_lds(c, p)) {
        const uint32_t bytes = 1u << p;
        const dim3 grid(persistent_grid(c, n, bytes));
        if (mode == 0)
            hipLaunchKernelGGL(k_hll_lds<0>, grid, block, bytes, c->stream, base, off, len, stream_len, n, p, reg, err);
        else
            hipLaunchKernelGGL(k_hll_lds<1>, grid, block, bytes, c->stream, base, off, len, stream_len, n, p, reg, err);
    } else {
        const dim3 grid(tiles_of(n));
        if (mode == 0)
            hipLaunchKernelGGL(k_hll_direct<0>, grid, block, 0, c->stream, base, off, len, stream_len, n, p, reg, err);
        else
            hipLaunchKernelGGL(k_hll_direct<1>, grid, block, 0, c->stream, base, off, len, stream_len, n, p, reg, err);
    }
    return st(hipGetLastError());
}

int cms_insert(nkv_ctx* c, int mode, const uint8_t* base, const uint64_t* off, const uint64_t* len,
               uint64_t stream_len, uint64_t n, uint32_t m, uint32_t k, uint32_t seed0, uint32_t* table,
               unsigned int* err) {
    const dim3 block(kSkBlock);
    const uint64_t M = fastmod_magic(m);
    const uint32_t copies = cms_lds_copies(c, n, m, k);
    if (copies) {
        const uint32_t bytes = copies * m * k * 4u;
        const dim3 grid(persistent_grid(c, n, bytes));
        if (mode == 0)
            hipLaunchKernelGGL(k_cms_lds<0>, grid, block, bytes, c->stream, base, off, len, stream_len, n, m, M, k,
                               seed0, copies, table, err);
        else
            hipLaunchKernelGGL(k_cms_lds<1>, grid, block, bytes, c->stream, base, off, len, stream_len, n, m, M, k,
                               seed0, copies, table, err);
    } else {
        const dim3 grid(tiles_of(n));
        if (mode == 0)
            hipLaunchKernelGGL(k_cms_direct<0>, grid, block, 0, c->stream, base, off, len, stream_len, n, m, M, k,
                               seed0, table, err);
        else
            hipLaunchKernelGGL(k_cms_direct<1>, grid, block, 0, c->stream, base, off, len, stream_len, n, m, M, k,
                               seed0, table, err);
    }
    return st(hipGetLastError());
}

bool hll_p_ok(int p) { return p >= NKV_HLL_MIN_PRECISION && p <= NKV_HLL_MAX_PRECISION; }
bool cms_shape_ok(uint32_t m, uint32_t k) { return m >= 1 && k >= 1 && uint64_t(m) * k <= 0x7FFFFFFFull; }

// the caller's register file or table to d_img and, after the work, back
int image_in(nkv_ctx* c, const void* host, uint64_t bytes) {
    TRY(grow(c->d_img, bytes));
    return st(c->stage.upload(static_cast<const uint8_t*>(host), bytes, static_cast<uint8_t*>(c->d_img.p), c->stream));
}

int image_out(nkv_ctx* c, void* host, uint64_t bytes) {
    HIPTRY(c->stage.download(static_cast<uint8_t*>(host), static_cast<const uint8_t*>(c->d_img.p), bytes, c->stream));
    return st(hipStreamSynchronize(c->stream));
}

}  // namespace

// ---------------------------------------------------------------------------
// C-ABI: device forms

int nkv_hll_add_dev(nkv_ctx* c, const void* d_keys, const uint64_t* d_off, const uint64_t* d_len, uint64_t n, int p,
                    void* d_reg) try {
    TRY(bind(c));
    if (n > kMaxN || !hll_p_ok(p) || !d_reg) return NKV_ERR_INVALID;
    if (n == 0) return NKV_OK;
    if (!d_keys || !d_off || !d_len) return NKV_ERR_INVALID;
    return hll_add(c, 0, static_cast<const uint8_t*>(d_keys), d_off, d_len, 0, n, p, static_cast<uint32_t*>(d_reg),
                   nullptr);
} NKV_CATCH

int nkv_hll_add_records_dev(nkv_ctx* c, const void* d_stream, uint64_t stream_len, const uint64_t* d_rec_off,
                            uint64_t n, int p, void* d_reg) try {
    TRY(bind(c));
    if (n > kMaxN || !hll_p_ok(p) || !d_reg) return NKV_ERR_INVALID;
    if (n == 0) return NKV_OK;
    if (!d_stream || !d_rec_off) return NKV_ERR_INVALID;
    TRY(grow(c->d_err, 4));
    unsigned int* err = static_cast<unsigned int*>(c->d_err.p);
    HIPTRY(hipMemsetAsync(err, 0, 4, c->stream));
    TRY(hll_add(c, 1, static_cast<const uint8_t*>(d_stream), d_rec_off, nullptr, stream_len, n, p,
                static_cast<uint32_t*>(d_reg), err));
    return read_verdict(c, err);
} NKV_CATCH

int nkv_cms_insert_dev(nkv_ctx* c, const void* d_keys, const uint64_t* d_off, const uint64_t* d_len, uint64_t n,
                       uint32_t m, uint32_t k, uint32_t seed0, uint32_t* d_table) try {
    TRY(bind(c));
    if (n > kMaxN || !cms_shape_ok(m, k) || !d_table) return NKV_ERR_INVALID;
    if (n == 0) return NKV_OK;
    if (!d_keys || !d_off || !d_len) return NKV_ERR_INVALID;
    return cms_insert(c, 0, static_cast<const uint8_t*>(d_keys), d_off, d_len, 0, n, m, k, seed0, d_table, nullptr);
} NKV_CATCH

int nkv_cms_insert_records_dev(nkv_ctx* c, const void* d_stream, uint64_t stream_len, const uint64_t* d_rec_off,
                               uint64_t n, uint32_t m, uint32_t k, uint32_t seed0, uint32_t* d_table) try {
    TRY(bind(c));
    if (n > kMaxN || !cms_shape_ok(m, k) || !d_table) return NKV_ERR_INVALID;
    if (n == 0) return NKV_OK;
    if (!d_stream || !d_rec_off) return NKV_ERR_INVALID;
    TRY(grow(c->d_err, 4));
    unsigned int* err = static_cast<unsigned int*>(c->d_err.p);
    HIPTRY(hipMemsetAsync(err, 0, 4, c->stream));
    TRY(cms_insert(c, 1, static_cast<const uint8_t*>(d_stream), d_rec_off, nullptr, stream_len, n, m, k, seed0,
                   d_table, err));
    return read_verdict(c, err);
} NKV_CATCH

int nkv_cms_query_dev(nkv_ctx* c, const void* d_keys, const uint64_t* d_off, const uint64_t* d_len, uint64_t n,
                      uint32_t m, uint32_t k, uint32_t seed0, const uint32_t* d_table, uint32_t* d_out) try {
    TRY(bind(c));
    if (n > kMaxN || !cms_shape_ok(m, k) || !d_table) return NKV_ERR_INVALID;
    if (n == 0) return NKV_OK;
    if (!d_keys || !d_off || !d_len || !d_out) return NKV_ERR_INVALID;
    hipLaunchKernelGGL(k_cms_query, dim3(tiles_of(n)), dim3(kSkBlock), 0, c->stream,
                       static_cast<const uint8_t*>(d_keys), d_off, d_len, n, m, fastmod_magic(m), k, seed0, d_table,
                       d_out);
    return st(hipGetLastError());
} NKV_CATCH

// ---------------------------------------------------------------------------
// C-ABI: host-pointer forms (synchronous)

int nkv_hll_add(nkv_ctx* c, const uint8_t* keys, const uint64_t* off, const uint64_t* len, uint64_t n, int p,
                uint8_t* reg) try {
    TRY(bind(c));
    if (n > kMaxN || !hll_p_ok(p) || !reg) return NKV_ERR_INVALID;
    if (n == 0) return NKV_OK;
    if (!keys || !off || !len) return NKV_ERR_INVALID;
    const uint64_t bytes = uint64_t(1) << p;
    TRY(image_in(c, reg, bytes));
    TRY(stage_spans(c, keys, off, len, n));
    TRY(nkv_hll_add_dev(c, c->d_data.p, static_cast<const uint64_t*>(c->d_off.p),
                        static_cast<const uint64_t*>(c->d_len.p), n, p, c->d_img.p));
    return image_out(c, reg, bytes);
} NKV_CATCH

int nkv_hll_add_records(nkv_ctx* c, const uint8_t* stream, uint64_t stream_len, const uint64_t* rec_size, uint64_t n,
                        int p, uint8_t* reg) try {
    TRY(bind(c));
    if (n > kMaxN || !hll_p_ok(p) || !reg) return NKV_ERR_INVALID;
    if (n == 0) return NKV_OK;
    if (!stream || !rec_size) return NKV_ERR_INVALID;
    const uint64_t bytes = uint64_t(1) << p;
    const uint64_t* rec_off = nullptr;
    TRY(image_in(c, reg, bytes));
    TRY(stage_records(c, stream, stream_len, rec_size, n, &rec_off));
    TRY(nkv_hll_add_records_dev(c, c->d_data.p, stream_len, rec_off, n, p, c->d_img.p));
    return image_out(c, reg, bytes);
} NKV_CATCH

int nkv_cms_insert(nkv_ctx* c, const uint8_t* keys, const uint64_t* off, const uint64_t* len, uint64_t n, uint32_t m,
                   uint32_t k, uint32_t seed0, uint32_t* table) try {
    TRY(bind(c));
    if (n > kMaxN || !cms_shape_ok(m, k) || !table) return NKV_ERR_INVALID;
    if (n == 0) return NKV_OK;
    if (!keys || !off || !len) return NKV_ERR_INVALID;
    const uint64_t bytes = 4 * uint64_t(m) * k;
    TRY(image_in(c, table, bytes));
    TRY(stage_spans(c, keys, off, len, n));
    TRY(nkv_cms_insert_dev(c, c->d_data.p, static_cast<const uint64_t*>(c->d_off.p),
                           static_cast<const uint64_t*>(c->d_len.p), n, m, k, seed0,
                           static_cast<uint32_t*>(c->d_img.p)));
    return image_out(c, table, bytes);
} NKV_CATCH

int nkv_cms_insert_records(nkv_ctx* c, const uint8_t* stream, uint64_t stream_len, const uint64_t* rec_size,
                           uint64_t n, uint32_t m, uint32_t k, uint32_t seed0, uint32_t* table) try {
    TRY(bind(c));
    if (n > kMaxN || !cms_shape_ok(m, k) || !table) return NKV_ERR_INVALID;
    if (n == 0) return NKV_OK;
    if (!stream || !rec_size) return NKV_ERR_INVALID;
    const uint64_t bytes = 4 * uint64_t(m) * k;
    const uint64_t* rec_off = nullptr;
    TRY(image_in(c, table, bytes));
    TRY(stage_records(c, stream, stream_len, rec_size, n, &rec_off));
    TRY(nkv_cms_insert_records_dev(c, c->d_data.p, stream_len, rec_off, n, m, k, seed0,
                                   static_cast<uint32_t*>(c->d_img.p)));
    return image_out(c, table, bytes);
} NKV_CATCH

int nkv_cms_query(nkv_ctx* c, const uint8_t* keys, const uint64_t* off, const uint64_t* len, uint64_t n, uint32_t m,
                  uint32_t k, uint32_t seed0, const uint32_t* table, uint32_t* out) try {
    TRY(bind(c));
    if (n > kMaxN || !cms_shape_ok(m, k) || !table) return NKV_ERR_INVALID;
    if (n == 0) return NKV_OK;
    if (!keys || !off || !len || !out) return NKV_ERR_INVALID;
    TRY(image_in(c, table, 4 * uint64_t(m) * k));
    TRY(stage_spans(c, keys, off, len, n));
    TRY(grow(c->d_nodes, 4 * n));
    TRY(nkv_cms_query_dev(c, c->d_data.p, static_cast<const uint64_t*>(c->d_off.p),
                          static_cast<const uint64_t*>(c->d_len.p), n, m, k, seed0,
                          static_cast<const uint32_t*>(c->d_img.p), static_cast<uint32_t*>(c->d_nodes.p)));
    HIPTRY(c->stage.download(reinterpret_cast<uint8_t*>(out), static_cast<const uint8_t*>(c->d_nodes.p), 4 * n,
                             c->stream));
    return st(hipStreamSynchronize(c->stream));
} NKV_CATCH

// ---------------------------------------------------------------------------
// C-ABI: pure host functions

int nkv_cms_params(double epsilon, double delta, uint32_t* m, uint32_t* k) try {
    if (!m || !k || !(epsilon > 0.0 && epsilon <= 1.0) || !(delta > 0.0 && delta < 1.0)) return NKV_ERR_INVALID;
    const double mm = std::ceil(M_E / epsilon);           // cmsketch.go:18-20
    const double kk = std::ceil(std::log(1.0 / delta));   // cmsketch.go:22-24
    if (!(mm >= 1.0 && mm <= 4294967295.0) || !(kk >= 1.0 && kk <= 4294967295.0)) return NKV_ERR_INVALID;
    *m = uint32_t(mm);
    *k = uint32_t(kk);
    return NKV_OK;
} NKV_CATCH

int nkv_hll_estimate(const uint8_t* reg, int p, int mode, double* out) try {
    if (!reg || !out || !hll_p_ok(p)) return NKV_ERR_INVALID;
    if (mode != NKV_HLL_ESTIMATE_REFERENCE && mode != NKV_HLL_ESTIMATE_STANDARD) return NKV_ERR_INVALID;
    const uint64_t M = uint64_t(1) << p;
    double sum = 0.0;
    uint64_t empty = 0;
    for (uint64_t i = 0; i < M; ++i) {
        const uint8_t val = reg[i];
        // hll.go:78: float64(-val) of a uint8 wraps modulo 256
        if (mode == NKV_HLL_ESTIMATE_REFERENCE) sum = sum + std::pow(double(uint8_t(-val)), 2.0);
        else sum = sum + std::pow(2.0, -double(val));
        empty += val == 0;
    }
    const double alpha = 0.7213 / (1.0 + 1.079 / double(M));
    double estimation = alpha * std::pow(double(M), 2.0) / sum;
    if (estimation < 2.5 * double(M)) {
        if (empty > 0) estimation = double(M) * std::log(double(M) / double(empty));
    } else if (estimation > std::pow(2.0, 32.0) / 30.0) {
        estimation = -std::pow(2.0, 32.0) * std::log(1.0 - estimation / std::pow(2.0, 32.0));
    }
    *out = estimation;
    return NKV_OK;
} NKV_CATCH
