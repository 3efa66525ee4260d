// search_dev.hpp -- the search of the get paths, once: the query, the search
// of one sorted table, the table set and the kernel that walks it, and what a
// hit answers.  lookup.hip (Data tables) and locate.hip (Index tables) each add
// an entry format and nothing else; memindex.hip, whose index is a hash, uses
// the query and the answers.
//
// The upper half is pure and compiles as plain host C++
// (tests/cpp/test_search_layer.cpp), as record_dev.hpp does.  The lower half
// (the filter test in front of the search, the kernel body, the table set) is
// for the HIP units.
//
// An entry format F says how an entry is bounds-checked and where its key lies:
//   F::key_in(img, L, o, &ks)   the entry at img + o lies in the image (key_span_in / entry_in)
//   F::kKeyAt                   bytes in front of its key
// and, for the kernel, what a FOUND entry answers:
//   F::kOverlay                 the kernel honours f.overlay (answered queries are left alone)
//   f.answer(entry, &status)    the status; false demotes the hit to stage INDEX and the search moves on
//   f.store(i)                  the format's own output for query i, beside hit and status
#pragma once
#include <stdint.h>

#include "nkv_merkle.h"
#include "record_dev.hpp"

namespace nkv {

struct Query {
    const uint8_t* key;
    uint64_t len;
    uint64_t pfx;  // first 8 key bytes, big-endian, zero-padded
};

// Query i of a batch: the klen[i] bytes at keys + koff[i].
NKV_HD inline Query query_of(const uint8_t* keys, const uint64_t* koff, const uint64_t* klen, uint64_t i) {
    Query Q;
    Q.key = keys + koff[i];
    Q.len = klen[i];
    Q.pfx = key_prefix(Q.key, Q.len);
    return Q;
}

constexpr uint64_t kNoHit = ~uint64_t(0);  // the hit word of a key no table holds

NKV_HD inline uint64_t hit_word(uint32_t table, uint64_t index) { return (uint64_t(table) << 32) | index; }

// What a found record answers: its Status byte's bit 0 is the tombstone.
NKV_HD inline uint8_t status_answer(uint8_t status_byte) {
    return (status_byte & 1) ? NKV_GET_TOMBSTONE : NKV_GET_LIVE;
}

constexpr int kBad = 2;  // probe: the entry reaches outside its image

// bytes.Compare(query, key of entry j): -1, 0, 1, or kBad.  Nothing outside
// [img, img + L) is read.
template <class F>
NKV_HD inline __attribute__((always_inline)) int probe(const Query& Q, const uint8_t* img, uint64_t L,
                                                        const uint64_t* off, uint64_t j) {
    const uint64_t o = off[j];
    uint64_t ks;
    if (!F::key_in(img, L, o, &ks)) return kBad;
    const uint8_t* k = img + o + F::kKeyAt;
    return cmp_prefixed(Q.pfx, Q.len, Q.key + 8, key_prefix(k, ks), ks, k + 8);
}

// The search of n >= 1 entries in ascending key order; at(j) is the probe of
// entry j.  The stage it ends at and, when FOUND, the entry's index: SUMMARY
// outside [K_0, K_(n-1)], else the lower bound over the interior.  A bad probe
// ends the search at INDEX (no equal key) and raises *bad.
template <class P>
NKV_HD inline __attribute__((always_inline)) uint32_t search(uint64_t n, P at, uint64_t* found, bool* bad) {
    int c = at(0);
    uint64_t j = 0;
    if (c < 0) return NKV_STAGE_SUMMARY;  // key < MinKey
    if (c == 1 && n > 1) {
        j = n - 1;
        c = at(j);
    }
    if (c == 1) return NKV_STAGE_SUMMARY;  // key > MaxKey
    if (c < 0) {  // K_0 < key < K_(n-1): the first entry in (0, n - 1) whose key is not below the query's
        uint64_t lo = 1, hi = n - 1;
        while (lo < hi) {
            j = lo + (hi - lo) / 2;
            c = at(j);
            if (c == 1) lo = j + 1;
            else if (c < 0) hi = j;
            else break;  // equal, or a bad entry
        }
    }
    if (c == kBad) *bad = true;
    if (c != 0) return NKV_STAGE_INDEX;
    *found = j;
    return NKV_STAGE_FOUND;
}

}  // namespace nkv

#if defined(__HIPCC__)
#include "context.hpp"
#include "murmur_dev.hpp"

namespace nkv {

struct Tables {  // kernel argument: the T tables in search order, named base, base + 1, ..
    const uint8_t* img[NKV_LOOKUP_MAX_TABLES];  // the Data stream, or the Index image
    uint64_t len[NKV_LOOKUP_MAX_TABLES];
    const uint64_t* off[NKV_LOOKUP_MAX_TABLES];
    const uint32_t* bits[NKV_LOOKUP_MAX_TABLES];  // nullptr: every key passes
    uint64_t M[NKV_LOOKUP_MAX_TABLES];            // fastmod_magic(m)
    uint32_t n[NKV_LOOKUP_MAX_TABLES], m[NKV_LOOKUP_MAX_TABLES], k[NKV_LOOKUP_MAX_TABLES],
        seed[NKV_LOOKUP_MAX_TABLES];
    int T;
    uint32_t base;
};

struct TableView {  // one caller's table, whatever its struct calls the fields
    const void* img;
    uint64_t len;
    const uint64_t* off;
    uint64_t n;
    const void* bits;
    uint32_t m, k, seed0;
};

// The tables as the kernels take them; NKV_ERR_INVALID for what the header
// refuses.  view(tables[t]) is the entry point's adapter.
template <class U, class V>
int pack_tables(const U* tables, int T, uint32_t table_base, V view, Tables* R) {
    if (!tables || T < 1 || T > NKV_LOOKUP_MAX_TABLES) return NKV_ERR_INVALID;
    if (uint64_t(table_base) + uint64_t(T) > 65536) return NKV_ERR_INVALID;
    *R = Tables{};
    R->T = T;
    R->base = table_base;
    for (int t = 0; t < T; ++t) {
        const TableView u = view(tables[t]);
        if (u.n < 1 || u.n > kMaxN || !u.img || !u.off) return NKV_ERR_INVALID;
        if (u.bits && u.k && u.m == 0) return NKV_ERR_INVALID;
        R->img[t] = static_cast<const uint8_t*>(u.img);
        R->len[t] = u.len;
        R->off[t] = u.off;
        R->n[t] = uint32_t(u.n);
        const bool filtered = u.bits && u.k;  // k = 0: Query's loop has no bit to miss
        R->bits[t] = filtered ? static_cast<const uint32_t*>(u.bits) : nullptr;
        R->m[t] = filtered ? u.m : 1;
        R->M[t] = fastmod_magic(R->m[t]);
        R->k[t] = filtered ? u.k : 0;
        R->seed[t] = u.seed0;
    }
    return NKV_OK;
}

// One table's search: the filter test (murmur_dev.hpp), then the sorted search
// with every probed key read in place.
template <class F>
__device__ __forceinline__ uint32_t search_table(const Tables& R, int t, const Query& Q, uint64_t* found, bool* bad) {
    const uint32_t* bits = R.bits[t];
    if (bits && !filter_query(Q.key, Q.len, bits, R.m[t], R.M[t], R.k[t], R.seed[t])) return NKV_STAGE_FILTER;
    const uint8_t* __restrict__ img = R.img[t];
    const uint64_t L = R.len[t];
    const uint64_t* __restrict__ off = R.off[t];
    return search(uint64_t(R.n[t]), [&](uint64_t j) { return probe<F>(Q, img, L, off, j); }, found, bad);
}

// The body of k_lookup and k_locate: one lane per query, the tables in order.
// Every wave with a query keeps its 64 lanes busy: lanes past q redo the last
// query and store nothing.
template <class F>
__device__ __forceinline__ void search_tables(const Tables& R, F f, const uint8_t* __restrict__ keys,
                                              const uint64_t* __restrict__ koff, const uint64_t* __restrict__ klen,
                                              uint64_t q, uint64_t* __restrict__ hit, uint8_t* __restrict__ status,
                                              uint8_t* __restrict__ stage, unsigned int* __restrict__ err) {
    const uint64_t gi = uint64_t(blockIdx.x) * kBlock + threadIdx.x;
    if ((gi & ~uint64_t(63)) >= q) return;
    const bool live = gi < q;
    const uint64_t i = live ? gi : q - 1;
    bool answered = false;  // left exactly as it was
    if constexpr (F::kOverlay) answered = f.overlay && status[i] != NKV_GET_ABSENT;
    const Query Q = query_of(keys, koff, klen, i);
    uint64_t h = kNoHit;
    uint8_t st = NKV_GET_ABSENT;
    bool bad = false;
    for (int t = 0; t < R.T; ++t) {
        uint32_t sg = NKV_STAGE_NOT_SEARCHED;
        if (h == kNoHit && !answered) {
            uint64_t j = 0;
            sg = search_table<F>(R, t, Q, &j, &bad);
            if (sg == NKV_STAGE_FOUND && !f.answer(R.img[t] + R.off[t][j], &st)) sg = NKV_STAGE_INDEX;
            if (sg == NKV_STAGE_FOUND) h = hit_word(R.base + uint32_t(t), j);
        }
        if (stage && live) stage[i * uint64_t(R.T) + t] = uint8_t(sg);
    }
    if (live && !answered) {
        hit[i] = h;
        status[i] = st;
        f.store(i);
        if (bad) atomicOr(err, 1u);
    }
}

}  // namespace nkv
#endif
