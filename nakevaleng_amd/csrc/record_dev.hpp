// record_dev.hpp -- the record format and the key order, once, for every
// kernel and host function that reads records: the header's layout, the
// bounds checks that keep a wild offset or size from reaching a load (a
// record's, and an Index entry's beside them), the dense entry the merge and
// the flush validate, and bytes.Compare by an 8-byte prefix.  The functions are pure and compile as plain host C++ too
// (tests/cpp/test_record_layer.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define NKV_HD __host__ __device__
#else
#define NKV_HD
#endif

namespace nkv {

// record.go:191-199:
//   Crc u32 | Timestamp i64 | Status u8 | TypeInfo u8 | KeySize u64 | ValueSize u64 | Key | Value
// little endian, at any alignment.
constexpr int kHdr = 30;  // bytes in front of the key
constexpr int kAtCrc = 0, kAtTimestamp = 4, kAtStatus = 12, kAtTypeInfo = 13, kAtKeySize = 14, kAtValueSize = 22;

NKV_HD inline __attribute__((always_inline)) uint64_t ld_le64(const uint8_t* p) {  // any alignment
    uint64_t v = 0;
#if defined(__clang__)
#pragma unroll
#endif
    for (int b = 0; b < 8; ++b) v |= uint64_t(p[b]) << (8 * b);
    return v;
}

// bytes.Compare: unsigned lexicographic, a proper prefix sorts first
NKV_HD inline int cmp_bytes(const uint8_t* a, uint64_t la, const uint8_t* b, uint64_t lb) {
    const uint64_t m = la < lb ? la : lb;
    for (uint64_t i = 0; i < m; ++i) {
        const uint8_t x = a[i], y = b[i];
        if (x != y) return x < y ? -1 : 1;
    }
    return la < lb ? -1 : (la > lb ? 1 : 0);
}

// A record header [r, r + 30) lies inside a stream of len bytes; written so
// that a wild offset near 2^64 cannot wrap past the check.
NKV_HD inline bool header_in(uint64_t r, uint64_t len) { return r <= len && len - r >= kHdr; }

// The two checks compare a size against the room left behind the header and
// never form o + 30 + KeySize first, so no offset or size can wrap past them;
// nothing outside [s, s + L) is read, and nothing at all unless the header is in.
//
// Key span: the header of the record at s + o lies in the stream and so does
// its key, [o + 30, o + 30 + KeySize).  Yields KeySize.
NKV_HD inline bool key_span_in(const uint8_t* s, uint64_t L, uint64_t o, uint64_t* ks) {
    if (!header_in(o, L)) return false;
    const uint64_t k = ld_le64(s + o + kAtKeySize);
    if (k > L - o - kHdr) return false;
    *ks = k;
    return true;
}

// The same check for an Index or Summary entry, KeySize u64 | Offset i64 | Key:
// the entry at img + o lies inside the image of L bytes, its two fields and
// its key.  Yields KeySize.
constexpr uint64_t kEntryHdr = 16;  // KeySize + Offset in front of every entry's key
NKV_HD inline bool entry_in(const uint8_t* img, uint64_t L, uint64_t o, uint64_t* ks) {
    if (o > L || L - o < kEntryHdr) return false;
    const uint64_t k = ld_le64(img + o);
    if (k > L - o - kEntryHdr) return false;
    *ks = k;
    return true;
}

// Record span: the key span holds and the value ends inside the stream too.
// Yields KeySize and ValueSize (both fields are loaded before either is judged).
NKV_HD inline bool record_span_in(const uint8_t* s, uint64_t L, uint64_t o, uint64_t* ks, uint64_t* vs) {
    if (!header_in(o, L)) return false;
    const uint64_t k = ld_le64(s + o + kAtKeySize), v = ld_le64(s + o + kAtValueSize);
    const uint64_t room = L - o - kHdr;
    if (k > room || v > room - k) return false;
    *ks = k;
    *vs = v;
    return true;
}

// The first 8 key bytes big-endian, zero-padded: keys compare as their
// prefixes do wherever the prefixes differ.
NKV_HD inline uint64_t key_prefix(const uint8_t* key, uint64_t len) {
    uint64_t p = 0;
    for (uint32_t b = 0; b < 8 && b < len; ++b) p |= uint64_t(key[b]) << (56 - 8 * b);
    return p;
}

// What lies behind a key's prefix: its length and the bytes after the first 8.
struct KeyRest {
    uint64_t n;
    const uint8_t* t;
    NKV_HD uint64_t len() const { return n; }
    NKV_HD const uint8_t* tail() const { return t; }
};

// bytes.Compare of two keys given as prefix and rest.  Equal padded prefixes:
// a key of at most 8 bytes is a prefix of the other, so the lengths decide.
// len() is asked for only when the prefixes are equal and tail() only when
// both keys are longer than 8 bytes as well, so a rest that has to load them
// (the dense arrays of merge.hip and memtable.hip) loads them only then.
template <class A, class B>
NKV_HD inline int cmp_prefixed(uint64_t pa, const A& a, uint64_t pb, const B& b) {
    if (pa != pb) return pa < pb ? -1 : 1;
    const uint64_t la = a.len(), lb = b.len();
    if (la <= 8 || lb <= 8) return la < lb ? -1 : (la > lb ? 1 : 0);
    return cmp_bytes(a.tail(), la - 8, b.tail(), lb - 8);
}
// The same with both rests at hand: prefix, length, pointer to the bytes after the first 8.
NKV_HD inline int cmp_prefixed(uint64_t pa, uint64_t la, const uint8_t* ta, uint64_t pb, uint64_t lb,
                               const uint8_t* tb) {
    return cmp_prefixed(pa, KeyRest{la, ta}, pb, KeyRest{lb, tb});
}

// What the merge and the flush keep of a validated record.
struct DenseEntry {
    uint64_t pfx;   // key_prefix
    uint64_t klen;  // KeySize
    uint64_t size;  // TotalSize
};

// Record i of the n records at s + off[] in a stream of L bytes.  True: its
// span holds and *e is filled.  *bad: the span does not hold, the record does
// not end where the next starts (the last: where the stream ends), or the
// first record does not start the stream.
NKV_HD inline bool dense_entry(const uint8_t* s, uint64_t L, const uint64_t* off, uint32_t i, uint32_t n,
                               DenseEntry* e, bool* bad) {
    const uint64_t o = off[i];
    uint64_t ks, vs;
    *bad = true;
    if ((i == 0 && o != 0) || !record_span_in(s, L, o, &ks, &vs)) return false;
    const uint64_t end = o + kHdr + ks + vs;  // <= L: no overflow
    *bad = end != (i + 1 < n ? off[i + 1] : L);
    e->pfx = key_prefix(s + o + kHdr, ks);
    e->klen = ks;
    e->size = kHdr + ks + vs;
    return true;
}

}  // namespace nkv
