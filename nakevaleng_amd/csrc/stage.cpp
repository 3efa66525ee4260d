// stage.cpp -- the staging layer of the host-pointer entries: every step that
// moves such an entry's inputs to the device or its results back (declared in
// context.hpp).  The entries themselves live with their paths (tree.cpp and
// the *.hip units) and pick their scratch; what they share is here, once.
#include <string.h>

#include "context.hpp"

namespace nkv {

// What the n sizes leave of stream_len, taken off term by term so a wrapped
// sum cannot pass; false if they do not fit.
static bool records_left(const uint64_t* rec_size, uint64_t n, uint64_t stream_len, uint64_t* left) {
    *left = stream_len;
    for (uint64_t i = 0; i < n; ++i) {
        if (rec_size[i] > *left) return false;
        *left -= rec_size[i];
    }
    return true;
}

bool records_fit(const uint64_t* rec_size, uint64_t n, uint64_t stream_len) {
    uint64_t left;
    return records_left(rec_size, n, stream_len, &left);
}

bool records_fill(const uint64_t* rec_size, uint64_t n, uint64_t stream_len) {
    uint64_t left;
    return records_left(rec_size, n, stream_len, &left) && left == 0;
}

int read_verdict(nkv_ctx* c, const unsigned int* d_err) {
    unsigned int h = 0;
    HIPTRY(hipMemcpyAsync(&h, d_err, 4, hipMemcpyDeviceToHost, c->stream));
    HIPTRY(hipStreamSynchronize(c->stream));
    return h ? NKV_ERR_INVALID : NKV_OK;
}

int verdict_word(nkv_ctx* c, uint32_t* d_err, unsigned int** err) {
    *err = d_err;
    if (!d_err) {
        TRY(grow(c->d_stats, 8));
        *err = static_cast<unsigned int*>(c->d_stats.p);
    }
    HIPTRY(hipMemsetAsync(*err, 0, 4, c->stream));
    return NKV_OK;
}

int finish_verdict(nkv_ctx* c, const uint32_t* d_err, const unsigned int* err) {
    return d_err ? NKV_OK : read_verdict(c, err);
}

// Plain copies from the caller's (pageable) memory, not the pipelined Stager:
// the route of nkv_sort_records, nkv_merge_records and
// nkv_index_summary_from_records.  Moving them onto the Stager (stage_records)
// would probably be faster, but it changes their timing and needs a
// measurement of its own: a separate change.
int upload_records(nkv_ctx* c, const uint8_t* stream, uint64_t stream_len, const uint64_t* rec_size, uint64_t n,
                   void* d_stream, uint64_t* d_size, uint64_t* d_off) {
    HIPTRY(hipMemcpyAsync(d_stream, stream, stream_len, hipMemcpyHostToDevice, c->stream));
    HIPTRY(hipMemcpyAsync(d_size, rec_size, 8 * n, hipMemcpyHostToDevice, c->stream));
    return nkv_record_offsets_dev(c, d_size, n, d_off);
}

int download_table(nkv_ctx* c, const void* d_table, uint64_t len, const uint64_t* d_off, uint64_t n, uint8_t* out,
                   uint64_t* out_rec_size) {
    std::vector<uint64_t> off(n);
    HIPTRY(hipMemcpyAsync(out, d_table, len, hipMemcpyDeviceToHost, c->stream));
    HIPTRY(hipMemcpyAsync(off.data(), d_off, 8 * n, hipMemcpyDeviceToHost, c->stream));
    HIPTRY(hipStreamSynchronize(c->stream));
    for (uint64_t j = 0; j < n; ++j) out_rec_size[j] = (j + 1 < n ? off[j + 1] : len) - off[j];
    return NKV_OK;
}

// n offsets and lengths in h_stage to d_off / d_len (grown by the caller, before
// it queues anything: growing frees, and a free waits for the device)
static int upload_off_len(nkv_ctx* c, const uint64_t* off, const uint64_t* len, uint64_t n) {
    HIPTRY(hipMemcpyAsync(c->d_off.p, off, 8 * n, hipMemcpyHostToDevice, c->stream));
    HIPTRY(hipMemcpyAsync(c->d_len.p, len, 8 * n, hipMemcpyHostToDevice, c->stream));
    return NKV_OK;
}

// Move n host values to the device and upload their offsets/lengths to d_off /
// d_len; *d_base / *aligned tell the kernels where the values are.
//  - Values inside one pinned block of this context (the deferred-NewLeaf
//    arena, nkv_host_alloc): one DMA straight from the block into its device
//    mirror, minus the prefix nkv_host_stream already queued; offsets are the
//    values' places in the block (aligned iff all are 16-byte aligned).
//  - Anything else: packed at 16-byte aligned offsets through the pipelined
//    pinned stager (a pool of host threads gathers chunk k+1 while chunk k is
//    in flight).
// No caller pointer is kept either way.
int stage_values(nkv_ctx* c, const uint8_t* base, const uint64_t* off, const uint64_t* len, uint64_t n,
                 const uint8_t** d_base, bool* aligned) {
    uint64_t lo = 0, hi = 0, total = 0;
    nkv_ctx::Pinned* const blk = pinned_extent(c, base, off, len, n, &lo, &hi);
    *d_base = nullptr;
    *aligned = true;
    for (uint64_t i = 0; !blk && i < n; ++i) {
        if (len[i] > (uint64_t(1) << 62) || total > (uint64_t(1) << 62)) return NKV_ERR_INVALID;
        total += align16(len[i]);
    }
    TRY(grow_host(c, 16 * n));
    if (!blk) TRY(grow(c->d_data, total));
    TRY(grow(c->d_off, 8 * n));
    TRY(grow(c->d_len, 8 * n));
    uint64_t* hoff = static_cast<uint64_t*>(c->h_stage);
    uint64_t* hlen = hoff + n;
    const uint64_t adj = blk ? uint64_t(base - blk->p) : 0;
    uint64_t p = 0, ormask = 0;
    for (uint64_t i = 0; i < n; ++i) {  // places in the block, or packed at multiples of 16
        hoff[i] = blk ? adj + off[i] : p;
        hlen[i] = len[i];
        ormask |= hoff[i];
        p += align16(len[i]);
    }
    if (blk) {
        // the prefix nkv_host_stream queued is already on its way; the rest now
        TRY(stream_block(c, blk, std::max(lo, blk->streamed), hi));
        blk->streamed = 0;  // this call consumes the batch: a new one streams from 0
    } else {
        const Segments seg{base, off, len, hoff, n};
        HIPTRY(c->stage.upload(seg, total, static_cast<uint8_t*>(c->d_data.p), c->stream));
    }
    TRY(upload_off_len(c, hoff, hlen, n));
    *d_base = static_cast<const uint8_t*>(blk ? blk->d_arena.p : c->d_data.p);
    *aligned = (ormask & 15) == 0;
    return NKV_OK;
}

int stage_spans(nkv_ctx* c, const uint8_t* base, const uint64_t* off, const uint64_t* len, uint64_t n) {
    uint64_t total = 0;
    for (uint64_t i = 0; i < n; ++i) total = std::max(total, off[i] + len[i]);
    TRY(grow_host(c, 16 * n));
    TRY(grow(c->d_data, total + 1));
    TRY(grow(c->d_off, 8 * n));
    TRY(grow(c->d_len, 8 * n));
    uint64_t* h = static_cast<uint64_t*>(c->h_stage);
    HIPTRY(c->stage.upload(base, total, static_cast<uint8_t*>(c->d_data.p), c->stream));
    memcpy(h, off, 8 * n);
    memcpy(h + n, len, 8 * n);
    return upload_off_len(c, h, h + n, n);
}

int stage_records(nkv_ctx* c, const uint8_t* stream, uint64_t stream_len, const uint64_t* rec_size, uint64_t n,
                  const uint64_t** rec_off) {
    if (!records_fit(rec_size, n, stream_len)) return NKV_ERR_INVALID;
    TRY(grow(c->d_data, stream_len));
    TRY(grow(c->d_aux, 8 * n));
    TRY(grow(c->d_rec_off, 8 * n));
    TRY(grow_host(c, 8 * n));
    HIPTRY(c->stage.upload(stream, stream_len, static_cast<uint8_t*>(c->d_data.p), c->stream));
    memcpy(c->h_stage, rec_size, 8 * n);
    HIPTRY(hipMemcpyAsync(c->d_aux.p, c->h_stage, 8 * n, hipMemcpyHostToDevice, c->stream));
    *rec_off = static_cast<const uint64_t*>(c->d_rec_off.p);
    return nkv_record_offsets_dev(c, static_cast<const uint64_t*>(c->d_aux.p), n, static_cast<uint64_t*>(c->d_rec_off.p));
}

}  // namespace nkv
