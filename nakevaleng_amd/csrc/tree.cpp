// tree.cpp -- the Merkle tree path's host side: the order plan of a ragged
// batch, level 0 in that order, the records forms, and the tree entries of
// the C-ABI (host-buffer and device-resident).  Kernels: leaf.hip, plan.hip,
// reduce.hip.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "context.hpp"

using namespace nkv;

namespace nkv {
namespace {

// This call's pass flags and the set its leaf kernel resets for the next call
// (internal.hpp kPassFlagWords); flip_pass_flags once that kernel is launched.
void pass_flags(nkv_ctx* c, uint32_t** cur, uint32_t** next) {
    uint32_t* f = static_cast<uint32_t*>(c->state.d_flags.p);
    *cur = f + kPassFlagWords * c->flag_set;
    *next = f + kPassFlagWords * (1 - c->flag_set);
}
void flip_pass_flags(nkv_ctx* c) { c->flag_set ^= 1; }

// scratch for k_locate's per-workgroup partials
int locate_parts(nkv_ctx* c, uint64_t n, uint32_t** part) {
    TRY(grow(c->d_part, 4 * locate_part_words(n)));
    *part = static_cast<uint32_t*>(c->d_part.p);
    return NKV_OK;
}

// Order of a ragged batch for the leaf kernel (NKV_OPT_BUCKET): input order
// (no sort), length-sorted (work queue), or both kernels
// launched behind a device-side Gate.  Auto mode (2) sorts batches of fewer than
// 4096 values; for larger ones a narrow range of full-block counts
// (max <= min + max(1, min / 16), e.g. SSTable records of one size) gains
// nothing from sorting.  With the lengths on the host the choice is made here;
// with device lengths only, k_len_range measures the range and the two leaf
// kernels read it (no host read-back, so device-resident calls stay
// asynchronous; the sort then runs either way).
enum Plan { kInputOrder = 0, kSorted = 1, kGated = 2 };

// THE rule, before anything is known about the lengths: input order without
// bucketing or for tiny batches; gated for >= 4096 values in auto mode; else
// everything sorted.  As a number it is the policy of k_leaf_records and
// k_leaf_verify (0 hash every wave, 2 defer every wave, 1 defer the ragged ones).
Plan batch_plan(const nkv_ctx* c, uint64_t n) {
    if (c->bucket == 0 || n <= 64) return kInputOrder;
    return c->bucket == 2 && n >= 4096 ? kGated : kSorted;
}
int policy_of(Plan p) { return p == kInputOrder ? 0 : p == kGated ? 1 : 2; }

// dev_range (nullable): the batch's range already on the device (k_locate wrote it)
int plan_of(nkv_ctx* c, const uint64_t* len, const uint64_t* host_len, uint64_t n, int* plan, Gate* gate,
            const unsigned int* dev_range = nullptr) {
    *plan = batch_plan(c, n);
    *gate = Gate{};
    if (*plan != kGated) return NKV_OK;
    if (host_len) {
        uint64_t lo = ~uint64_t(0), hi = 0;
        for (uint64_t i = 0; i < n; ++i) {
            const uint64_t b = host_len[i] >> 6;
            lo = std::min(lo, b);
            hi = std::max(hi, b);
        }
        *plan = hi <= lo + std::max<uint64_t>(1, lo / 16) ? kInputOrder : kSorted;
        return NKV_OK;
    }
    if (dev_range) {
        gate->range = dev_range;
        return NKV_OK;
    }
    TRY(grow(c->d_range, 8));
    unsigned int* d = static_cast<unsigned int*>(c->d_range.p);
    uint32_t* part = nullptr;
    TRY(locate_parts(c, n, &part));
    DevBuf& d_ticket = c->state.d_ticket;
    const size_t tcap = d_ticket.cap;
    TRY(grow(d_ticket, 16));
    if (d_ticket.cap != tcap) HIPTRY(hipMemsetAsync(d_ticket.p, 0, 16, c->stream));
    HIPTRY(launch_len_range(len, n, d, part, static_cast<unsigned int*>(d_ticket.p), c->stream));
    gate->range = d;
    return NKV_OK;
}

// The context's second stream and its fork / join events (NKV_OPT_SIDE_GATE).
int side_ready(nkv_ctx* c) {
    if (!c->side) HIPTRY(hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking));
    for (hipEvent_t& e : c->side_ev)
        if (!e) HIPTRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return NKV_OK;
}

// Level 0 in the order plan_of chose.  Gated plans also launch the input-order
// kernel (it runs when the range is narrow) unless the caller has its own
// (narrow_kernel = false: k_leaf_verify).
int leaf_level(nkv_ctx* c, const uint8_t* base, const uint64_t* off, const uint64_t* len, uint64_t n,
               bool aligned, uint8_t* nodes, int plan, Gate range, bool narrow_kernel = true,
               CopyWords cw = CopyWords{}) {
    if (plan == kInputOrder && cw.n) return NKV_ERR_INVALID;  // the copy rides on the sort
    if (plan == kInputOrder) return st(launch_leaf_offsets(base, off, len, n, aligned, c->leaf_load, nodes, c->stream));
    if (n > 0x7fffffffull) return NKV_ERR_INVALID;
    const Gate wide{range.range, plan == kGated ? 2 : 0};
    DevBuf& d_keys = c->state.d_keys;
    const size_t keys_cap = d_keys.cap;
    TRY(grow(d_keys, 4 * sort_hist_words(n)));
    // (re)allocated scratch, or a sort cut short by an error: the sort's bucket
    // totals must start at zero (its last workgroup leaves them zero again)
    if (d_keys.cap != keys_cap || c->sort_dirty) {
        HIPTRY(hipMemsetAsync(d_keys.p, 0, 4 * sort_head_words(), c->stream));
        c->sort_dirty = false;
    }
    c->sort_dirty = true;  // until the sort and the kernels behind it are queued
    TRY(grow(c->d_perm, 4 * n));
    uint32_t* perm = static_cast<uint32_t*>(c->d_perm.p);
    TRY(grow(c->d_queue, 4 * queue_words(n)));
    const QueueInit qi{static_cast<uint32_t*>(c->d_queue.p), queue_words(n), uint32_t(c->queue_split)};
    // the gated input-order kernel writes level 0 only when the range is narrow,
    // the sort and the queue only when it is wide: on the side stream it runs
    // beside them, so the closed ones cost the batch no launch slot
    const bool narrow = plan == kGated && narrow_kernel;
    const bool forked = narrow && c->side_gate;
    if (forked) {
        TRY(side_ready(c));
        HIPTRY(hipEventRecord(c->side_ev[0], c->stream));
        HIPTRY(hipStreamWaitEvent(c->side, c->side_ev[0], 0));
        HIPTRY(launch_leaf_offsets(base, off, len, n, aligned, c->leaf_load, nodes, c->side, Gate{range.range, 1}));
        HIPTRY(hipEventRecord(c->side_ev[1], c->side));
    }
    int rc = st(sort_by_length_desc(len, n, perm, static_cast<uint32_t*>(d_keys.p), c->stream, wide, qi, cw));
    if (rc == NKV_OK)
        rc = st(launch_leaf_queue(base, off, len, perm, n, static_cast<uint32_t*>(c->d_queue.p), c->simds,
                                  uint32_t(c->queue_waves), nodes, c->stream, wide));
    if (forked) {  // joined whatever happened above: nothing on the stream may pass it
        const int j = st(hipStreamWaitEvent(c->stream, c->side_ev[1], 0));
        if (rc == NKV_OK) rc = j;
    } else if (rc == NKV_OK && narrow) {
        rc = st(launch_leaf_offsets(base, off, len, n, aligned, c->leaf_load, nodes, c->stream, Gate{range.range, 1}));
    }
    TRY(rc);
    c->sort_dirty = false;
    return NKV_OK;
}

// Behind level 0 of every tree call: the levels above it, between the timing marks.
int levels_above(nkv_ctx* c, uint8_t* nodes, uint64_t n) {
    TRY(mark(c, 1));
    HIPTRY(launch_reduce(nodes, n, 0, levels_of(n) - 1, c->stream));
    return mark(c, 2);
}

// The deferred plan's value places (d_off / d_len), the range word and the
// locate partials of a records batch.
struct RecordsScratch {
    uint64_t *voff, *vlen;
    unsigned int* range;
    uint32_t* part;
};
int records_scratch(nkv_ctx* c, uint64_t n, RecordsScratch* s) {
    TRY(grow(c->d_off, 8 * n));
    TRY(grow(c->d_len, 8 * n));
    TRY(grow(c->d_range, 8));
    s->voff = static_cast<uint64_t*>(c->d_off.p);
    s->vlen = static_cast<uint64_t*>(c->d_len.p);
    s->range = static_cast<unsigned int*>(c->d_range.p);
    return locate_parts(c, n, &s->part);
}

// The Merkle step of a device-resident Data table: one k_leaf_records launch
// locates every record's value and hashes it in input order -- all of them
// (NKV_OPT_BUCKET 0), or (auto) the waves whose block counts are narrow, the
// others deferred -- then the length-sorted work queue takes what was deferred
// (behind a device Gate: on a table of one record size it is never opened),
// then the levels.  err (device u32) = 1 if a header points outside the stream.
int records_tree(nkv_ctx* c, const uint8_t* stream, uint64_t stream_len, const uint64_t* rec_off, uint64_t n,
                 uint8_t* nodes, unsigned int* err) {
    RecordsScratch s;
    TRY(records_scratch(c, n, &s));
    const Plan plan = batch_plan(c, n);
    if (!c->records_fused) {  // NKV_OPT_RECORDS_FUSED 0: separate locate pass, then the leaf plan
        const bool gated = plan == kGated;
        HIPTRY(launch_locate(stream, stream_len, rec_off, n, s.voff, s.vlen, err, gated ? s.range : nullptr, s.part,
                             c->stream));
        return tree_from_device_values(c, stream, s.voff, s.vlen, n, false, nodes, nullptr, gated ? s.range : nullptr);
    }
    TRY(mark(c, 0));
    if (plan == kInputOrder) {
        HIPTRY(launch_leaf_records(stream, stream_len, rec_off, n, 0, s.voff, s.vlen, nodes, err, s.range, s.part,
                                   c->stream));
    } else {  // deferred plan: the pass flags gate the sorted pass, whose first launch copies err out
        uint32_t *flags, *next;
        pass_flags(c, &flags, &next);
        HIPTRY(launch_leaf_records(stream, stream_len, rec_off, n, policy_of(plan), s.voff, s.vlen, nodes, nullptr,
                                   nullptr, nullptr, c->stream, flags, next));
        flip_pass_flags(c);
        TRY(leaf_level(c, stream, s.voff, s.vlen, n, false, nodes, plan, Gate{flags, 0}, false,
                       CopyWords{flags + 2, err, 1}));
    }
    return levels_above(c, nodes, n);
}

}  // namespace

int leaf_level(nkv_ctx* c, const uint8_t* base, const uint64_t* off, const uint64_t* len, uint64_t n,
               bool aligned, uint8_t* nodes, const uint64_t* host_len) {
    int plan = kInputOrder;
    Gate g;
    TRY(plan_of(c, len, host_len, n, &plan, &g));
    return leaf_level(c, base, off, len, n, aligned, nodes, plan, g);
}

// host_len (nullable): the value lengths on the host, when the caller has them.
// Every order leaves level 0 complete, so one reduce sequence follows.
int tree_from_device_values(nkv_ctx* c, const uint8_t* base, const uint64_t* off, const uint64_t* len,
                            uint64_t n, bool aligned, uint8_t* nodes, const uint64_t* host_len,
                            const unsigned int* dev_range) {
    int plan = kInputOrder;
    Gate g;
    TRY(plan_of(c, len, host_len, n, &plan, &g, dev_range));
    TRY(mark(c, 0));
    TRY(leaf_level(c, base, off, len, n, aligned, nodes, plan, g));
    return levels_above(c, nodes, n);
}

int finish_tree(nkv_ctx* c, uint8_t* nodes, uint64_t n, uint8_t* root20, uint8_t* nodes_out,
                uint8_t* img_out) {
    const uint64_t tot = total_of(n);
    if (img_out) {
        BfsLayout lay = layout_of(counts_of(n));
        TRY(grow(c->d_img, lay.total));
        HIPTRY(launch_bfs_image(nodes, lay, static_cast<uint8_t*>(c->d_img.p), c->stream));
        HIPTRY(c->stage.download(img_out, static_cast<const uint8_t*>(c->d_img.p), lay.total, c->stream));
    }
    if (nodes_out) HIPTRY(c->stage.download(nodes_out, nodes, 20 * tot, c->stream));
    if (root20)
        HIPTRY(hipMemcpyAsync(root20, nodes + 20 * (tot - 1), 20, hipMemcpyDeviceToHost, c->stream));
    HIPTRY(hipStreamSynchronize(c->stream));
    return NKV_OK;
}

}  // namespace nkv

// the staged offsets and lengths of stage_values
static const uint64_t* staged_off(const nkv_ctx* c) { return static_cast<const uint64_t*>(c->d_off.p); }
static const uint64_t* staged_len(const nkv_ctx* c) { return static_cast<const uint64_t*>(c->d_len.p); }

extern "C" {

// ---- host-buffer API ----
int nkv_leaf_hash(nkv_ctx* c, const uint8_t* base, const uint64_t* off, const uint64_t* len,
                  uint64_t n, uint8_t* out20) try {
    TRY(bind(c));
    if (n > kMaxN) return NKV_ERR_INVALID;
    if (n == 0) return NKV_OK;
    if (!base || !off || !len || !out20) return NKV_ERR_INVALID;
    const uint8_t* d_base = nullptr;
    bool aligned = true;
    TRY(stage_values(c, base, off, len, n, &d_base, &aligned));
    TRY(grow(c->d_nodes, 20 * n));
    uint8_t* nodes = static_cast<uint8_t*>(c->d_nodes.p);
    TRY(leaf_level(c, d_base, staged_off(c), staged_len(c), n, aligned, nodes, len));
    HIPTRY(c->stage.download(out20, nodes, 20 * n, c->stream));
    return st(hipStreamSynchronize(c->stream));
} NKV_CATCH

int nkv_tree_build(nkv_ctx* c, const uint8_t* leaf20, uint64_t n, uint8_t* root20,
                   uint8_t* nodes_out, uint8_t* img_out) try {
    TRY(bind(c));
    if (n > kMaxN) return NKV_ERR_INVALID;
    if (n == 0) return NKV_ERR_EMPTY;
    if (!leaf20) return NKV_ERR_INVALID;
    TRY(grow(c->d_nodes, 20 * total_of(n)));
    uint8_t* nodes = static_cast<uint8_t*>(c->d_nodes.p);
    HIPTRY(c->stage.upload(leaf20, 20 * n, nodes, c->stream));
    HIPTRY(launch_reduce(nodes, n, 0, levels_of(n) - 1, c->stream));
    return finish_tree(c, nodes, n, root20, nodes_out, img_out);
} NKV_CATCH

int nkv_tree_from_values(nkv_ctx* c, const uint8_t* base, const uint64_t* off, const uint64_t* len,
                         uint64_t n, uint8_t* root20, uint8_t* nodes_out, uint8_t* img_out) try {
    TRY(bind(c));
    if (n > kMaxN) return NKV_ERR_INVALID;
    if (n == 0) return NKV_ERR_EMPTY;
    if (!base || !off || !len) return NKV_ERR_INVALID;
    bool small = false;
    TRY(small_tree(c, base, off, len, n, root20, nodes_out, img_out, &small));
    if (small) return NKV_OK;
    c->last_path = NKV_PATH_GRID;
    TRY(host_mark(c, 0));
    const uint8_t* d_base = nullptr;
    bool aligned = true;
    TRY(stage_values(c, base, off, len, n, &d_base, &aligned));
    TRY(grow(c->d_nodes, 20 * total_of(n)));
    uint8_t* nodes = static_cast<uint8_t*>(c->d_nodes.p);
    TRY(tree_from_device_values(c, d_base, staged_off(c), staged_len(c), n, aligned, nodes, len));
    TRY(finish_tree(c, nodes, n, root20, nodes_out, img_out));
    return host_mark(c, 1);
} NKV_CATCH

uint64_t nkv_generic_bfs_size(const uint64_t* len, uint64_t n) {
    if (n == 0 || !len) return 0;
    // levels 1..top are 20-byte nodes; level 0 is the raw leaves
    uint64_t s = nkv_bfs_size(n) - 21 * n;
    for (uint64_t i = 0; i < n; ++i) s += len[i] ? 1 + len[i] : 1;
    return s;
}

int nkv_tree_generic(nkv_ctx* c, const uint8_t* data, const uint64_t* off, const uint64_t* len,
                     uint64_t n, uint8_t* root20, uint8_t* upper_out, uint8_t* img_out) try {
    TRY(bind(c));
    if (n > kMaxN) return NKV_ERR_INVALID;
    if (n == 0) return NKV_ERR_EMPTY;
    if (!data || !off || !len) return NKV_ERR_INVALID;
    // Level 1 node i = SHA-1(leaf[2i].Data || leaf[2i+1].Data) (merkletree.go:44-46;
    // the pad of an odd level contributes no bytes).  Stage each parent's
    // message contiguously and hash the messages with the leaf kernel; the
    // rest of the tree is the 20-byte reduce over the n1 level-1 nodes.
    const uint64_t n1 = (n + 1) / 2;
    std::vector<uint64_t> moff(n1), mlen(n1);
    std::vector<uint8_t> tmp;
    uint64_t total = 0;
    for (uint64_t i = 0; i < n1; ++i) {
        mlen[i] = len[2 * i] + (2 * i + 1 < n ? len[2 * i + 1] : 0);
        total += mlen[i];
    }
    tmp.resize(total ? total : 1);
    uint64_t p = 0;
    for (uint64_t i = 0; i < n1; ++i) {
        moff[i] = p;
        memcpy(tmp.data() + p, data + off[2 * i], len[2 * i]);
        p += len[2 * i];
        if (2 * i + 1 < n) {
            memcpy(tmp.data() + p, data + off[2 * i + 1], len[2 * i + 1]);
            p += len[2 * i + 1];
        }
    }
    const uint8_t* d_base = nullptr;
    bool aligned = true;
    TRY(stage_values(c, tmp.data(), moff.data(), mlen.data(), n1, &d_base, &aligned));
    const uint64_t up_total = n1 == 1 ? 1 : total_of(n1);
    TRY(grow(c->d_nodes, 20 * up_total));
    uint8_t* up = static_cast<uint8_t*>(c->d_nodes.p);
    TRY(leaf_level(c, d_base, staged_off(c), staged_len(c), n1, aligned, up, mlen.data()));
    if (n1 > 1) HIPTRY(launch_reduce(up, n1, 0, levels_of(n1) - 1, c->stream));
    if (upper_out) HIPTRY(c->stage.download(upper_out, up, 20 * up_total, c->stream));
    if (root20)
        HIPTRY(hipMemcpyAsync(root20, up + 20 * (up_total - 1), 20, hipMemcpyDeviceToHost,
                              c->stream));
    uint64_t upper_img = 0;
    if (img_out) {
        // levels top..1 from the device, level 0 (raw leaf Data) appended here
        std::vector<uint64_t> cnt = n1 == 1 ? std::vector<uint64_t>{1} : counts_of(n1);
        BfsLayout lay = layout_of(cnt);
        // the bottom of this sub-image is level 1 of the whole tree, which is
        // never the top when n1 > 1; its pad is already handled by layout_of
        upper_img = lay.total;
        TRY(grow(c->d_img, lay.total));
        HIPTRY(launch_bfs_image(up, lay, static_cast<uint8_t*>(c->d_img.p), c->stream));
        HIPTRY(c->stage.download(img_out, static_cast<const uint8_t*>(c->d_img.p), lay.total, c->stream));
    }
    HIPTRY(hipStreamSynchronize(c->stream));
    if (img_out) {
        uint8_t* q = img_out + upper_img;
        for (uint64_t i = 0; i < n; ++i) {
            if (len[i] == 0) {
                *q++ = NKV_MERKLE_NODE_EMPTY;
            } else {
                *q++ = 0;
                memcpy(q, data + off[i], len[i]);
                q += len[i];
            }
        }
        if (n & 1) *q++ = NKV_MERKLE_NODE_EMPTY;
    }
    return NKV_OK;
} NKV_CATCH

int nkv_tree_validate(nkv_ctx* c, const uint8_t* leaf_data, const uint64_t* off, const uint64_t* len,
                      uint64_t n, const uint8_t* root20, int* ok) try {
    TRY(bind(c));
    if (n > kMaxN) return NKV_ERR_INVALID;
    if (!ok) return NKV_ERR_INVALID;
    *ok = 0;
    if (n == 0) return NKV_ERR_EMPTY;  // New never builds an empty tree (merkletree.go:19-21)
    if (!leaf_data || !off || !len || !root20) return NKV_ERR_INVALID;
    bool all20 = true;
    for (uint64_t i = 0; i < n && all20; ++i) all20 = len[i] == NKV_DIGEST_SIZE;
    uint8_t got[NKV_DIGEST_SIZE];
    if (all20) {
        // NewLeaf leaves: gather the digests into level 0 and reduce to the root
        TRY(grow_host(c, 8 * n));
        uint64_t* dst = static_cast<uint64_t*>(c->h_stage);
        for (uint64_t i = 0; i < n; ++i) dst[i] = NKV_DIGEST_SIZE * i;
        TRY(grow(c->d_nodes, NKV_DIGEST_SIZE * total_of(n)));
        uint8_t* nodes = static_cast<uint8_t*>(c->d_nodes.p);
        const Segments seg{leaf_data, off, len, dst, n};
        HIPTRY(c->stage.upload(seg, NKV_DIGEST_SIZE * n, nodes, c->stream));
        HIPTRY(launch_reduce(nodes, n, 0, levels_of(n) - 1, c->stream));
        HIPTRY(hipMemcpyAsync(c->h_small, nodes + NKV_DIGEST_SIZE * (total_of(n) - 1), NKV_DIGEST_SIZE,
                              hipMemcpyDeviceToHost, c->stream));
        HIPTRY(hipStreamSynchronize(c->stream));
        memcpy(got, c->h_small, NKV_DIGEST_SIZE);
    } else {
        TRY(nkv_tree_generic(c, leaf_data, off, len, n, got, nullptr, nullptr));
    }
    *ok = memcmp(got, root20, NKV_DIGEST_SIZE) == 0;
    return NKV_OK;
} NKV_CATCH

int nkv_tree_from_records(nkv_ctx* c, const uint8_t* stream, uint64_t stream_len,
                          const uint64_t* rec_size, uint64_t n, uint8_t* root20,
                          uint8_t* nodes_out, uint8_t* img_out) try {
    TRY(bind(c));
    if (n > kMaxN) return NKV_ERR_INVALID;
    if (n == 0) return NKV_ERR_EMPTY;
    if (!stream || !rec_size) return NKV_ERR_INVALID;
    const SmallPath& sp = c->small;
    if (sp.path != 0 && n <= sp.max_n && n <= kSmallMaxN && stream_len <= sp.max_bytes) {
        // a small table (one lsm_run_max compaction at the default sizes): the
        // values' places from the headers here (record.go:191-199, the same
        // bounds k_locate applies), then the one-launch path
        if (!records_fit(rec_size, n, stream_len)) return NKV_ERR_INVALID;
        std::vector<uint64_t> voff(n), vlen(n);
        uint64_t r = 0;
        for (uint64_t i = 0; i < n; ++i) {
            if (!header_in(r, stream_len)) return NKV_ERR_INVALID;
            uint64_t ks = 0, vs = 0;
            memcpy(&ks, stream + r + 14, 8);
            memcpy(&vs, stream + r + 22, 8);
            if (ks > stream_len || vs > stream_len || r + 30 + ks + vs > stream_len) return NKV_ERR_INVALID;
            voff[i] = r + 30 + ks;
            vlen[i] = vs;
            r += rec_size[i];
        }
        bool small = false;
        TRY(small_tree(c, stream, voff.data(), vlen.data(), n, root20, nodes_out, img_out, &small));
        if (small) return NKV_OK;
    }
    const uint64_t* rec_off = nullptr;
    TRY(stage_records(c, stream, stream_len, rec_size, n, &rec_off));
    c->last_path = NKV_PATH_GRID;
    TRY(grow(c->d_nodes, 20 * total_of(n)));
    uint8_t* nodes = static_cast<uint8_t*>(c->d_nodes.p);
    TRY(grow(c->d_err, 4));
    unsigned int* err = static_cast<unsigned int*>(c->d_err.p);
    TRY(records_tree(c, static_cast<const uint8_t*>(c->d_data.p), stream_len, rec_off, n, nodes, err));
    TRY(read_verdict(c, err));
    return finish_tree(c, nodes, n, root20, nodes_out, img_out);
} NKV_CATCH

// ---- device-resident API ----
int nkv_leaf_hash_dev(nkv_ctx* c, const void* d_base, const uint64_t* d_off,
                      const uint64_t* d_len, uint64_t n, void* d_nodes) try {
    TRY(bind(c));
    if (n > kMaxN) return NKV_ERR_INVALID;
    if (n == 0) return NKV_OK;
    if (!d_base || !d_off || !d_len || !d_nodes) return NKV_ERR_INVALID;
    return leaf_level(c, static_cast<const uint8_t*>(d_base), d_off, d_len, n, false,
                      static_cast<uint8_t*>(d_nodes), nullptr);
} NKV_CATCH

int nkv_leaf_hash_strided_dev(nkv_ctx* c, const void* d_base, uint64_t stride, uint64_t len,
                              uint64_t n, void* d_nodes) try {
    TRY(bind(c));
    if (n > kMaxN) return NKV_ERR_INVALID;
    if (n == 0) return NKV_OK;
    if (!d_base || !d_nodes) return NKV_ERR_INVALID;
    return st(launch_leaf_strided(static_cast<const uint8_t*>(d_base), stride, len, n,
                                  c->leaf_load, static_cast<uint8_t*>(d_nodes), c->stream));
} NKV_CATCH

int nkv_tree_reduce_dev(nkv_ctx* c, void* d_nodes, uint64_t n) try {
    TRY(bind(c));
    if (n > kMaxN) return NKV_ERR_INVALID;
    if (n == 0) return NKV_ERR_EMPTY;
    if (!d_nodes) return NKV_ERR_INVALID;
    return st(launch_reduce(static_cast<uint8_t*>(d_nodes), n, 0, levels_of(n) - 1, c->stream));
} NKV_CATCH

int nkv_tree_from_values_dev(nkv_ctx* c, const void* d_base, const uint64_t* d_off,
                             const uint64_t* d_len, uint64_t n, void* d_nodes) try {
    TRY(bind(c));
    if (n > kMaxN) return NKV_ERR_INVALID;
    if (n == 0) return NKV_ERR_EMPTY;
    if (!d_base || !d_off || !d_len || !d_nodes) return NKV_ERR_INVALID;
    return tree_from_device_values(c, static_cast<const uint8_t*>(d_base), d_off, d_len, n, false,
                                   static_cast<uint8_t*>(d_nodes));
} NKV_CATCH

int nkv_tree_from_strided_dev(nkv_ctx* c, const void* d_base, uint64_t stride, uint64_t len,
                              uint64_t n, void* d_nodes) try {
    TRY(bind(c));
    if (n > kMaxN) return NKV_ERR_INVALID;
    if (n == 0) return NKV_ERR_EMPTY;
    if (!d_base || !d_nodes) return NKV_ERR_INVALID;
    uint8_t* nodes = static_cast<uint8_t*>(d_nodes);
    TRY(mark(c, 0));
    HIPTRY(launch_leaf_strided(static_cast<const uint8_t*>(d_base), stride, len, n,
                               c->leaf_load, nodes, c->stream));
    return levels_above(c, nodes, n);
} NKV_CATCH

int nkv_bfs_image_dev(nkv_ctx* c, const void* d_nodes, uint64_t n, void* d_img) try {
    TRY(bind(c));
    if (n > kMaxN) return NKV_ERR_INVALID;
    if (n == 0) return NKV_ERR_EMPTY;
    if (!d_nodes || !d_img) return NKV_ERR_INVALID;
    BfsLayout lay = layout_of(counts_of(n));
    return st(launch_bfs_image(static_cast<const uint8_t*>(d_nodes), lay,
                               static_cast<uint8_t*>(d_img), c->stream));
} NKV_CATCH

int nkv_record_offsets_dev(nkv_ctx* c, const uint64_t* d_rec_size, uint64_t n,
                           uint64_t* d_rec_off) try {
    TRY(bind(c));
    if (n > kMaxN) return NKV_ERR_INVALID;
    if (n == 0) return NKV_OK;
    if (!d_rec_size || !d_rec_off || n > 0x7fffffffull) return NKV_ERR_INVALID;
    size_t tb = 0;
    HIPTRY(scan_exclusive_u64(d_rec_size, d_rec_off, n, nullptr, &tb, c->stream));
    TRY(grow(c->d_tmp, tb));
    return st(scan_exclusive_u64(d_rec_size, d_rec_off, n, c->d_tmp.p, &tb, c->stream));
} NKV_CATCH

int nkv_locate_values_dev(nkv_ctx* c, const void* d_stream, uint64_t stream_len,
                          const uint64_t* d_rec_off, uint64_t n, uint64_t* d_voff,
                          uint64_t* d_vlen) try {
    TRY(bind(c));
    if (n > kMaxN) return NKV_ERR_INVALID;
    if (n == 0) return NKV_OK;
    if (!d_stream || !d_rec_off || !d_voff || !d_vlen) return NKV_ERR_INVALID;
    TRY(grow(c->d_err, 4));
    unsigned int* err = static_cast<unsigned int*>(c->d_err.p);
    uint32_t* part = nullptr;
    TRY(locate_parts(c, n, &part));
    HIPTRY(launch_locate(static_cast<const uint8_t*>(d_stream), stream_len, d_rec_off, n, d_voff,
                         d_vlen, err, nullptr, part, c->stream));
    return read_verdict(c, err);
} NKV_CATCH

int nkv_tree_from_records_dev(nkv_ctx* c, const void* d_stream, uint64_t stream_len, const uint64_t* d_rec_off,
                              uint64_t n, void* d_nodes, uint32_t* d_err) try {
    TRY(bind(c));
    if (n > kMaxN) return NKV_ERR_INVALID;
    if (n == 0) return NKV_ERR_EMPTY;
    if (!d_stream || !d_rec_off || !d_nodes) return NKV_ERR_INVALID;
    unsigned int* err = reinterpret_cast<unsigned int*>(d_err);
    if (!err) {
        TRY(grow(c->d_err, 4));
        err = static_cast<unsigned int*>(c->d_err.p);
    }
    TRY(records_tree(c, static_cast<const uint8_t*>(d_stream), stream_len, d_rec_off, n,
                     static_cast<uint8_t*>(d_nodes), err));
    if (d_err) return NKV_OK;
    return read_verdict(c, err);
} NKV_CATCH

// Compaction read in one pass: the Merkle tree of the records' Values and the
// check of every record's Crc.  k_leaf_verify parses the headers, checks every
// Crc and hashes the waves whose value sizes are narrow (the range rule of
// plan_of), reading each record once for both; it defers ragged waves (after
// their checksums) to the length-sorted leaf pass behind a device Gate, as
// records_tree does.
int nkv_tree_verify_records_dev(nkv_ctx* c, const void* d_stream, uint64_t stream_len, const uint64_t* d_rec_off,
                                uint64_t n, void* d_nodes, uint32_t* d_crc, uint64_t* d_stats) try {
    TRY(bind(c));
    if (n > kMaxN) return NKV_ERR_INVALID;
    if (n == 0) return NKV_ERR_EMPTY;
    if (!d_stream || !d_rec_off || !d_nodes) return NKV_ERR_INVALID;
    const uint8_t* stream = static_cast<const uint8_t*>(d_stream);
    uint8_t* nodes = static_cast<uint8_t*>(d_nodes);
    unsigned long long* stats = reinterpret_cast<unsigned long long*>(d_stats);
    if (!stats) {
        TRY(grow(c->d_stats, 24));
        stats = static_cast<unsigned long long*>(c->d_stats.p);
    }
    const Plan plan = batch_plan(c, n);
    if (plan == kInputOrder) {  // else the stats start in the pass flags (reset by the previous call)
        HIPTRY(hipMemsetAsync(stats, 0, 24, c->stream));
        HIPTRY(hipMemsetAsync(stats + 1, 0xFF, 8, c->stream));
    }
    RecordsScratch s;
    TRY(records_scratch(c, n, &s));
    TRY(mark(c, 0));
    if (plan == kInputOrder) {
        HIPTRY(launch_leaf_verify(stream, stream_len, d_rec_off, n, 0, s.voff, s.vlen, nodes, d_crc, stats, s.range,
                                  s.part, c->stream));
    } else {  // as records_tree: the pass flags, the stats copied out by the sort's first launch
        uint32_t *flags, *next;
        pass_flags(c, &flags, &next);
        HIPTRY(launch_leaf_verify(stream, stream_len, d_rec_off, n, policy_of(plan), s.voff, s.vlen, nodes, d_crc,
                                  stats, nullptr, nullptr, c->stream, flags, next));
        flip_pass_flags(c);
        TRY(leaf_level(c, stream, s.voff, s.vlen, n, false, nodes, plan, Gate{flags, 0}, false,
                       CopyWords{flags + 4, reinterpret_cast<uint32_t*>(stats), 6}));
    }
    return levels_above(c, nodes, n);
} NKV_CATCH

}  // extern "C"
