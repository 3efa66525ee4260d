#!/usr/bin/env python3
"""The Index/Summary readers on the device: nkv_index_open_dev (parse and
validate one pair) and nkv_locate_dev (the batched search over opened tables).

Open.  One table of 1 Mi Index entries with 16-byte keys, its Summary written
at page sizes 3 and 1,024.  Per page size, the median host wall clock of the
(synchronous) call over --open-steps calls after --open-warmup:
  walk_ms          NKV_OPT_INDEX_OPEN_PATH 1: one lane follows the Summary
  chunked_ms       path 2 at the default bytes per lane; chunk_sweep_ms the same
                   at every NKV_OPT_INDEX_OPEN_CHUNK of --chunks
  auto_ms          path 0
  cpu_walk_ms      one host thread walking the same two images
                   (tools/cpu_locate.cpp cpu_index_walk), the best of three
and size_sweep: walk_ms and chunked_ms for tables of 2^8 .. 2^18 entries at
page size 3, with each payload's bytes -- the auto switch is chosen from where
the two cross.  Every open's entry offsets, n and s are checked.

Locate.  T = 4 opened tables of 1 Mi entries, q = 1 Mi keys per call in
tools/bench_lookup.py's mix (half present, a quarter absent but passed by every
filter, a quarter absent and rejected), device events around the call:
  locate_ms        nkv_locate_dev with d_stage and d_err given
  lookup_ms        nkv_lookup_dev over the same four tables resident as Data
                   streams of 146-byte records: the same question answered the
                   way the library answered it before
  cpu_s            16 threads of std::lower_bound over the parsed Index images
                   in host memory (tools/cpu_locate.cpp cpu_locate), best of three
The hits and Data offsets are checked against the host search and the mix.

Prints one JSON line and writes it to profiles/locate_bench.json.
"""
import argparse
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import benchlib  # noqa: E402
from benchlib import keys_of  # noqa: E402
from nakevaleng_amd import _lib  # noqa: E402

KS, VS, T = 16, 100, 4
RB = 30 + KS + VS  # 146
EB = 16 + KS       # bytes per Index entry


def cpu_lib():
    vp, u64, dbl = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_double
    return benchlib.build_cpu("locate", {"cpu_index_walk": (dbl, [vp, u64, vp, u64, vp, vp, vp]),
                                         "cpu_locate": (dbl, [vp, vp, vp, ctypes.c_int, vp, vp, vp, u64, vp, vp,
                                                              ctypes.c_int])}, ["-pthread"])


def entries(keys, field):
    """KeySize | field | Key per row."""
    e = np.empty((keys.shape[0], EB), np.uint8)
    e[:, :8] = np.frombuffer(np.uint64(KS).tobytes(), np.uint8)
    e[:, 8:16] = np.ascontiguousarray(field, dtype="<i8").view(np.uint8).reshape(-1, 8)
    e[:, 16:] = keys
    return e


def pair_of(keys, page):
    """(Index, Summary) of makeIndexAndSummary over records of RB bytes."""
    n = keys.shape[0]
    index = entries(keys, np.arange(n, dtype=np.int64) * RB)
    sel = np.unique(np.concatenate([np.arange(0, n, page), [n - 1]]))
    payload = entries(keys[sel], sel.astype(np.int64) * EB)
    head = np.concatenate([np.asarray([KS, KS, payload.size], "<u8").view(np.uint8), keys[0], keys[-1]])
    return index.reshape(-1), np.concatenate([head, payload.reshape(-1)]), int(sel.size)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()


def time_open(L, ctx, d_index, d_summary, d_ent, n, s, path, chunk, steps, warmup):
    gn, gs, v = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint32(0)
    ctx.set_option(_lib.NKV_OPT_INDEX_OPEN_PATH, path)
    ctx.set_option(_lib.NKV_OPT_INDEX_OPEN_CHUNK, chunk)
    ms = []
    for it in range(warmup + steps):
        d_ent.zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _lib.check(L.nkv_index_open_dev(ctx.h, d_index.data_ptr(), d_index.numel(), d_summary.data_ptr(),
                                        d_summary.numel(), d_ent.data_ptr(), n, ctypes.byref(gn), ctypes.byref(gs),
                                        ctypes.byref(v)))
        if it >= warmup:
            ms.append((time.perf_counter() - t0) * 1e3)
    ctx.set_option(_lib.NKV_OPT_INDEX_OPEN_PATH, 0)
    ctx.set_option(_lib.NKV_OPT_INDEX_OPEN_CHUNK, 0)
    ent = d_ent.cpu().numpy().view(np.uint64)[:n]
    if (gn.value, gs.value, v.value) != (n, s, 0) or not np.array_equal(ent, np.arange(n, dtype=np.uint64) * EB):
        raise SystemExit(f"bench_locate: open (path {path}, chunk {chunk}) differs from the images")
    return round(benchlib.median(ms), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--open-steps", type=int, default=5)
    ap.add_argument("--open-warmup", type=int, default=2)
    ap.add_argument("--chunks", default="256,1024,4096,16384,65536")
    ap.add_argument("--scale", type=int, default=1, help="divide the entry and query counts (a quick look)")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "locate_bench.json"))
    args = ap.parse_args()
    n = q = (1 << 20) // args.scale
    chunks = [int(c) for c in args.chunks.split(",")]
    cpu = cpu_lib()
    L, ctx, s = benchlib.open_ctx()
    rng = np.random.default_rng(0x6C6F6361)

    us = [benchlib.distinct_u64(rng, n) for _ in range(T)]
    keys = [keys_of(u) for u in us]

    # ---- open
    opens = {}
    for page in (3, 1024):
        index, summary, sn = pair_of(keys[0], page)
        d_index, d_summary = dev(index), dev(summary)
        d_ent = torch.zeros(8 * n, dtype=torch.uint8, device="cuda")
        one = lambda path, chunk=0: time_open(L, ctx, d_index, d_summary, d_ent, n, sn, path, chunk,  # noqa: E731
                                              args.open_steps, args.open_warmup)
        h_ent = np.zeros(n, np.uint64)
        hn, hs = ctypes.c_uint64(0), ctypes.c_uint64(0)
        cpu_s = min(cpu.cpu_index_walk(index.ctypes.data, index.size, summary.ctypes.data, summary.size,
                                       h_ent.ctypes.data, ctypes.byref(hn), ctypes.byref(hs)) for _ in range(3))
        assert (hn.value, hs.value) == (n, sn)
        opens[f"page_{page}"] = {"summary_entries": sn, "payload_bytes": int(sn * EB), "walk_ms": one(1),
                                 "chunked_ms": one(2), "auto_ms": one(0),
                                 "chunk_sweep_ms": {str(c): one(2, c) for c in chunks},
                                 "cpu_walk_ms": round(cpu_s * 1e3, 3)}
    sweep = {}
    for lg in range(8, 20, 2):
        m = min(1 << lg, n)
        index, summary, sn = pair_of(keys[0][:m], 3)
        d_index, d_summary = dev(index), dev(summary)
        d_ent = torch.zeros(8 * m, dtype=torch.uint8, device="cuda")
        sweep[str(m)] = {"payload_bytes": int(sn * EB),
                         "walk_ms": time_open(L, ctx, d_index, d_summary, d_ent, m, sn, 1, 0, args.open_steps,
                                              args.open_warmup),
                         "chunked_ms": time_open(L, ctx, d_index, d_summary, d_ent, m, sn, 2, 0, args.open_steps,
                                                 args.open_warmup)}
    clock_open = benchlib.sclk()

    # ---- locate: the queries
    kind = rng.permutation(np.repeat(np.arange(4), q // 4))  # 0, 1: present; 2: passes the filters; 3: rejected
    tq, jq = rng.integers(0, T, q), rng.integers(0, n, q)
    uq = rng.integers(0, 2**63, q, dtype=np.uint64)
    for t in range(T):
        uq[(kind < 2) & (tq == t)] = us[t][jq[(kind < 2) & (tq == t)]]
    qkeys = keys_of(uq)
    koff, klen = np.arange(q, dtype=np.uint64) * np.uint64(KS), np.full(q, KS, np.uint64)
    passed = np.ascontiguousarray(qkeys[kind == 2])

    # the tables: resident Data streams (for nkv_lookup_dev and the filters), and their opened Index images
    m, k = ctypes.c_uint32(0), ctypes.c_uint32(0)
    _lib.check(L.nkv_bloom_params(n + passed.shape[0], 0.01, ctypes.byref(m), ctypes.byref(k)))
    off = np.arange(n, dtype=np.uint64) * np.uint64(RB)
    d_off, d_passed = dev(off), dev(passed)
    d_poff, d_plen = dev(koff[:passed.shape[0]]), dev(klen[:passed.shape[0]])
    rtabs, itabs, keep, h_index = (_lib.NkvLookupTable * T)(), (_lib.NkvIndexTable * T)(), [], []
    gn, gs, v = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint32(0)
    for t in range(T):
        d_rec = dev(benchlib.host_records(keys[t], VS))
        d_bits = torch.zeros(((m.value + 31) // 32) * 4, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        _lib.check(L.nkv_bloom_insert_records_dev(ctx.h, d_rec.data_ptr(), n * RB, d_off.data_ptr(), n, m.value,
                                                  k.value, 1000 + t, d_bits.data_ptr()))
        _lib.check(L.nkv_bloom_insert_dev(ctx.h, d_passed.data_ptr(), d_poff.data_ptr(), d_plen.data_ptr(),
                                          passed.shape[0], m.value, k.value, 1000 + t, d_bits.data_ptr()))
        index, summary, sn = pair_of(keys[t], 3)
        d_index, d_summary = dev(index), dev(summary)
        d_ent = torch.zeros(8 * n, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        _lib.check(L.nkv_index_open_dev(ctx.h, d_index.data_ptr(), index.size, d_summary.data_ptr(), summary.size,
                                        d_ent.data_ptr(), n, ctypes.byref(gn), ctypes.byref(gs), ctypes.byref(v)))
        assert (gn.value, gs.value, v.value) == (n, sn, 0)
        rtabs[t] = _lib.NkvLookupTable(d_rec.data_ptr(), n * RB, d_off.data_ptr(), n, d_bits.data_ptr(), m.value,
                                       k.value, 1000 + t)
        itabs[t] = _lib.NkvIndexTable(d_index.data_ptr(), index.size, d_ent.data_ptr(), n, d_bits.data_ptr(),
                                      m.value, k.value, 1000 + t)
        keep += [d_rec, d_bits, d_index, d_ent]
        h_index.append(index)
    d_keys, d_koff, d_klen = dev(qkeys), dev(koff), dev(klen)
    out2 = [torch.zeros(q, dtype=torch.int64, device="cuda") for _ in range(3)]  # hit, data_off; lookup's hit
    st2 = [torch.zeros(q, dtype=torch.uint8, device="cuda") for _ in range(2)]
    d_stage = torch.zeros(q * T, dtype=torch.uint8, device="cuda")
    d_err = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def locate():
        _lib.check(L.nkv_locate_dev(ctx.h, itabs, T, 0, d_keys.data_ptr(), d_koff.data_ptr(), d_klen.data_ptr(), q, 0,
                                    out2[0].data_ptr(), out2[1].data_ptr(), st2[0].data_ptr(), d_stage.data_ptr(),
                                    d_err.data_ptr()))

    def lookup():
        _lib.check(L.nkv_lookup_dev(ctx.h, rtabs, T, d_keys.data_ptr(), d_koff.data_ptr(), d_klen.data_ptr(), q,
                                    out2[2].data_ptr(), st2[1].data_ptr(), d_stage.data_ptr(), d_err.data_ptr()))

    # the two alternate call by call, so both see the same clocks
    locate_ms, lookup_ms = benchlib.alternating_ms(s, (locate, lookup), args.warmup, args.steps)
    clock = benchlib.sclk()
    locate()
    torch.cuda.synchronize()

    # the host search, and the checks
    idx_p = (ctypes.c_void_p * T)(*[a.ctypes.data for a in h_index])
    ent = np.arange(n, dtype=np.uint64) * np.uint64(EB)
    off_p = (ctypes.c_void_p * T)(*[ent.ctypes.data] * T)
    ns = np.full(T, n, np.uint64)
    h_hit, h_off = np.empty(q, np.uint64), np.empty(q, np.int64)
    cpu_s = min(cpu.cpu_locate(idx_p, off_p, ns.ctypes.data, T, qkeys.ctypes.data, koff.ctypes.data,
                               klen.ctypes.data, q, h_hit.ctypes.data, h_off.ctypes.data, args.threads)
                for _ in range(3))
    hit, data_off = out2[0].cpu().numpy().view(np.uint64), out2[1].cpu().numpy()
    present = kind < 2
    ok = int(d_err.cpu().numpy()[0]) == 0 and np.array_equal(hit, h_hit) and np.array_equal(data_off, h_off)
    ok = ok and np.array_equal(hit, out2[2].cpu().numpy().view(np.uint64))  # the resident lookup names the same entries
    ok = ok and np.array_equal(hit[present], (tq[present].astype(np.uint64) << np.uint64(32)) | jq[present].astype(np.uint64))
    ok = ok and np.array_equal(data_off[present], jq[present] * RB) and (hit[~present] == _lib.NKV_HIT_NONE).all()
    ok = ok and (st2[0].cpu().numpy()[present] == _lib.NKV_GET_LOCATED).all()
    if not ok:
        raise SystemExit("bench_locate: the device's hits or Data offsets differ from the host's")

    loc = {"tables": T, "queries": q, "filter_bits": m.value, "filter_hashes": k.value,
           "index_bytes_per_table": int(n * EB), "data_bytes_per_table": int(n * RB),
           "steps": args.steps, "warmup": args.warmup}
    locate_med = benchlib.put(loc, "locate_ms", locate_ms, 3)
    lookup_med = benchlib.put(loc, "lookup_ms", lookup_ms, 3)
    loc.update({"locate_keys_per_s": round(q / (locate_med * 1e-3)),
                "lookup_keys_per_s": round(q / (lookup_med * 1e-3)),
                "locate_vs_lookup": round(lookup_med / locate_med, 3),
                "cpu_threads": args.threads, "cpu_s": round(cpu_s, 4), "cpu_keys_per_s": round(q / cpu_s),
                "locate_speedup_vs_cpu": round(cpu_s * 1e3 / locate_med, 1),
                "sclk_mhz_after": clock, "verified_vs_host_search": True})
    out = {"metric": "Index/Summary readers on the device", "key_bytes": KS, "entries_per_table": n,
           "open": opens, "open_size_sweep_page_3": sweep, "open_steps": args.open_steps,
           "sclk_mhz_after_open": clock_open, "locate": loc}
    benchlib.emit(out, args.out)
    ctx.close()


if __name__ == "__main__":
    main()
