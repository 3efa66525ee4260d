#!/usr/bin/env python3
"""Batched point lookup over device-resident tables (nkv_lookup_dev) and the
gather of the found Values (nkv_lookup_values_dev): T = 4 tables of 1 Mi
records (a 16-B key, a 100-B value) each, q = 1 Mi keys per call.

The key mix, shuffled: half present (spread evenly over the tables, so a key of
table t is first refused by the filters of the tables in front of it), a
quarter absent but in range and passed by every filter (they end at INDEX in
all four tables: the full binary search four times), a quarter absent and
rejected by the filters (but for their 1 % of false positives).  Absent keys
are drawn like the tables' own, so all but a few per table are in range.  To
get the second kind on purpose, its keys are inserted into every table's filter
next to the table's own keys (the filters are sized for both,
bloomfilter.New(n + q / 4, 0.01)); the filters are built on the device
(nkv_bloom_insert_records_dev, nkv_bloom_insert_dev).

Prints one JSON line and writes it to profiles/lookup_bench.json.  In one run
of --steps calls after --warmup:
  lookup_ms        nkv_lookup_dev with d_stage and d_err given (no host sync
                   inside), device events around the call
  keys_per_s       q / lookup_ms
  cpu_s            the same batch over the same tables in host memory: 16
                   threads of std::lower_bound (tools/cpu_lookup.cpp, built here
                   with g++), the best of three runs; cpu_keys_per_s = q / cpu_s
  gather_call_ms   nkv_lookup_values_dev, host wall clock around the call (it
                   synchronizes once for the length) and a synchronize
  copy_ms          the copy of the q + 1 offsets and the copy kernel, from the
                   context's events (measure_ms: the measure kernel, the scan and
                   the host's read of the length in front of them)
  copy_gbs         out_len bytes written / copy_ms
  memcpy_ms        hipMemcpyDtoDAsync of out_len bytes in the same process;
                   memcpy_gbs the same bytes / memcpy_ms, and
                   copy_vs_memcpy = copy_gbs / memcpy_gbs
  sclk_mhz_after   the shader clock the box reports right after the timed loops
Before the figures are kept, the device's hits are compared with the host
search's, every stage row with what the mix implies, and the gathered bytes
and offsets with a numpy gather over the host copy of the tables.
"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import benchlib  # noqa: E402
from benchlib import keys_of  # noqa: E402
from nakevaleng_amd import _lib  # noqa: E402

KS, VS, T = 16, 100, 4
RB = 30 + KS + VS


def cpu_lib():
    vp = ctypes.c_void_p
    return benchlib.build_cpu("lookup", {"cpu_lookup": (ctypes.c_double, [vp, vp, vp, ctypes.c_int, vp, vp, vp,
                                                                          ctypes.c_uint64, vp, ctypes.c_int])},
                              ["-pthread"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--scale", type=int, default=1, help="divide the record and query counts (a quick look)")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lookup_bench.json"))
    args = ap.parse_args()
    n = q = (1 << 20) // args.scale
    cpu = cpu_lib()
    L, ctx, s = benchlib.open_ctx()
    rng = np.random.default_rng(0x6C6B7570)

    # the tables and the queries, on the host
    recs, us = zip(*[benchlib.host_table(rng, n, VS) for _ in range(T)])
    off = np.arange(n, dtype=np.uint64) * np.uint64(RB)
    kind = rng.permutation(np.repeat(np.arange(4), q // 4))  # 0, 1: present; 2: passes the filters; 3: rejected
    tq, jq = rng.integers(0, T, q), rng.integers(0, n, q)
    uq = rng.integers(0, 2**63, q, dtype=np.uint64)  # absent: drawn like the tables' keys, so in range but for a few
    for t in range(T):
        uq[(kind < 2) & (tq == t)] = us[t][jq[(kind < 2) & (tq == t)]]
    qkeys = keys_of(uq)
    koff, klen = np.arange(q, dtype=np.uint64) * np.uint64(KS), np.full(q, KS, np.uint64)
    passed = np.ascontiguousarray(qkeys[kind == 2])

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()

    # the tables and their filters on the device
    m, k = ctypes.c_uint32(0), ctypes.c_uint32(0)
    _lib.check(L.nkv_bloom_params(n + passed.shape[0], 0.01, ctypes.byref(m), ctypes.byref(k)))
    d_off, d_passed = dev(off), dev(passed)
    d_poff, d_plen = dev(koff[:passed.shape[0]]), dev(klen[:passed.shape[0]])
    tabs = (_lib.NkvLookupTable * T)()
    keep = []
    for t in range(T):
        d_rec = dev(recs[t])
        d_bits = torch.zeros(((m.value + 31) // 32) * 4, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        _lib.check(L.nkv_bloom_insert_records_dev(ctx.h, d_rec.data_ptr(), n * RB, d_off.data_ptr(), n, m.value,
                                                  k.value, 1000 + t, d_bits.data_ptr()))
        _lib.check(L.nkv_bloom_insert_dev(ctx.h, d_passed.data_ptr(), d_poff.data_ptr(), d_plen.data_ptr(),
                                          passed.shape[0], m.value, k.value, 1000 + t, d_bits.data_ptr()))
        tabs[t] = _lib.NkvLookupTable(d_rec.data_ptr(), n * RB, d_off.data_ptr(), n, d_bits.data_ptr(), m.value,
                                      k.value, 1000 + t)
        keep += [d_rec, d_bits]
    d_keys, d_koff, d_klen = dev(qkeys), dev(koff), dev(klen)
    d_hit = torch.zeros(q, dtype=torch.int64, device="cuda")
    d_status = torch.zeros(q, dtype=torch.uint8, device="cuda")
    d_stage = torch.zeros(q * T, dtype=torch.uint8, device="cuda")
    d_err = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def lookup():
        _lib.check(L.nkv_lookup_dev(ctx.h, tabs, T, d_keys.data_ptr(), d_koff.data_ptr(), d_klen.data_ptr(), q,
                                    d_hit.data_ptr(), d_status.data_ptr(), d_stage.data_ptr(), d_err.data_ptr()))

    lookup_ms = benchlib.event_ms(s, lookup, args.warmup, args.steps)
    clock_lookup = benchlib.sclk()

    # the gather
    out_len = ctypes.c_uint64(0)
    vargs = (ctx.h, tabs, T, d_hit.data_ptr(), d_status.data_ptr(), q)
    _lib.check(L.nkv_lookup_values_dev(*vargs, None, 0, None, ctypes.byref(out_len)))
    nb = out_len.value
    d_out = torch.empty(nb, dtype=torch.uint8, device="cuda")
    d_out_off = torch.zeros(q + 1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    def gather():
        _lib.check(L.nkv_lookup_values_dev(*vargs, d_out.data_ptr(), nb, d_out_off.data_ptr(), ctypes.byref(out_len)))
        torch.cuda.synchronize()

    call_ms, measure_ms, copy_ms = benchlib.phase_ms(ctx, gather, args.warmup, args.steps)

    # the comparator: hipMemcpyDtoDAsync of as many bytes as the gather writes
    d_src = torch.empty(nb, dtype=torch.uint8, device="cuda")
    d_dst = torch.empty(nb, dtype=torch.uint8, device="cuda")
    memcpy_ms = benchlib.memcpy_ms(s, d_dst, d_src, nb, args.warmup, args.steps)
    clock = benchlib.sclk()
    del d_src, d_dst

    # the host search over the same tables, and the checks
    streams = (ctypes.c_void_p * T)(*[r.ctypes.data for r in recs])
    offs = (ctypes.c_void_p * T)(*[off.ctypes.data] * T)
    ns = np.full(T, n, np.uint64)
    h_hit = np.empty(q, np.uint64)
    cpu_s = min(cpu.cpu_lookup(streams, offs, ns.ctypes.data, T, qkeys.ctypes.data, koff.ctypes.data,
                               klen.ctypes.data, q, h_hit.ctypes.data, args.threads) for _ in range(3))
    hit = d_hit.cpu().numpy().view(np.uint64)
    stage = d_stage.cpu().numpy().reshape(q, T)
    present = kind < 2
    ok = int(d_err.cpu().numpy()[0]) == 0 and np.array_equal(hit, h_hit)
    ok = ok and np.array_equal(hit[present], (tq[present].astype(np.uint64) << np.uint64(32)) | jq[present].astype(np.uint64))
    ok = ok and (hit[~present] == _lib.NKV_HIT_NONE).all()
    # absent keys are in range but for the few below a table's first key or above its last
    absent_ends = (_lib.NKV_STAGE_FILTER, _lib.NKV_STAGE_SUMMARY, _lib.NKV_STAGE_INDEX)
    ok = ok and np.isin(stage[kind == 2], absent_ends[1:]).all()  # passed by every filter
    ok = ok and np.isin(stage[kind == 3], absent_ends).all()
    searched = float((stage[kind == 2] == _lib.NKV_STAGE_INDEX).mean())
    rejected = float((stage[kind == 3] == _lib.NKV_STAGE_FILTER).mean())
    found_col = np.take_along_axis(stage[present], tq[present][:, None], 1)[:, 0]
    ok = ok and (found_col == _lib.NKV_STAGE_FOUND).all()
    want_len = np.where(present, VS, 0).astype(np.uint64)
    want_off = np.concatenate([[0], np.cumsum(want_len)]).astype(np.uint64)
    ok = ok and nb == int(want_off[-1]) and np.array_equal(d_out_off.cpu().numpy().view(np.uint64), want_off)
    idx = np.flatnonzero(present)  # the LIVE queries, in the order their Values are packed
    want = np.empty((idx.size, VS), np.uint8)
    for t in range(T):
        sel = tq[idx] == t
        want[sel] = recs[t][jq[idx][sel], 30 + KS:]
    ok = ok and np.array_equal(d_out.cpu().numpy().reshape(-1, VS), want)
    if not ok:
        raise SystemExit("bench_lookup: the device's hits, stages or Values differ from the host's")

    out = {"metric": "batched point lookup over device-resident tables", "tables": T, "records_per_table": n,
           "key_bytes": KS, "value_bytes": VS, "queries": q, "filter_bits": m.value, "filter_hashes": k.value,
           "mix": {"present": int(present.sum()), "absent_in_range_passing_every_filter": int((kind == 2).sum()),
                   "absent_random": int((kind == 3).sum()),
                   "searched_to_index_per_table_of_the_passing": round(searched, 6),
                   "rejected_by_the_filter_per_table_of_the_random": round(rejected, 4)},
           "steps": args.steps, "warmup": args.warmup}
    lookup_med = benchlib.put(out, "lookup_ms", lookup_ms, 3)
    out.update({"keys_per_s": round(q / (lookup_med * 1e-3)),
                "cpu_threads": args.threads, "cpu_s": round(cpu_s, 4), "cpu_keys_per_s": round(q / cpu_s),
                "lookup_speedup_vs_cpu": round(cpu_s * 1e3 / lookup_med, 1),
                "sclk_mhz_after_lookup": clock_lookup, "gather_bytes": nb})
    benchlib.put(out, "gather_call_ms", call_ms, 3)
    benchlib.put(out, "measure_ms", measure_ms, 3)
    copy_gbs = nb / (benchlib.put(out, "copy_ms", copy_ms, 3) * 1e-3) / 1e9
    memcpy_gbs = nb / (benchlib.put(out, "memcpy_ms", memcpy_ms, 3) * 1e-3) / 1e9
    out.update({"copy_gbs": round(copy_gbs, 1), "memcpy_gbs": round(memcpy_gbs, 1),
                "copy_vs_memcpy": round(copy_gbs / memcpy_gbs, 3),
                "sclk_mhz_after": clock, "verified_vs_host_search_and_gather": True})
    benchlib.emit(out, args.out)
    ctx.close()


if __name__ == "__main__":
    main()
