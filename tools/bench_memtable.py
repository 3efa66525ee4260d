#!/usr/bin/env python3
"""The live memtable on the device (nkv_memtable_add_dev / nkv_memtable_find_dev)
at 1 Mi writes of 146-byte records (16-byte keys, 100-byte Values), three key
mixes:
  distinct   every write a new key
  sixteenth  1/16 of that many distinct keys, drawn uniformly
  single     one key written 1 Mi times (every lane on one slot)

Per mix one JSON line, all of them in profiles/memtable_bench.json.  Every time
is the median of --steps device-event intervals on the context's stream after
--warmup untimed rounds (the index is cleared, untimed, in front of every add):
  add_ms / find_ms         the index: one add of all the writes into 2 Mi slots;
                           one find of 1 Mi keys (the writes' keys, shuffled)
  sort_ms / lookup_ms      the route the flush and the table lookup already
                           give to the same answers: nkv_sort_records_dev over
                           the log, and nkv_lookup_dev of the same keys over
                           the flushed table (one table, no filter)
  cpu1_* / cpu16_*         tools/cpu_memtable.cpp on this box: one
                           std::unordered_map, and 16 threads sharded by hash
  *_vs_*                   comparator time / index time (above 1: the index wins)
Before any timing counts the device's is_new, state, hits and statuses are held
to a numpy result, and the host program's to the same.
"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import benchlib  # noqa: E402

N, KS, VS = 1 << 20, 16, 100
RB = 30 + KS + VS
MIXES = {"distinct": N, "sixteenth": N // 16, "single": 1}
NONE = 2**64 - 1


def cpu_lib():
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    return benchlib.build_cpu("memtable", {"cpu_memtable": (None, [vp, vp, u64, ctypes.c_int, vp, vp, vp, u64, vp, vp,
                                                                   vp, vp])}, ["-pthread"])


def host_answers(which, n):
    """is_new and the latest write of every write's key, from the key ids."""
    _, first, inverse = np.unique(which, return_index=True, return_inverse=True)
    is_new = np.zeros(n, np.uint8)
    is_new[first] = 1
    last = np.zeros(first.size, np.int64)
    np.maximum.at(last, inverse, np.arange(n))
    return is_new, last[inverse].astype(np.uint64)


def run_mix(name, args, cpu):
    import torch
    from nakevaleng_amd import _lib
    n = args.records
    distinct = max(1, MIXES[name] * n // N)
    rng = np.random.default_rng(0x6D656D74 + len(name))
    L, ctx, s = benchlib.open_ctx()
    uniq = rng.integers(0, 256, (distinct, KS), dtype=np.uint8)
    assert np.unique(uniq, axis=0).shape[0] == distinct
    which = np.arange(n) if distinct == n else rng.integers(0, distinct, n)
    distinct = int(np.unique(which).size)  # a uniform draw may miss a key
    keys = uniq[which]
    total = n * RB
    d_log = benchlib.device_log(ctx, n, KS, VS, keys)
    d_log.view(n, RB)[:, 12] = 0  # Status: all live
    d_roff = torch.arange(n, dtype=torch.int64, device="cuda") * RB
    slots = 2
    while slots < 2 * n:
        slots *= 2
    d_index = torch.empty(8 * slots, dtype=torch.uint8, device="cuda")
    d_state = torch.empty(32, dtype=torch.uint8, device="cuda")
    d_new = torch.empty(n, dtype=torch.uint8, device="cuda")
    d_err = torch.zeros(4, dtype=torch.uint8, device="cuda")
    perm = rng.permutation(n)
    d_keys = torch.from_numpy(np.ascontiguousarray(keys[perm])).cuda()
    d_koff = torch.arange(n, dtype=torch.int64, device="cuda") * KS
    d_klen = torch.full((n,), KS, dtype=torch.int64, device="cuda")
    d_hit = torch.empty(8 * n, dtype=torch.uint8, device="cuda")
    d_status = torch.empty(n, dtype=torch.uint8, device="cuda")
    d_out = torch.empty(total, dtype=torch.uint8, device="cuda")
    d_ooff = torch.empty(8 * n, dtype=torch.uint8, device="cuda")
    n_out, out_len = ctypes.c_uint64(0), ctypes.c_uint64(0)

    def clear():
        _lib.check(L.nkv_memtable_clear_dev(ctx.h, d_index.data_ptr(), slots, d_state.data_ptr()))

    def add():
        _lib.check(L.nkv_memtable_add_dev(ctx.h, d_log.data_ptr(), total, d_roff.data_ptr(), 0, n, d_index.data_ptr(),
                                          slots, 3, 10, 1 << 62, d_state.data_ptr(), d_new.data_ptr(),
                                          d_err.data_ptr()))

    def find():
        _lib.check(L.nkv_memtable_find_dev(ctx.h, d_log.data_ptr(), total, d_roff.data_ptr(), n, d_index.data_ptr(),
                                           slots, d_keys.data_ptr(), d_koff.data_ptr(), d_klen.data_ptr(), n, 0, 0,
                                           d_hit.data_ptr(), d_status.data_ptr(), d_err.data_ptr()))

    def sort():
        _lib.check(L.nkv_sort_records_dev(ctx.h, d_log.data_ptr(), total, d_roff.data_ptr(), n, d_out.data_ptr(),
                                          total, d_ooff.data_ptr(), None, ctypes.byref(n_out), ctypes.byref(out_len)))

    def lookup():
        tab = (_lib.NkvLookupTable * 1)(_lib.NkvLookupTable(d_out.data_ptr(), out_len.value, d_ooff.data_ptr(),
                                                           n_out.value, None, 0, 0, 0))
        _lib.check(L.nkv_lookup_dev(ctx.h, tab, 1, d_keys.data_ptr(), d_koff.data_ptr(), d_klen.data_ptr(), n,
                                    d_hit.data_ptr(), d_status.data_ptr(), None, d_err.data_ptr()))

    # verify before any timing counts
    want_new, want_latest = host_answers(which, n)
    clear()
    add()
    find()
    torch.cuda.synchronize()
    state = d_state.cpu().numpy().view(np.uint64).tolist()
    ok = (int(d_err.cpu().numpy().view(np.uint32)[0]) == 0 and np.array_equal(d_new.cpu().numpy(), want_new)
          and state[:3] == [distinct, distinct * RB, n]
          and state[3] == (int(np.flatnonzero(want_new)[9]) if distinct >= 10 else NONE)
          and np.array_equal(d_hit.cpu().numpy().view(np.uint64), want_latest[perm])
          and (d_status.cpu().numpy() == 1).all())
    if not ok:
        raise SystemExit(f"bench_memtable: mix {name}: the device answers differ from the host result")
    sort()
    if n_out.value != distinct:
        raise SystemExit(f"bench_memtable: mix {name}: the flush kept {n_out.value} records, not {distinct}")

    def timed(fn, before=None):
        return benchlib.event_ms(s, fn, args.warmup, args.steps, before)

    t = {"add_ms": timed(add, clear), "find_ms": timed(find), "sort_ms": timed(sort), "lookup_ms": timed(lookup)}
    out = {"mix": name, "records": n, "distinct_keys": distinct, "record_bytes": RB, "slots": slots,
           "steps": args.steps, "warmup": args.warmup, "verified_vs_host": True}
    med = {k: benchlib.put(out, k, x, 4) for k, x in t.items()}
    out["add_mwrites_s"] = round(n / med["add_ms"] / 1e3, 1)
    out["find_mkeys_s"] = round(n / med["find_ms"] / 1e3, 1)
    out["sort_vs_add"] = round(med["sort_ms"] / med["add_ms"], 2)
    out["lookup_vs_find"] = round(med["lookup_ms"] / med["find_ms"], 2)
    if cpu is not None:
        host_log = d_log.cpu().numpy()
        off = np.arange(n, dtype=np.uint64) * RB
        qk = np.ascontiguousarray(keys[perm])
        qoff, qlen = np.arange(n, dtype=np.uint64) * KS, np.full(n, KS, np.uint64)
        for threads in (1, 16):
            is_new, totals, latest = np.zeros(n, np.uint8), np.zeros(2, np.uint64), np.zeros(n, np.uint64)
            secs = np.zeros(2, np.float64)
            best = None
            for _ in range(args.cpu_repeats):
                cpu.cpu_memtable(host_log.ctypes.data, off.ctypes.data, n, threads, qk.ctypes.data, qoff.ctypes.data,
                                 qlen.ctypes.data, n, is_new.ctypes.data, totals.ctypes.data, latest.ctypes.data,
                                 secs.ctypes.data)
                best = secs.copy() if best is None else np.minimum(best, secs)
            agrees = bool(np.array_equal(is_new, want_new) and totals.tolist() == [distinct, distinct * RB]
                          and np.array_equal(latest, want_latest[perm]))
            if not agrees:
                raise SystemExit(f"bench_memtable: mix {name}: tools/cpu_memtable.cpp ({threads} threads) differs")
            out[f"cpu{threads}_add_ms"] = round(best[0] * 1e3, 3)
            out[f"cpu{threads}_find_ms"] = round(best[1] * 1e3, 3)
            out[f"cpu{threads}_vs_add"] = round(best[0] * 1e3 / med["add_ms"], 1)
            out[f"cpu{threads}_vs_find"] = round(best[1] * 1e3 / med["find_ms"], 1)
    benchlib.line(out)
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mixes", default="distinct,sixteenth,single")
    ap.add_argument("--records", type=int, default=N)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cpu-repeats", type=int, default=3, help="the host program's best of this many runs")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "memtable_bench.json"))
    args = ap.parse_args()
    cpu = None if args.no_cpu else cpu_lib()
    results = [run_mix(name, args, cpu) for name in args.mixes.split(",")]
    benchlib.write({"metric": "live memtable on the device", "mixes": results}, args.out)


if __name__ == "__main__":
    main()
