#!/usr/bin/env python3
"""Memtable flush on the device (nkv_sort_records_dev) at four shapes:
  a  1 Mi writes, 16-byte random keys, 100-byte values, a quarter of the writes
     overwriting an earlier key
  b  256 Ki writes with 4 KiB values, the same key mix
  c  as a with keys "user:%012d": all share their first 8 bytes, so every
     comparison goes to the log (the comparator's slow path)
  bs as b with the log already in key order, so that the copy's sources
     ascend as they do in the merge (a reference point for the copy kernel)

Prints one JSON line per shape and writes them all to profiles/sort_bench.json:
  call_ms        the whole call (validate, tile sort, merge passes, survive,
                 scans, scatter, copy; host wall clock, the call synchronizes)
  prepare_ms     sort + survive + scans + scatter, from the context's events
                 (the split between the sort and the rest comes from a kernel
                 trace: rocprofv3 --kernel-trace --stats over this tool)
  copy_ms        the copy kernel alone, from the context's events
  copy_gbs       bytes read + written (2 x out_len) / copy_ms
  memcpy_gbs     hipMemcpyDtoDAsync of out_len bytes in the same process, same
                 accounting; copy_vs_memcpy = copy_gbs / memcpy_gbs
  cpu_sort_s     a single-thread std::stable_sort of indices by key and a copy
                 of each key's last record (tools/cpu_sort.cpp, built here)
Before a shape's timings count, the device's sources, offsets and totals are
checked against a host result (numpy: a lexicographic sort of the fixed-length
keys with the arrival index as the last key), and the whole output stream
against the C++ loop's; the C++ loop itself is checked against
tests/memtable_ref.flush_closed on a small ragged log first.
"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import benchlib  # noqa: E402

SHAPES = {"a": (1 << 20, 100, "random16"), "b": (1 << 18, 4096, "random16"), "c": (1 << 20, 100, "user"),
          "bs": (1 << 18, 4096, "random16-sorted")}
OVERWRITE = 0.25


def cpu_lib():
    vp, u64, pu64 = ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)
    return benchlib.build_cpu("sort", {"cpu_sort": (ctypes.c_double, [vp, u64, u64, vp, vp, pu64, pu64])})


def check_cpu_sort(cpu):
    """The C++ loop against flush_closed on 3,000 ragged writes over 700 keys."""
    from nakevaleng_amd import record
    from tests.memtable_ref import flush_closed
    rng = np.random.default_rng(0x63707573)
    pool = [bytes(rng.choice([0, 97, 98, 255], int(rng.integers(0, 14))).tolist()) for _ in range(700)]
    log = [record.New(pool[int(j)], rng.bytes(int(v)), timestamp=int(v) % 5)
           for j, v in zip(rng.integers(0, 700, 3000), rng.integers(0, 50, 3000))]
    data, _ = record.data_table(log)
    want, want_src = flush_closed(log)
    buf = np.frombuffer(data, np.uint8)
    out, src = np.empty(buf.size, np.uint8), np.empty(len(log), np.uint64)
    a, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
    cpu.cpu_sort(buf.ctypes.data, buf.size, len(log), out.ctypes.data, src.ctypes.data, ctypes.byref(a), ctypes.byref(b))
    if src[:a.value].tolist() != want_src or out[:b.value].tobytes() != b"".join(r.ToBytes() for r in want):
        raise SystemExit("bench_sort: tools/cpu_sort.cpp differs from flush_closed")


def make_keys(rng, n, kind):
    """(n, klen) key bytes in arrival order: a write overwrites, with probability
    OVERWRITE, the key of a uniformly chosen earlier first write."""
    fresh = rng.random(n) >= OVERWRITE
    fresh[0] = True
    first = np.flatnonzero(fresh)  # arrival indices of the first writes, ascending
    if kind.startswith("random16"):
        uniq = rng.integers(0, 256, (first.size, 16), dtype=np.uint8)
    else:
        ids = rng.choice(10**12, first.size, replace=False)
        uniq = np.frombuffer(b"".join(b"user:%012d" % int(i) for i in ids), np.uint8).reshape(first.size, 17)
    before = np.cumsum(fresh) - fresh  # first writes strictly before each arrival
    which = np.where(fresh, before, (rng.random(n) * np.maximum(before, 1)).astype(np.int64))
    keys = uniq[which]
    if kind.endswith("-sorted"):  # the same writes, arriving in key order
        cols = keys.view(">u8")
        keys = keys[np.lexsort([cols[:, 1], cols[:, 0]])]
    return keys


def host_flush(keys):
    """Arrival indices of the flushed records: sort by (key, arrival), keep the last of each key."""
    n, klen = keys.shape
    pad = np.zeros((n, (klen + 7) // 8 * 8), np.uint8)
    pad[:, :klen] = keys
    cols = pad.view(">u8")  # equal lengths: zero padding keeps the order
    order = np.lexsort([np.arange(n)] + [cols[:, c] for c in range(cols.shape[1] - 1, -1, -1)])
    s = cols[order]
    keep = np.ones(n, bool)
    keep[:-1] = (s[1:] != s[:-1]).any(axis=1)
    return order[keep].astype(np.uint64)


def run_shape(name, args, cpu):
    import torch
    from nakevaleng_amd import _lib
    n, vs, kind = SHAPES[name]
    vs = args.value_bytes if args.value_bytes is not None else vs
    rng = np.random.default_rng(0x736F7274 + ord(name[0]))
    L, ctx, s = benchlib.open_ctx()
    keys = make_keys(rng, n, kind)
    ks = keys.shape[1]
    rb = 30 + ks + vs
    total = n * rb
    d_log = benchlib.device_log(ctx, n, ks, vs, keys)
    d_roff = torch.arange(n, dtype=torch.int64, device="cuda") * rb
    d_out = torch.empty(total, dtype=torch.uint8, device="cuda")
    d_off = torch.empty(8 * n, dtype=torch.uint8, device="cuda")
    d_src = torch.empty(8 * n, dtype=torch.uint8, device="cuda")
    n_out, out_len = ctypes.c_uint64(0), ctypes.c_uint64(0)

    def call():
        _lib.check(L.nkv_sort_records_dev(ctx.h, d_log.data_ptr(), total, d_roff.data_ptr(), n, d_out.data_ptr(), total,
                                          d_off.data_ptr(), d_src.data_ptr(), ctypes.byref(n_out),
                                          ctypes.byref(out_len)))

    torch.cuda.synchronize()
    call()
    # verify before any timing counts
    want = host_flush(keys)
    no, nb = n_out.value, out_len.value
    src = d_src.cpu().numpy().view(np.uint64)[:no]
    offs = d_off.cpu().numpy().view(np.uint64)[:no]
    if not (no == want.size and nb == no * rb and np.array_equal(src, want)
            and np.array_equal(offs, np.arange(no, dtype=np.uint64) * rb)):
        raise SystemExit(f"bench_sort: shape {name}: the device flush differs from the host result")
    host_log = d_log.cpu().numpy()
    got = d_out.cpu().numpy()[:nb]
    if not np.array_equal(got.reshape(no, rb), host_log.reshape(n, rb)[want.astype(np.int64)]):
        raise SystemExit(f"bench_sort: shape {name}: output bytes differ from the records at the host's sources")

    call_ms, prep_ms, copy_ms = benchlib.phase_ms(ctx, call, args.warmup, args.steps)
    # the comparator: hipMemcpyDtoDAsync of out_len bytes on the same stream
    d_cmp = torch.empty(nb, dtype=torch.uint8, device="cuda")
    memcpy_ms = benchlib.memcpy_ms(s, d_cmp, d_out, nb, args.warmup, args.steps)

    out = {"shape": name, "records": n, "key_bytes": ks, "value_bytes": vs, "keys": kind, "log_len": total,
           "n_out": no, "out_len": nb, "steps": args.steps, "warmup": args.warmup}
    call_med = benchlib.put(out, "call_ms", call_ms, 3)
    benchlib.put(out, "prepare_ms", prep_ms, 3)
    copy_gbs = 2 * nb / (benchlib.put(out, "copy_ms", copy_ms, 3) * 1e-3) / 1e9
    memcpy_gbs = 2 * nb / (benchlib.put(out, "memcpy_ms", memcpy_ms, 3) * 1e-3) / 1e9
    out.update({"copy_gbs": round(copy_gbs, 1), "memcpy_gbs": round(memcpy_gbs, 1),
                "copy_vs_memcpy": round(copy_gbs / memcpy_gbs, 3), "verified_vs_host_sort": True,
                "sclk_mhz_after": benchlib.sclk()})  # right after the timed loops

    if cpu is not None:
        h_out = np.empty(total, np.uint8)
        a, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
        secs = cpu.cpu_sort(host_log.ctypes.data, total, n, h_out.ctypes.data, None, ctypes.byref(a), ctypes.byref(b))
        out["cpu_sort_s"] = round(secs, 3)
        out["cpu_sort_agrees"] = bool((a.value, b.value) == (no, nb) and np.array_equal(h_out[:nb], got))
        out["call_speedup_vs_cpu"] = round(secs * 1e3 / call_med, 1)
    benchlib.line(out)
    ctx.close()
    del d_log, d_out, d_cmp
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="a,b,c,bs")
    ap.add_argument("--value-bytes", type=int, default=None, help="ValueSize of every shape (default: the shape's own)")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sort_bench.json"))
    args = ap.parse_args()
    cpu = None
    if not args.no_cpu:
        cpu = cpu_lib()
        check_cpu_sort(cpu)
    results = [run_shape(name, args, cpu) for name in args.shapes.split(",")]
    by = {r["shape"]: r for r in results}
    out = {"metric": "memtable flush on the device", "shapes": results}
    if "a" in by and "c" in by:
        out["prepare_c_over_a"] = round(by["c"]["prepare_ms"] / by["a"]["prepare_ms"], 2)
    if "a" in by and "cpu_sort_s" in by["a"]:
        out["device_beats_cpu_on_a"] = bool(by["a"]["call_ms"] < by["a"]["cpu_sort_s"] * 1e3)
    benchlib.write(out, args.out)


if __name__ == "__main__":
    main()
