#!/usr/bin/env python3
"""HyperLogLog adds and Count-Min Sketch inserts on the device at three shapes:
  a  the keys of 1 Mi records of 146 bytes (16-byte keys), records form
  s  1 Mi 16-byte keys, packed spans
  d  shape a with every key equal
For each shape: HLL at P = 14, CMS at (M, K) = (28, 3) and (27183, 14), each on
every NKV_OPT_SKETCH_PATH (0 auto, 1 direct global atomics, 2 LDS copies), and
the filter insert the gates compare with, in the same process on the same
table: nkv_bloom_insert[_records]_dev with k = 1, m = 8 * 2^14 for the HLL and
with the CMS's own (m, k) for the CMS.

Prints one JSON line per shape and writes them all to profiles/sketch_bench.json:
  *_ms            median over --steps calls after --warmup, [min, max] next to
                  it, between two events on the stream; the output is zeroed
                  before every call, outside the events (a warmed-up register
                  file would make every Add a no-op)
  hll_vs_bloom    HLL auto / Bloom k = 1; the gate is <= 1.25 on shape a
  cms_vs_bloom    CMS auto / Bloom with the same m and k; the gate is <= 2
  cpu_*_s         tools/cpu_sketch.cpp (built here with g++): the plain murmur3
                  loop plus the update on 1 thread and on 16 with per-thread
                  copies merged; *_speedup = that time / the device's
The device output of every path is compared with the C++ loop's before any
timing counts, and the C++ loop's with tests/sketch_ref.py on a small ragged
batch first.

--sweep adds "tier_sweep": the A/B behind the auto rule of NKV_OPT_SKETCH_PATH,
paths 1 and 2 on packed 16-byte keys for n = 4 Ki .. 16 Mi, HLL at P = 4, 10,
12, 13, 14, 16 and CMS at (28, 3), (100, 33), (2719, 5), (1024, 16), medians of
15 calls after 3, and which path auto takes for each.
"""
import argparse
import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import benchlib  # noqa: E402

N = 1 << 20
REC = 146
HLL_P = 14
CMS_TABLES = ((28, 3), (27183, 14))
SEED0 = 0x5EED
CPU_THREADS = 16
GATE_HLL, GATE_CMS = 1.25, 2.0


def cpu_lib():
    vp, u32, dbl = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_double
    return benchlib.build_cpu("sketch", {
        "cpu_hll": (dbl, [vp] * 3 + [ctypes.c_uint64, ctypes.c_int, ctypes.c_int, vp]),
        "cpu_cms": (dbl, [vp] * 3 + [ctypes.c_uint64, u32, u32, u32, ctypes.c_int, vp])}, ["-pthread"])


def cpu_hll(cpu, base, off, ln, p, threads):
    reg = np.zeros(1 << p, np.uint8)
    secs = cpu.cpu_hll(base.ctypes.data, off.ctypes.data, ln.ctypes.data, ln.size, p, threads, reg.ctypes.data)
    return secs, reg


def cpu_cms(cpu, base, off, ln, m, k, threads):
    tab = np.zeros((k, m), np.uint32)
    secs = cpu.cpu_cms(base.ctypes.data, off.ctypes.data, ln.ctypes.data, ln.size, m, k, SEED0, threads,
                       tab.ctypes.data)
    return secs, tab


def check_cpu_sketch(cpu):
    """The C++ loops against tests/sketch_ref.py on 3,000 ragged keys, on one thread and on several."""
    from tests import sketch_ref as ref
    rng = np.random.default_rng(0x736B62)
    ln = rng.integers(0, 41, 3000).astype(np.uint64)
    ln[0] = 0
    off = np.zeros(3000, np.uint64)
    off[1:] = np.cumsum(ln[:-1])
    data = rng.integers(0, 256, int(ln.sum()) + 1, dtype=np.uint8)
    for threads in (1, 5):
        if not np.array_equal(cpu_hll(cpu, data, off, ln, 11, threads)[1],
                              ref.hll_add_many(np.zeros(1 << 11, np.uint8), data, off, ln, 11)):
            raise SystemExit("bench_sketch: tools/cpu_sketch.cpp's HLL differs from tests/sketch_ref.py")
        if not np.array_equal(cpu_cms(cpu, data, off, ln, 28, 3, threads)[1],
                              ref.cms_insert_many(np.zeros((3, 28), np.uint32), data, off, ln, SEED0)):
            raise SystemExit("bench_sketch: tools/cpu_sketch.cpp's CMS differs from tests/sketch_ref.py")


def make_shape(name):
    """(host bytes, key offsets, key lengths, records?, record offsets)."""
    rng = np.random.default_rng(0x6E6B76)
    ln = np.full(N, 16, np.uint64)
    if name == "s":
        data = rng.integers(0, 256, N * 16, dtype=np.uint8)
        return data, np.arange(N, dtype=np.uint64) * 16, ln, False, None
    tab = rng.integers(0, 256, (N, REC), dtype=np.uint8)
    tab[:, 14:30] = benchlib.size_fields(16, REC - 46)
    if name == "d":
        tab[:, 30:46] = np.frombuffer(b"every key is one", np.uint8)
    rec_off = np.arange(N, dtype=np.uint64) * REC
    return tab.reshape(-1), rec_off + 30, ln, True, rec_off


def run_shape(name, args, cpu):
    import torch
    from nakevaleng_amd import _lib
    L, ctx, s = benchlib.open_ctx()
    data, koff, klen, records, rec_off = make_shape(name)

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8)).cuda()

    d_data = up(data)
    d_off = up(rec_off if records else koff)
    d_len = up(klen)
    torch.cuda.synchronize()
    base, off, ln, nbytes = d_data.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), data.size

    def hll(out):
        if records:
            return L.nkv_hll_add_records_dev(ctx.h, base, nbytes, off, N, HLL_P, out)
        return L.nkv_hll_add_dev(ctx.h, base, off, ln, N, HLL_P, out)

    def cms(m, k):
        def go(out):
            if records:
                return L.nkv_cms_insert_records_dev(ctx.h, base, nbytes, off, N, m, k, SEED0, out)
            return L.nkv_cms_insert_dev(ctx.h, base, off, ln, N, m, k, SEED0, out)
        return go

    def bloom(m, k):
        def go(out):
            if records:
                return L.nkv_bloom_insert_records_dev(ctx.h, base, nbytes, off, N, m, k, SEED0, out)
            return L.nkv_bloom_insert_dev(ctx.h, base, off, ln, N, m, k, SEED0, out)
        return go

    def timed(call, out_bytes, path=None):
        """(ms per call, the output of the last call)"""
        d_out = torch.zeros(out_bytes, dtype=torch.uint8, device="cuda")
        if path is not None:
            ctx.set_option(_lib.NKV_OPT_SKETCH_PATH, path)
        ms = benchlib.event_ms(s, lambda: _lib.check(call(d_out.data_ptr())), args.warmup, args.steps, d_out.zero_)
        ctx.set_option(_lib.NKV_OPT_SKETCH_PATH, 0)
        return ms, d_out.cpu().numpy()

    out = {"shape": name, "keys": N, "records_form": records, "steps": args.steps, "warmup": args.warmup}

    def put(key, ms):
        return benchlib.put(out, key + "_ms", ms, 4)

    # HLL
    want = None
    if cpu is not None:
        t1, want = cpu_hll(cpu, data, koff, klen, HLL_P, 1)
        t16, w16 = cpu_hll(cpu, data, koff, klen, HLL_P, CPU_THREADS)
        if not np.array_equal(want, w16):
            raise SystemExit("bench_sketch: the C++ HLL loop differs between 1 and 16 threads")
        out["cpu_hll_s"] = {"1": round(t1, 5), str(CPU_THREADS): round(t16, 5)}
    hll_ms = {}
    for path in (0, 1, 2):
        ms, got = timed(hll, 1 << HLL_P, path)
        if want is not None and not np.array_equal(got, want):
            raise SystemExit(f"bench_sketch: shape {name}: HLL path {path} differs from the C++ loop")
        hll_ms[path] = put(f"hll_p{HLL_P}_path{path}", ms)
    bm = 8 << HLL_P
    b_ms = put(f"bloom_m{bm}_k1", timed(bloom(bm, 1), ((bm + 31) // 32) * 4)[0])
    out["hll_vs_bloom"] = round(hll_ms[0] / b_ms, 3)
    out["hll_gate"] = GATE_HLL
    if cpu is not None:
        out["hll_speedup_vs_cpu"] = {k: round(v * 1e3 / hll_ms[0], 1) for k, v in out["cpu_hll_s"].items()}
    # CMS
    for m, k in CMS_TABLES:
        tag = f"cms_{m}x{k}"
        want = None
        if cpu is not None:
            t1, want = cpu_cms(cpu, data, koff, klen, m, k, 1)
            t16, w16 = cpu_cms(cpu, data, koff, klen, m, k, CPU_THREADS)
            if not np.array_equal(want, w16):
                raise SystemExit("bench_sketch: the C++ CMS loop differs between 1 and 16 threads")
            out[f"cpu_{tag}_s"] = {"1": round(t1, 5), str(CPU_THREADS): round(t16, 5)}
        c_ms = {}
        for path in (0, 1, 2):
            ms, got = timed(cms(m, k), 4 * m * k, path)
            if want is not None and not np.array_equal(got.view(np.uint32).reshape(k, m), want):
                raise SystemExit(f"bench_sketch: shape {name}: CMS {m}x{k} path {path} differs from the C++ loop")
            c_ms[path] = put(f"{tag}_path{path}", ms)
        b_ms = put(f"bloom_m{m}_k{k}", timed(bloom(m, k), ((m + 31) // 32) * 4)[0])
        out[f"{tag}_vs_bloom"] = round(c_ms[0] / b_ms, 3)
        if cpu is not None:
            out[f"{tag}_speedup_vs_cpu"] = {kk: round(v * 1e3 / c_ms[0], 1) for kk, v in out[f"cpu_{tag}_s"].items()}
    out["cms_gate"] = GATE_CMS
    out["verified_vs_cpu_loop"] = cpu is not None
    ctx.close()
    benchlib.line(out)
    del d_data, d_off, d_len
    torch.cuda.empty_cache()
    return out


SWEEP_N = (4096, 32768, 262144, 1 << 20, 1 << 22, 1 << 24)
SWEEP_P = (4, 10, 12, 13, 14, 16)
SWEEP_TABLES = ((28, 3), (100, 33), (2719, 5), (1024, 16))


def run_sweep():
    import torch
    from nakevaleng_amd import _lib
    L, ctx, s = benchlib.open_ctx()
    nmax = max(SWEEP_N)
    d_keys = torch.empty(nmax * 16, dtype=torch.uint8, device="cuda")
    _lib.check(L.nkv_fill_splitmix64_dev(ctx.h, d_keys.data_ptr(), nmax * 16, 7))
    d_off = torch.from_numpy((np.arange(nmax, dtype=np.uint64) * 16).view(np.uint8)).cuda()
    d_len = torch.from_numpy(np.full(nmax, 16, np.uint64).view(np.uint8)).cuda()
    torch.cuda.synchronize()
    keys = (d_keys.data_ptr(), d_off.data_ptr(), d_len.data_ptr())

    def timed(call, nbytes, path, steps=15, warm=3):
        d_out = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        ctx.set_option(_lib.NKV_OPT_SKETCH_PATH, path)
        ms = benchlib.event_ms(s, lambda: _lib.check(call(d_out.data_ptr())), warm, steps, d_out.zero_)
        ctx.set_option(_lib.NKV_OPT_SKETCH_PATH, 0)
        return round(benchlib.median(ms), 4)

    rows = []
    for n in SWEEP_N:
        for p in SWEEP_P:
            def f(out, n=n, p=p):
                return L.nkv_hll_add_dev(ctx.h, *keys, n, p, out)
            rows.append({"hll_p": p, "n": n, "auto_ms": timed(f, 1 << p, 0), "direct_ms": timed(f, 1 << p, 1),
                         "lds_ms": timed(f, 1 << p, 2)})
        for m, k in SWEEP_TABLES:
            def g(out, n=n, m=m, k=k):
                return L.nkv_cms_insert_dev(ctx.h, *keys, n, m, k, SEED0, out)
            rows.append({"cms": [m, k], "n": n, "auto_ms": timed(g, 4 * m * k, 0), "direct_ms": timed(g, 4 * m * k, 1),
                         "lds_ms": timed(g, 4 * m * k, 2)})
    for r in rows:
        benchlib.line(r)
    ctx.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="a,s,d")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--sweep", action="store_true", help="also the path 1 / path 2 A/B over n and table sizes")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sketch_bench.json"))
    args = ap.parse_args()
    if args.steps < 20:
        print("bench_sketch: fewer than 20 timed calls: the medians are not for the record", file=sys.stderr)
    cpu = None
    if not args.no_cpu:
        cpu = cpu_lib()
        check_cpu_sketch(cpu)
    results = [run_shape(name, args, cpu) for name in args.shapes.split(",")]
    out = {"metric": "HyperLogLog add and Count-Min Sketch insert on the device", "shapes": results}
    if args.sweep:
        out["tier_sweep"] = run_sweep()
    benchlib.write(out, args.out)


if __name__ == "__main__":
    main()
