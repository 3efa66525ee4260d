#!/usr/bin/env python3
"""Record encode on the device (nkv_encode_records_dev) at three shapes:
  a  1 Mi puts, 16-byte random keys, 100-byte values: 146-byte records
  b  256 Ki puts, 16-byte keys, 4 KiB values
  r  256 Ki puts, value lengths cycling through tests/far.RAGGED and key lengths
     through 0..33
Every put carries its own Timestamp; Status and TypeInfo are left NULL.

Prints one JSON line per shape and writes them all to profiles/encode_bench.json:
  call_ms        the whole call (measure, scan, the host's read of the verdict,
                 writer, checksums, patch; host wall clock, then a synchronize)
  prepare_ms     everything before the writer, from the context's events
  reduce_ms      writer + checksums + patch, from the context's events
  crc_ms         the checksum launch alone: nkv_crc32_dev over the spans the
                 encoder checksums (d_out + 30 + off[i], klen + vlen), the same
                 kernel over the same bytes, between two events on the stream
  write_ms       reduce_ms - crc_ms: the writer, and with it the patch kernel
                 (4 bytes per record), so write_gbs is a lower bound
  write_gbs      (key and value bytes read + out_len written) / write_ms
  memcpy_gbs     hipMemcpyDtoDAsync of out_len bytes in the same process, read +
                 written; write_vs_memcpy = write_gbs / memcpy_gbs
  crc_gbs        checksummed bytes / crc_ms
  cpu_encode_s   tools/cpu_encode.cpp (zlib crc32 + memcpy, built here), on one
                 thread and on 16
  flush_puts_ms  lsmtree.flush_puts end to end from Python lists of keys and
                 values (pack, upload, encode, flush, tree, filter, downloads)
Medians over --steps calls after --warmup, with the minimum and the maximum
next to them.  Before a shape's timings count, the whole device output is
compared with the C++ loop's; the C++ loop itself is compared with
nakevaleng_amd/record.py on a small ragged batch first.
"""
import argparse
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import benchlib  # noqa: E402
from tests.far import RAGGED  # noqa: E402

SHAPES = {"a": 1 << 20, "b": 1 << 18, "r": 1 << 18}
CPU_THREADS = 16


def lengths(name):
    n = SHAPES[name]
    i = np.arange(n)
    if name == "a":
        return np.full(n, 16, np.uint64), np.full(n, 100, np.uint64)
    if name == "b":
        return np.full(n, 16, np.uint64), np.full(n, 4096, np.uint64)
    return (i % 34).astype(np.uint64), np.asarray(RAGGED, np.uint64)[i % len(RAGGED)]


def cpu_lib():
    vp = ctypes.c_void_p
    return benchlib.build_cpu("encode", {"cpu_encode": (ctypes.c_double, [vp] * 7 + [
        ctypes.c_int64, vp, vp, ctypes.c_uint64, ctypes.c_int, vp, ctypes.POINTER(ctypes.c_uint64)])},
        ["-pthread", "-lz"])


def cpu_encode(cpu, kb, koff, klen, vb, voff, vlen, ts, status, type_info, threads, out):
    nb = ctypes.c_uint64(0)

    def p(a):
        return None if a is None else a.ctypes.data

    secs = cpu.cpu_encode(p(kb), p(koff), p(klen), p(vb), p(voff), p(vlen), p(ts), 0, p(status), p(type_info),
                          len(koff), threads, p(out), ctypes.byref(nb))
    return secs, nb.value


def check_cpu_encode(cpu):
    """The C++ loop against record.py on 3,000 ragged puts, on one thread and on several."""
    from nakevaleng_amd import record
    rng = np.random.default_rng(0x63707565)
    keys = [rng.bytes(int(k)) for k in rng.integers(0, 34, 3000)]
    vals = [rng.bytes(int(v)) for v in rng.integers(0, 300, 3000)]
    ts = rng.integers(-2**62, 2**62, 3000)
    st, ty = rng.integers(0, 256, 3000).astype(np.uint8), rng.integers(0, 256, 3000).astype(np.uint8)
    recs = []
    for k, v, t, s, y in zip(keys, vals, ts, st, ty):
        r = record.New(k, v, int(t))
        r.Status, r.TypeInfo = int(s), int(y)
        recs.append(r)
    want = record.data_table(recs)[0]
    p = record.pack_puts(keys, vals, ts, st, ty)
    for threads in (1, 5):
        out = np.zeros(len(want) + 1, np.uint8)
        _, nb = cpu_encode(cpu, np.append(p["keys"], np.uint8(0)), p["koff"], p["klen"],
                           np.append(p["vals"], np.uint8(0)), p["voff"], p["vlen"], p["ts"], p["status"], p["type"],
                           threads, out)
        if nb != len(want) or out[:nb].tobytes() != want:
            raise SystemExit("bench_encode: tools/cpu_encode.cpp differs from record.py")


def run_shape(name, args, cpu):
    import torch
    from nakevaleng_amd import _lib, lsmtree
    n = SHAPES[name]
    klen, vlen = lengths(name)
    koff, voff = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    koff[1:], voff[1:] = np.cumsum(klen[:-1]), np.cumsum(vlen[:-1])
    kbytes, vbytes = int(klen.sum()), int(vlen.sum())
    total = 30 * n + kbytes + vbytes
    ts = (1_700_000_000 + np.arange(n) // 1000).astype(np.int64)
    L, ctx, s = benchlib.open_ctx()

    def up(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()

    d_keys = torch.empty(kbytes, dtype=torch.uint8, device="cuda")
    d_vals = torch.empty(vbytes, dtype=torch.uint8, device="cuda")
    _lib.check(L.nkv_fill_splitmix64_dev(ctx.h, d_keys.data_ptr(), kbytes, 0x6B657973))
    _lib.check(L.nkv_fill_splitmix64_dev(ctx.h, d_vals.data_ptr(), vbytes, 0x76616C73))
    d_koff, d_klen, d_voff, d_vlen, d_ts, d_plen = up(koff), up(klen), up(voff), up(vlen), up(ts), up(klen + vlen)
    puts = _lib.NkvPuts(d_keys.data_ptr(), kbytes, d_koff.data_ptr(), d_klen.data_ptr(), d_vals.data_ptr(), vbytes,
                        d_voff.data_ptr(), d_vlen.data_ptr(), d_ts.data_ptr(), 0, None, None, n)
    d_out = torch.empty(total, dtype=torch.uint8, device="cuda")
    d_off = torch.empty(8 * n, dtype=torch.uint8, device="cuda")
    d_crc = torch.empty(4 * n, dtype=torch.uint8, device="cuda")
    out_len = ctypes.c_uint64(0)

    def call():
        _lib.check(L.nkv_encode_records_dev(ctx.h, ctypes.byref(puts), d_out.data_ptr(), total, d_off.data_ptr(),
                                            d_crc.data_ptr(), ctypes.byref(out_len)))
        torch.cuda.synchronize()

    torch.cuda.synchronize()
    call()
    # verify before any timing counts: the whole output against the C++ loop's
    out = {"shape": name, "puts": n, "key_bytes": kbytes, "value_bytes": vbytes, "out_len": total,
           "steps": args.steps, "warmup": args.warmup}
    if out_len.value != total:
        raise SystemExit(f"bench_encode: shape {name}: out_len {out_len.value}, expected {total}")
    got = d_out.cpu().numpy()
    if cpu is not None:
        h_keys, h_vals = d_keys.cpu().numpy(), d_vals.cpu().numpy()
        h_out = np.zeros(total, np.uint8)
        secs1, nb = cpu_encode(cpu, h_keys, koff, klen, h_vals, voff, vlen, ts, None, None, 1, h_out)
        if nb != total or not np.array_equal(h_out, got):
            raise SystemExit(f"bench_encode: shape {name}: the device output differs from the C++ loop's")
        off = d_off.cpu().numpy().view(np.uint64)
        if not np.array_equal(off, np.cumsum(np.append(np.uint64(0), 30 + klen + vlen))[:-1]):
            raise SystemExit(f"bench_encode: shape {name}: d_out_off differs")
        if not np.array_equal(d_crc.cpu().numpy().view(np.uint32), h_out[off[:, None] + np.arange(4, dtype=np.uint64)]
                              .copy().view(np.uint32).reshape(-1)):
            raise SystemExit(f"bench_encode: shape {name}: d_crc differs from the headers")
        h_out16 = np.zeros(total, np.uint8)
        secs16, _ = cpu_encode(cpu, h_keys, koff, klen, h_vals, voff, vlen, ts, None, None, CPU_THREADS, h_out16)
        out["verified_vs_cpu_loop"] = True
        out["cpu_encode_s"] = {"1": round(secs1, 4), str(CPU_THREADS): round(secs16, 4)}
        out["cpu_threads_agree"] = bool(np.array_equal(h_out16, h_out))
        del h_out, h_out16

    call_ms, prep_ms, red_ms = benchlib.phase_ms(ctx, call, args.warmup, args.steps)

    # the checksum launch alone, and the comparator: hipMemcpyDtoDAsync of out_len bytes
    d_cmp = torch.empty(total, dtype=torch.uint8, device="cuda")
    d_crc2 = torch.empty(4 * n, dtype=torch.uint8, device="cuda")
    crc_ms = benchlib.event_ms(s, lambda: _lib.check(L.nkv_crc32_dev(ctx.h, d_out.data_ptr() + 30, d_off.data_ptr(),
                                                                     d_plen.data_ptr(), n, d_crc2.data_ptr())),
                               args.warmup, args.steps)
    if not torch.equal(d_crc2, d_crc):
        raise SystemExit(f"bench_encode: shape {name}: the separate checksum launch differs from d_crc")
    memcpy_ms = benchlib.memcpy_ms(s, d_cmp, d_out, total, args.warmup, args.steps)

    call_med = benchlib.put(out, "call_ms", call_ms, 3)
    benchlib.put(out, "prepare_ms", prep_ms, 3)
    red, crc = benchlib.put(out, "reduce_ms", red_ms, 3), benchlib.put(out, "crc_ms", crc_ms, 3)
    write_ms = red - crc
    write_gbs = (kbytes + vbytes + total) / (write_ms * 1e-3) / 1e9
    memcpy_gbs = 2 * total / (benchlib.put(out, "memcpy_ms", memcpy_ms, 3) * 1e-3) / 1e9
    out.update({"write_ms": round(write_ms, 3), "write_gbs": round(write_gbs, 1), "memcpy_gbs": round(memcpy_gbs, 1),
                "write_vs_memcpy": round(write_gbs / memcpy_gbs, 3),
                "crc_gbs": round((kbytes + vbytes) / (crc * 1e-3) / 1e9, 1)})
    if "cpu_encode_s" in out:
        out["call_speedup_vs_cpu"] = {k: round(v * 1e3 / call_med, 1) for k, v in out["cpu_encode_s"].items()}
    out["sclk_mhz_after"] = benchlib.sclk()  # right after the timed loops
    del d_cmp, got
    ctx.close()

    if args.flush_steps:  # end to end from Python lists
        kb, vb = d_keys.cpu().numpy().tobytes(), d_vals.cpu().numpy().tobytes()
        ko, vo = np.append(koff, np.uint64(kbytes)).tolist(), np.append(voff, np.uint64(vbytes)).tolist()
        keys = [kb[ko[i]:ko[i + 1]] for i in range(n)]
        vals = [vb[vo[i]:vo[i + 1]] for i in range(n)]
        del kb, vb
        flush_ms = []
        for it in range(1 + args.flush_steps):
            t0 = time.perf_counter()
            res = lsmtree.flush_puts(keys, vals, ts, device=0, seed=1)
            if it:
                flush_ms.append((time.perf_counter() - t0) * 1e3)
            flushed = len(res["table"][1])
            del res
        out["flush_puts_ms"] = round(benchlib.median(flush_ms), 1)  # its range keeps 3 digits
        out["flush_puts_ms_min_max"] = [round(min(flush_ms), 3), round(max(flush_ms), 3)]
        out["flush_puts_calls"] = args.flush_steps
        out["flushed_records"] = flushed
    benchlib.line(out)
    del d_out, d_keys, d_vals
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="a,b,r")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--flush-steps", type=int, default=3, help="timed lsmtree.flush_puts calls per shape (0: none)")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "encode_bench.json"))
    args = ap.parse_args()
    if args.steps < 20:
        print("bench_encode: fewer than 20 timed calls: the medians are not for the record", file=sys.stderr)
    cpu = None
    if not args.no_cpu:
        cpu = cpu_lib()
        check_cpu_encode(cpu)
    results = [run_shape(name, args, cpu) for name in args.shapes.split(",")]
    benchlib.write({"metric": "record encode on the device", "shapes": results}, args.out)


if __name__ == "__main__":
    main()
