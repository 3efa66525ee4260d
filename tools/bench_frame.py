#!/usr/bin/env python3
"""Framing a raw record stream on the device (nkv_frame_records_dev) on both
paths, NKV_OPT_FRAME_PATH 1 (walk) and 2 (speculative), against a single-thread
C++ walk of the same bytes in host memory (tools/cpu_frame.cpp), at four shapes:
  t146   1 Mi records of 146 bytes, one segment (a Data table)
  t4k    1 Mi records of 4 KiB, one segment
  wal    the 1 Mi records of t146 in segments of 5 (wal_max_recs_in_seg)
  zeros  64 Ki records with 4 KiB zero-filled values: nearly every position is
         a candidate start, the nodes pass the auto budget and the speculative
         path gives way to the walk
Keys and Values are the bytes of nkv_fill_splitmix64_dev; the tables are made on
the device and copied to the host once for the C++ walk.

Prints one JSON line per shape and writes them all to profiles/frame_bench.json:
  walk_ms / spec_ms / auto_ms   median wall time of the call (it synchronizes),
                  [min, max] next to it, over --steps calls after --warmup; a
                  call slower than 1 s is timed --slow-steps times
  *_leaf_ms / *_reduce_ms       the call's two NKV_TIMING_EVENTS intervals
  took            NKV_PATH_FRAME_* each setting really took
  cpu_ms          the C++ walk, best of 3
  m_over_n        candidate starts per record (from the marks, counted with torch)
The offsets of every device run are compared with the C++ walk's before any
timing counts.

--sweep adds "segment_sweep": t146 cut into segments of 5 .. 1 Mi records, both
paths: the measurement behind the auto rule's mean-segment threshold.
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

N = 1 << 20
SEED = 0x6672616D


def cpu_lib():
    vp, u64 = ctypes.c_void_p, ctypes.c_uint64
    return benchlib.build_cpu("frame", {"cpu_frame": (u64, [vp, u64, vp, u64, vp, ctypes.POINTER(ctypes.c_double),
                                                           ctypes.POINTER(u64)])})


def make_table(ctx, n, rec, zeros=False):
    """n records of rec bytes with 16-byte keys on the device: the fill's bytes, the size fields set."""
    import torch
    buf = benchlib.device_log(ctx, n, 16, rec - 46, seed=SEED)
    if zeros:
        buf.view(n, rec)[:, 46:] = 0
    torch.cuda.synchronize()
    return buf


def timed(call, args):
    """(median ms, [min, max], results of the last call): the host clock around
    a call that synchronizes, its own mode beside benchlib's loops because a
    call slower than 1 s is timed --slow-steps times."""
    out = None
    for _ in range(args.warmup):
        t0 = time.perf_counter()
        out = call()
        first = time.perf_counter() - t0
    steps = args.slow_steps if first > 1.0 else args.steps
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        out = call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return round(benchlib.median(ms), 3), [round(min(ms), 3), round(max(ms), 3)], out


def run_paths(ctx, d_stream, nbytes, seg, want_off, args, paths=(1, 2, 0)):
    """Each path's timing over (stream, segments); the offsets held to want_off."""
    import torch
    from nakevaleng_amd import _lib
    L = _lib.lib()
    S = 0 if seg is None else int(seg.size)
    d_seg = torch.from_numpy((seg if S else np.zeros(1, np.uint64)).view(np.uint8).copy()).cuda()
    cap = int(want_off.size)
    d_off = torch.zeros(8 * max(cap, 1), dtype=torch.uint8, device="cuda")
    n_out, stats = ctypes.c_uint64(0), (ctypes.c_uint64 * 4)()
    names = {1: "walk", 2: "spec", 0: "auto"}
    out = {}

    def call():
        _lib.check(L.nkv_frame_records_dev(ctx.h, d_stream.data_ptr(), nbytes, d_seg.data_ptr() if S else None, S, 0,
                                           d_off.data_ptr(), cap, None, None, ctypes.byref(n_out), stats),
                   "bench_frame")
        return ctx.last_path()

    for path in paths:
        ctx.set_option(_lib.NKV_OPT_FRAME_PATH, path)
        d_off.zero_()
        torch.cuda.synchronize()
        took = call()
        got = d_off.cpu().numpy().view(np.uint64)[:n_out.value]
        if n_out.value != cap or not np.array_equal(got, want_off):
            raise SystemExit(f"bench_frame: path {path} differs from the C++ walk")
        key = names[path]
        out[key + "_ms"], out[key + "_range_ms"], _ = timed(call, args)
        ctx.set_timing(True)
        call()
        leaf, red = ctx.last_timing()
        ctx.set_timing(False)
        out[key + "_leaf_ms"], out[key + "_reduce_ms"] = round(leaf, 3), round(red, 3)
        out.setdefault("took", {})[key] = {_lib.NKV_PATH_FRAME_WALK: "walk",
                                           _lib.NKV_PATH_FRAME_SPECULATIVE: "speculative"}.get(took, took)
    ctx.set_option(_lib.NKV_OPT_FRAME_PATH, 0)
    return out


def cpu_walk(cpu, host, seg):
    S = 0 if seg is None else int(seg.size)
    off = np.zeros(host.size // 30 + 1, np.uint64)
    best, n = None, 0
    secs, whole = ctypes.c_double(0), ctypes.c_uint64(0)
    for _ in range(3):
        n = cpu.cpu_frame(host.ctypes.data, host.size, seg.ctypes.data if S else None, S, off.ctypes.data,
                          ctypes.byref(secs), ctypes.byref(whole))
        best = secs.value if best is None else min(best, secs.value)
    return off[:n].copy(), best


def candidates(d_stream, nbytes):
    """Candidate starts of a one-segment stream, counted with torch in chunks (the mark rule)."""
    import torch
    total, step = 0, 1 << 26
    for lo in range(0, nbytes, step):
        hi = min(nbytes, lo + step + 29)
        x = d_stream[lo:hi].to(torch.int64)
        m = x.numel() - 29
        if m <= 0:
            break
        ks = sum(x[14 + b:14 + b + m] << (8 * b) for b in range(7))
        vs = sum(x[22 + b:22 + b + m] << (8 * b) for b in range(7))
        top = (x[21:21 + m] | x[29:29 + m]) == 0  # sizes below 2^56
        room = nbytes - 30 - (torch.arange(m, device=x.device) + lo)
        ok = top & (ks <= room) & (vs <= room - ks)
        total += int(ok[:min(m, step)].sum())
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--slow-steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--shapes", default="t146,t4k,wal,zeros")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_bench.json"))
    args = ap.parse_args()
    import torch
    from nakevaleng_amd import _lib, build as b
    b.build(quiet=True)
    cpu = cpu_lib()
    ctx = _lib.Context(0)
    results = []
    shapes = {"t146": (N, 146, False, 0), "t4k": (N, 4096, False, 0), "wal": (N, 146, False, 5),
              "zeros": (1 << 16, 4096 + 46, True, 0)}
    for name in args.shapes.split(","):
        n, rec, zeros, per = shapes[name]
        d_stream = make_table(ctx, n, rec, zeros)
        nbytes = n * rec
        host = d_stream.cpu().numpy()
        seg = (np.arange(0, n, per, dtype=np.uint64) * np.uint64(rec)) if per else None
        want, cpu_s = cpu_walk(cpu, host, seg)
        if want.size != n:
            raise SystemExit(f"bench_frame: the C++ walk found {want.size} records of {n}")
        r = {"shape": name, "records": n, "record_bytes": rec, "segments": 0 if seg is None else int(seg.size),
             "cpu_ms": round(cpu_s * 1e3, 3)}
        r.update(run_paths(ctx, d_stream, nbytes, seg, want, args))
        if seg is None:
            r["m_over_n"] = round(candidates(d_stream, nbytes) / n, 3)
        results.append(r)
        benchlib.line(r)
        if name == "t146" and args.sweep:
            sweep = []
            for per in (5, 20, 50, 100, 200, 500, 1000, 2000, 5000, 20000, 100000, N):
                seg = np.arange(0, n, per, dtype=np.uint64) * np.uint64(rec)
                row = {"records_per_segment": per, "mean_segment_bytes": per * rec}
                row.update(run_paths(ctx, d_stream, nbytes, seg, want, args, paths=(1, 2)))
                sweep.append(row)
                benchlib.line(row)
            results.append({"segment_sweep": sweep})
        del d_stream, host
        torch.cuda.empty_cache()
    benchlib.write(results, args.out)
    ctx.close()


if __name__ == "__main__":
    main()
