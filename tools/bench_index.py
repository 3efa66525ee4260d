#!/usr/bin/env python3
"""Index and Summary tables on the device (nkv_index_summary_dev) at two table
shapes, both at summary_page_size 3:
  1 Mi records of a 16-B key and a 4-KiB value (the flagship's record shape),
  4 Mi records of a 16-B key and a 100-B value (the reference's own small records).

Prints one JSON line and writes it to profiles/index_bench.json.  Per shape, in
one run of --steps calls:
  call_ms        the whole call (measure, scans, the host's read of the verdict
                 and the lengths, the writers; host wall clock around the call
                 and a synchronize)
  measure_ms     the measure kernel and the scans, from the context's events
  writer_ms      the three writer launches, from the context's events
  writer_gbs     (index_len + summary_len) bytes written / writer_ms
  memcpy_ms      hipMemcpyDtoDAsync of index_len + summary_len bytes in the same
                 process; memcpy_gbs the same bytes / memcpy_ms, and
                 writer_vs_memcpy = writer_gbs / memcpy_gbs
  cpu_s          the same two images by a single-thread C++ loop over the same
                 stream in host memory (tools/cpu_index.cpp, built here with g++)
  sclk_mhz_after the shader clock the box reports right after the timed loops
Before a shape's figures are kept, both device images are compared byte for
byte with the CPU loop's, and the CPU loop's Index prefix and a whole small
table with tests/sstable_ref's restatement of the reference.
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
from nakevaleng_amd import _lib  # noqa: E402

KS = 16
SHAPES = [("1Mi x (16 B key, 4 KiB value)", 1 << 20, 4096), ("4Mi x (16 B key, 100 B value)", 1 << 22, 100)]


def cpu_lib():
    vp, u64, pu64 = ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64)
    return benchlib.build_cpu("index", {"cpu_index": (ctypes.c_double, [vp, vp, u64, u64, vp, vp, pu64, pu64])})


def one_shape(L, ctx, s, name, n, vs, page, steps, warmup, cpu):
    from tests import sstable_ref as ref
    rb = 30 + KS + vs
    nbytes = n * rb
    d = benchlib.device_log(ctx, n, KS, vs, seed=0x696E6478 + vs)
    d_off = torch.arange(n, dtype=torch.int64, device="cuda") * rb
    ilen, slen = ctypes.c_uint64(0), ctypes.c_uint64(0)
    _lib.check(L.nkv_index_summary_dev(ctx.h, d.data_ptr(), nbytes, d_off.data_ptr(), n, page, None, 0, None, 0,
                                       ctypes.byref(ilen), ctypes.byref(slen)))
    ni, ns = ilen.value, slen.value
    d_index = torch.empty(ni, dtype=torch.uint8, device="cuda")
    d_summary = torch.empty(ns, dtype=torch.uint8, device="cuda")

    def call():
        _lib.check(L.nkv_index_summary_dev(ctx.h, d.data_ptr(), nbytes, d_off.data_ptr(), n, page, d_index.data_ptr(),
                                           ni, d_summary.data_ptr(), ns, ctypes.byref(ilen), ctypes.byref(slen)))
        torch.cuda.synchronize()

    torch.cuda.synchronize()
    call_ms, measure_ms, writer_ms = benchlib.phase_ms(ctx, call, warmup, steps)

    # the comparator: hipMemcpyDtoDAsync of as many bytes as the two images hold
    d_src = torch.empty(ni + ns, dtype=torch.uint8, device="cuda")
    d_dst = torch.empty(ni + ns, dtype=torch.uint8, device="cuda")
    memcpy_ms = benchlib.memcpy_ms(s, d_dst, d_src, ni + ns, warmup, steps)
    clock = benchlib.sclk()
    del d_src, d_dst

    out = {"shape": name, "records": n, "key_bytes": KS, "value_bytes": vs, "stream_bytes": nbytes,
           "index_len": ni, "summary_len": ns, "summary_entries": int(L.nkv_summary_entries(n, page))}
    call_med = benchlib.put(out, "call_ms", call_ms, 3)
    benchlib.put(out, "measure_ms", measure_ms, 3)
    writer_gbs = (ni + ns) / (benchlib.put(out, "writer_ms", writer_ms, 3) * 1e-3) / 1e9
    memcpy_gbs = (ni + ns) / (benchlib.put(out, "memcpy_ms", memcpy_ms, 3) * 1e-3) / 1e9
    out.update({"writer_gbs": round(writer_gbs, 1), "memcpy_gbs": round(memcpy_gbs, 1),
                "writer_vs_memcpy": round(writer_gbs / memcpy_gbs, 3), "sclk_mhz_after": clock})

    host = d.cpu().numpy()
    off = d_off.cpu().numpy().view(np.uint64)
    h_index, h_summary = np.empty(ni, np.uint8), np.empty(ns, np.uint8)
    a, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
    secs = cpu.cpu_index(host.ctypes.data, off.ctypes.data, n, page, h_index.ctypes.data, h_summary.ctypes.data,
                         ctypes.byref(a), ctypes.byref(b))
    same = (a.value, b.value) == (ni, ns) and np.array_equal(h_index, d_index.cpu().numpy()) and \
        np.array_equal(h_summary, d_summary.cpu().numpy())
    # the CPU loop itself against the restatement of the reference: the Index
    # of the first records is a prefix of the Index, and one small table whole
    k = 4099
    small = host[:k * rb].tobytes()
    want = ref.from_table(small, [rb] * k, page)
    same = same and h_index[:len(want[0])].tobytes() == want[0]
    si, ss = np.empty(len(want[0]), np.uint8), np.empty(len(want[1]), np.uint8)
    cpu.cpu_index(host.ctypes.data, off.ctypes.data, k, page, si.ctypes.data, ss.ctypes.data, ctypes.byref(a),
                  ctypes.byref(b))
    same = same and (si.tobytes(), ss.tobytes()) == want
    if not same:
        raise SystemExit(f"bench_index: {name}: the device images differ from the CPU loop or the restatement")
    out["cpu_s"] = round(secs, 4)
    out["cpu_gbs_of_output"] = round((ni + ns) / secs / 1e9, 2)
    out["verified_vs_cpu_loop_and_restatement"] = True
    out["call_speedup_vs_cpu"] = round(secs * 1e3 / call_med, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--page", type=int, default=3)
    ap.add_argument("--scale", type=int, default=1, help="divide the record counts (a quick look)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "index_bench.json"))
    args = ap.parse_args()
    cpu = cpu_lib()
    L, ctx, s = benchlib.open_ctx()
    out = {"metric": "SSTable Index and Summary tables on the device", "summary_page_size": args.page,
           "steps": args.steps, "shapes": []}
    for name, n, vs in SHAPES:
        out["shapes"].append(one_shape(L, ctx, s, name, n // args.scale, vs, args.page, args.steps, args.warmup, cpu))
    benchlib.emit(out, args.out)
    ctx.close()


if __name__ == "__main__":
    main()
