#!/usr/bin/env python3
"""Compaction merge on the device (nkv_merge_records_dev): 4 runs of 256 Ki
SSTable-shaped records (16-B key, 4,050-B value), about a quarter of the keys
in two runs, timestamps of three adjacent seconds.

Prints one JSON line and writes it to profiles/merge_bench.json:
  call_ms        the whole call (validate, rank, scans, scatter, copy; host wall
                 clock, the call synchronizes)
  copy_ms        the copy kernel alone, from the context's events
  copy_gbs       bytes read + written (2 x out_len) / copy_ms
  memcpy_gbs     hipMemcpyDtoDAsync of out_len bytes in the same process, same
                 accounting; copy_vs_memcpy = copy_gbs / memcpy_gbs
  cpu_merge_s    a single-thread heap-based C++ k-way merge of the same inputs
                 (tools/cpu_merge.cpp, built here with g++)
Before it prints, the sources of every output record are checked against
tests/merge_ref.merge_closed, and the bytes of a seeded sample of output
records against their input records.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from nakevaleng_amd import _lib  # noqa: E402
from nakevaleng_amd.record import Record  # noqa: E402

KS, VS = 16, 4050
RB = 30 + KS + VS


def build_cpu_merge():
    src = os.path.join(ROOT, "tools", "cpu_merge.cpp")
    so = os.path.join(ROOT, "build", "cpu_merge.so")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", src, "-o", so])
    lib = ctypes.CDLL(so)
    lib.cpu_merge.restype = ctypes.c_double
    lib.cpu_merge.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_uint64), ctypes.c_int,
                              ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
    return lib


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=4)
    ap.add_argument("--records", type=int, default=1 << 18, help="records per run")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--sample", type=int, default=512)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge_bench.json"))
    args = ap.parse_args()
    k, n = args.runs, args.records
    rng = np.random.default_rng(0x6D657267)
    L = _lib.lib()
    ctx = _lib.Context(0)
    s = torch.cuda.current_stream()
    ctx.set_stream(s.cuda_stream)

    pool = np.unique(rng.integers(0, 1 << 48, int(k * n * 0.8)).astype(np.uint64))
    ids, tss, d_runs = [], [], []
    runs = (_lib.NkvRun * k)()
    off = torch.arange(n, dtype=torch.int64, device="cuda") * RB
    for r in range(k):
        i = np.sort(rng.choice(pool, n, replace=False))
        t = rng.integers(0, 3, n).astype("<i8")
        d = torch.empty(n * RB, dtype=torch.uint8, device="cuda")
        _lib.check(L.nkv_fill_splitmix64_dev(ctx.h, d.data_ptr(), n * RB, 0x6E616B65 + r))
        v = d.view(n, RB)
        v[:, 4:12] = torch.from_numpy(t.view(np.uint8).reshape(n, 8).copy()).cuda()
        v[:, 14:22] = torch.from_numpy(np.frombuffer(np.uint64(KS).tobytes(), np.uint8).copy()).cuda()
        v[:, 22:30] = torch.from_numpy(np.frombuffer(np.uint64(VS).tobytes(), np.uint8).copy()).cuda()
        v[:, 30:38] = torch.from_numpy(i.astype(">u8").view(np.uint8).reshape(n, 8).copy()).cuda()
        v[:, 38:46] = 0
        ids.append(i)
        tss.append(t)
        d_runs.append(d)
        runs[r] = _lib.NkvRun(d.data_ptr(), n * RB, off.data_ptr(), n)
    total = k * n * RB
    d_out = torch.empty(total, dtype=torch.uint8, device="cuda")
    d_off = torch.empty(8 * k * n, dtype=torch.uint8, device="cuda")
    d_src = torch.empty(8 * k * n, dtype=torch.uint8, device="cuda")
    n_out, out_len = ctypes.c_uint64(0), ctypes.c_uint64(0)

    def call():
        _lib.check(L.nkv_merge_records_dev(ctx.h, runs, k, d_out.data_ptr(), total, d_off.data_ptr(),
                                           d_src.data_ptr(), ctypes.byref(n_out), ctypes.byref(out_len)))

    torch.cuda.synchronize()
    for _ in range(args.warmup):
        call()
    ctx.set_timing(True)
    call_ms, prep_ms, copy_ms = [], [], []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        call()
        call_ms.append((time.perf_counter() - t0) * 1e3)
        a, b = ctx.last_timing()
        prep_ms.append(a)
        copy_ms.append(b)
    ctx.set_timing(False)
    nb, no = out_len.value, n_out.value

    # the comparator: hipMemcpyDtoDAsync of out_len bytes on the same stream
    hip = ctypes.CDLL("libamdhip64.so.7")
    hip.hipMemcpyDtoDAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    d_cmp = torch.empty(nb, dtype=torch.uint8, device="cuda")
    memcpy_ms = []
    for it in range(args.warmup + args.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        rc = hip.hipMemcpyDtoDAsync(d_cmp.data_ptr(), d_out.data_ptr(), nb, s.cuda_stream)
        e1.record(s)
        torch.cuda.synchronize()
        if rc != 0:
            raise RuntimeError(f"hipMemcpyDtoDAsync -> {rc}")
        if it >= args.warmup:
            memcpy_ms.append(e0.elapsed_time(e1))

    # verify: every source against merge_closed (values left out: it reads keys and timestamps only)
    from tests.merge_ref import merge_closed
    model = [[Record(0, int(t), 0, 0, KS, 0, int(i).to_bytes(8, "big"), b"") for i, t in zip(ids[r], tss[r])]
             for r in range(k)]
    _, want = merge_closed(model)
    want = np.asarray([(r << 32) | i for r, i in want], dtype=np.uint64)
    src = d_src.cpu().numpy().view(np.uint64)[:no]
    offs = d_off.cpu().numpy().view(np.uint64)[:no]
    ok = no == want.size and np.array_equal(src, want) and nb == no * RB and \
        np.array_equal(offs, np.arange(no, dtype=np.uint64) * RB)
    if ok:
        for j in np.random.default_rng(1).choice(no, min(args.sample, no), replace=False).tolist() + [0, no - 1]:
            r, i = int(src[j]) >> 32, int(src[j]) & 0xFFFFFFFF
            ok = ok and torch.equal(d_out[j * RB:(j + 1) * RB], d_runs[r][i * RB:(i + 1) * RB])
    if not ok:
        raise SystemExit("bench_merge: the device merge differs from merge_closed")

    med = lambda x: float(np.median(x))  # noqa: E731
    copy_gbs = 2 * nb / (med(copy_ms) * 1e-3) / 1e9
    memcpy_gbs = 2 * nb / (med(memcpy_ms) * 1e-3) / 1e9
    out = {"metric": "compaction merge on the device", "runs": k, "records_per_run": n, "record_bytes": RB,
           "n_out": no, "out_len": nb, "steps": args.steps,
           "call_ms": round(med(call_ms), 3), "prepare_ms": round(med(prep_ms), 3),
           "copy_ms": round(med(copy_ms), 3), "copy_gbs": round(copy_gbs, 1),
           "memcpy_ms": round(med(memcpy_ms), 3), "memcpy_gbs": round(memcpy_gbs, 1),
           "copy_vs_memcpy": round(copy_gbs / memcpy_gbs, 3),
           "copy_ms_min_max": [round(min(copy_ms), 3), round(max(copy_ms), 3)],
           "memcpy_ms_min_max": [round(min(memcpy_ms), 3), round(max(memcpy_ms), 3)],
           "call_ms_min_max": [round(min(call_ms), 3), round(max(call_ms), 3)],
           "call_gbs_of_output": round(nb / (med(call_ms) * 1e-3) / 1e9, 1),
           "verified_vs_merge_closed": True, "verified_sample": min(args.sample, no) + 2}
    try:  # the shader clock the box reports right after the timed loops (read only)
        import re
        smi = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30).stdout
        m = re.search(r"sclk.*?\((\d+)Mhz\)", smi)
        out["sclk_mhz_after"] = int(m.group(1)) if m else None
    except Exception:
        out["sclk_mhz_after"] = None

    if not args.no_cpu:
        cpu = build_cpu_merge()
        host = [d.cpu().numpy() for d in d_runs]
        h_out = np.empty(total, np.uint8)
        a, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
        secs = cpu.cpu_merge((ctypes.c_void_p * k)(*[h.ctypes.data for h in host]),
                             (ctypes.c_uint64 * k)(*[h.size for h in host]), k, h_out.ctypes.data,
                             ctypes.byref(a), ctypes.byref(b))
        same = (a.value, b.value) == (no, nb)
        if same:
            same = all(bytes(h_out[j * RB:(j + 1) * RB]) == d_out[j * RB:(j + 1) * RB].cpu().numpy().tobytes()
                       for j in (0, no // 2, no - 1))
        out["cpu_merge_s"] = round(secs, 3)
        out["cpu_merge_gbs_of_output"] = round(nb / secs / 1e9, 2)
        out["cpu_merge_agrees"] = bool(same)
        out["call_speedup_vs_cpu"] = round(secs * 1e3 / med(call_ms), 1)
    print(json.dumps(out), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
