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
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import benchlib  # noqa: E402
from nakevaleng_amd import _lib  # noqa: E402
from nakevaleng_amd.record import Record  # noqa: E402

KS, VS = 16, 4050
RB = 30 + KS + VS


def cpu_lib():
    pu64 = ctypes.POINTER(ctypes.c_uint64)
    return benchlib.build_cpu("merge", {"cpu_merge": (ctypes.c_double, [ctypes.POINTER(ctypes.c_void_p), pu64,
                                                                        ctypes.c_int, ctypes.c_void_p, pu64, pu64])})


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
    L, ctx, s = benchlib.open_ctx()

    pool = np.unique(rng.integers(0, 1 << 48, int(k * n * 0.8)).astype(np.uint64))
    ids, tss, d_runs = [], [], []
    runs = (_lib.NkvRun * k)()
    off = torch.arange(n, dtype=torch.int64, device="cuda") * RB
    for r in range(k):
        i = np.sort(rng.choice(pool, n, replace=False))
        t = rng.integers(0, 3, n).astype("<i8")
        key = np.zeros((n, KS), np.uint8)
        key[:, :8] = i.astype(">u8").view(np.uint8).reshape(n, 8)
        d = benchlib.device_log(ctx, n, KS, VS, key, seed=benchlib.FILL_SEED + r)
        d.view(n, RB)[:, 4:12] = torch.from_numpy(t.view(np.uint8).reshape(n, 8).copy()).cuda()
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
    call_ms, prep_ms, copy_ms = benchlib.phase_ms(ctx, call, args.warmup, args.steps)
    nb, no = out_len.value, n_out.value

    # the comparator: hipMemcpyDtoDAsync of out_len bytes on the same stream
    d_cmp = torch.empty(nb, dtype=torch.uint8, device="cuda")
    memcpy_ms = benchlib.memcpy_ms(s, d_cmp, d_out, nb, args.warmup, args.steps)

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

    out = {"metric": "compaction merge on the device", "runs": k, "records_per_run": n, "record_bytes": RB,
           "n_out": no, "out_len": nb, "steps": args.steps}
    call_med = benchlib.put(out, "call_ms", call_ms, 3)
    benchlib.put(out, "prepare_ms", prep_ms, 3)
    copy_gbs = 2 * nb / (benchlib.put(out, "copy_ms", copy_ms, 3) * 1e-3) / 1e9
    memcpy_gbs = 2 * nb / (benchlib.put(out, "memcpy_ms", memcpy_ms, 3) * 1e-3) / 1e9
    out.update({"copy_gbs": round(copy_gbs, 1), "memcpy_gbs": round(memcpy_gbs, 1),
                "copy_vs_memcpy": round(copy_gbs / memcpy_gbs, 3),
                "call_gbs_of_output": round(nb / (call_med * 1e-3) / 1e9, 1),
                "verified_vs_merge_closed": True, "verified_sample": min(args.sample, no) + 2,
                "sclk_mhz_after": benchlib.sclk()})  # after the timed loops and the verification

    if not args.no_cpu:
        cpu = cpu_lib()
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
        out["call_speedup_vs_cpu"] = round(secs * 1e3 / call_med, 1)
    benchlib.emit(out, args.out)
    ctx.close()


if __name__ == "__main__":
    main()
