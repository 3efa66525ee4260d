#!/usr/bin/env python3
"""The engine's admission on the device (nkv_admit_dev) with 16-byte users and
keys, defaults of the reference (100 tokens, 1 second, start "$"), four cases:
  uniform64k  1 Mi requests, 64 Ki users drawn uniformly, the batch spanning 4 s
  distinct    1 Mi requests, every user another, 4 s
  single      1 Mi requests of one user at one time (ts_all)
  resets      64 Ki requests of one user, every one more than the interval after
              the one before: every request a reset, served by one lane as a
              chain of dependent loads (the adversarial shape; its 1 Mi figure
              is this one times 16, marked as extrapolated, not run)

Per case one JSON line, all of them in profiles/admit_bench.json.  Every device
time is the median of --steps device-event intervals on the context's stream
after --warmup untimed calls:
  admit_ms           one nkv_admit_dev with all five outputs
  memtable_add_ms    nkv_memtable_add_dev over a log of the same n whose keys
                     are the users (the nearest existing kernel chain: the same
                     hash grouping, no sort), the index cleared, untimed, in
                     front of every add
  cpu1_ms / cpu16_ms tools/admit/cpu_admit.cpp on this box: the literal loop
                     over one std::unordered_map, and 16 threads sharded by the
                     user's hash; the best of --cpu-repeats runs
  *_vs_admit         comparator time / admit time (above 1: the device wins)
Before any timing counts the device's verdicts and bucket images are held to the
host program's, byte for byte.
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
CASES = {"uniform64k": (N, 1 << 16), "distinct": (N, N), "single": (N, 1), "resets": (1 << 16, 1)}
START, MAX_TOKENS, INTERVAL = b"$", 100, 1  # coreconf.go:40-45


def cpu_lib():
    vp, u64, i64 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int64
    return benchlib.build_cpu("admit", {"cpu_admit": (None, [vp, vp, vp, vp, vp, vp, i64, u64, vp, u64, i64, i64,
                                                             ctypes.c_int, vp, vp, vp])}, ["-pthread"],
                              src_dir=os.path.join(ROOT, "tools", "admit"))


def run_case(name, args, cpu):
    import torch
    from nakevaleng_amd import _lib
    n, distinct = CASES[name]
    n = max(1, n * args.scale // 100)
    distinct = min(distinct, n)
    rng = np.random.default_rng(0x61646D74 + len(name))
    L, ctx, s = benchlib.open_ctx()
    uniq = benchlib.keys_of(benchlib.distinct_u64(rng, distinct))
    which = np.arange(n) if distinct == n else rng.integers(0, distinct, n)
    users = np.ascontiguousarray(uniq[which])
    keys = np.ascontiguousarray(benchlib.keys_of(rng.integers(0, 2**63, n, dtype=np.uint64)))
    keys[:, 0] = np.where(rng.random(n) < 1 / 64, START[0], ord("k"))  # one request in 64 is illegal
    off = np.arange(n, dtype=np.uint64) * KS
    length = np.full(n, KS, np.uint64)
    if name == "single":
        ts, ts_all = None, 1000
    elif name == "resets":
        ts, ts_all = 1000 + (INTERVAL + 1) * np.arange(n, dtype=np.int64), 0
    else:
        ts, ts_all = 1000 + (np.arange(n, dtype=np.int64) * 4) // n, 0

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8)).cuda()

    d_users, d_keys, d_off, d_len = dev(users), dev(keys), dev(off), dev(length)
    d_ts = None if ts is None else dev(ts)
    outs = [torch.empty(k * n, dtype=torch.uint8, device="cuda") for k in (1, 32, 8, 8, 1)]
    d_err = torch.zeros(4, dtype=torch.uint8, device="cuda")
    req = _lib.NkvRequests(d_users.data_ptr(), n * KS, d_off.data_ptr(), d_len.data_ptr(), d_keys.data_ptr(), n * KS,
                           d_off.data_ptr(), d_len.data_ptr(), None if d_ts is None else d_ts.data_ptr(), ts_all,
                           None, None, None, n)

    def admit():
        _lib.check(L.nkv_admit_dev(ctx.h, ctypes.byref(req), START, len(START), MAX_TOKENS, INTERVAL,
                                   *(t.data_ptr() for t in outs), d_err.data_ptr()))

    # the memtable's add over a log of the same n, keyed by the users
    d_log = benchlib.device_log(ctx, n, KS, VS, users)
    d_roff = torch.arange(n, dtype=torch.int64, device="cuda") * RB
    slots = 2
    while slots < 2 * n:
        slots *= 2
    d_index = torch.empty(8 * slots, dtype=torch.uint8, device="cuda")
    d_state = torch.empty(32, dtype=torch.uint8, device="cuda")
    d_new = torch.empty(n, dtype=torch.uint8, device="cuda")

    def clear():
        _lib.check(L.nkv_memtable_clear_dev(ctx.h, d_index.data_ptr(), slots, d_state.data_ptr()))

    def add():
        _lib.check(L.nkv_memtable_add_dev(ctx.h, d_log.data_ptr(), n * RB, d_roff.data_ptr(), 0, n, d_index.data_ptr(),
                                          slots, 3, 10, 1 << 62, d_state.data_ptr(), d_new.data_ptr(),
                                          d_err.data_ptr()))

    out = {"case": name, "requests": n, "users": int(np.unique(which).size), "user_bytes": KS, "key_bytes": KS,
           "max_tokens": MAX_TOKENS, "reset_interval": INTERVAL, "steps": args.steps, "warmup": args.warmup}
    # verify before any timing counts
    admit()
    torch.cuda.synchronize()
    if int(d_err.cpu().numpy().view(np.uint32)[0]):
        raise SystemExit(f"admit_bench: case {name}: the device refused the batch")
    verdict, image = outs[0].cpu().numpy(), outs[1].cpu().numpy()
    out["allowed"], out["throttled"], out["illegal"] = (int((verdict == v).sum()) for v in (1, 2, 0))
    cpu_best = {}
    if cpu is not None:
        start = np.frombuffer(START, np.uint8)
        for threads in (1, 16):
            v, img, secs = np.zeros(n, np.uint8), np.zeros(4 * n, np.int64), np.zeros(1, np.float64)
            best = None
            for _ in range(args.cpu_repeats):
                cpu.cpu_admit(users.ctypes.data, off.ctypes.data, length.ctypes.data, keys.ctypes.data, off.ctypes.data,
                              None if ts is None else ts.ctypes.data, ts_all, n, start.ctypes.data, len(START),
                              MAX_TOKENS, INTERVAL, threads, v.ctypes.data, img.ctypes.data, secs.ctypes.data)
                best = secs[0] if best is None else min(best, secs[0])
            if not (np.array_equal(v, verdict) and np.array_equal(img.view(np.uint8), image)):
                raise SystemExit(f"admit_bench: case {name}: tools/admit/cpu_admit.cpp ({threads} threads) and the "
                                 "device differ")
            cpu_best[threads] = best * 1e3
        out["verified_vs_host"] = True
    steps = min(args.steps, 10) if name == "resets" else args.steps
    med = {"admit_ms": benchlib.put(out, "admit_ms", benchlib.event_ms(s, admit, args.warmup, steps), 4),
           "memtable_add_ms": benchlib.put(out, "memtable_add_ms", benchlib.event_ms(s, add, args.warmup, steps, clear),
                                           4)}
    out["admit_mrequests_s"] = round(n / med["admit_ms"] / 1e3, 2)
    out["memtable_add_vs_admit"] = round(med["memtable_add_ms"] / med["admit_ms"], 2)
    for threads, ms in cpu_best.items():
        out[f"cpu{threads}_ms"] = round(ms, 3)
        out[f"cpu{threads}_vs_admit"] = round(ms / med["admit_ms"], 2)
    if name == "resets":
        out["admit_ms_at_1mi_extrapolated"] = round(med["admit_ms"] * N / n, 1)
    benchlib.line(out)
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--scale", type=int, default=100, help="percent of each case's requests (a quick look)")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cpu-repeats", type=int, default=3, help="the host program's best of this many runs")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "admit_bench.json"))
    args = ap.parse_args()
    cpu = None if args.no_cpu else cpu_lib()
    results = [run_case(name, args, cpu) for name in args.cases.split(",")]
    benchlib.write({"metric": "engine admission on the device", "cases": results}, args.out)


if __name__ == "__main__":
    main()
