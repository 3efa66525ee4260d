"""The bench layer of the component benchmarks (tools/bench_*.py): the one
place that opens a context, builds a host comparator, times a call, writes a
figure and makes the records the tools share.  A driver run as a script finds
this module through sys.path[0]; a new path's bench gets its loops here.

Three timing modes, three different measurements:
  event_ms   one call between a fresh pair of events, a synchronize after
             every call, the first `warmup` samples dropped (alternating_ms:
             the same for several calls taking turns, so all see the same clocks)
  phase_ms   host wall clock around a call that synchronizes, with the
             context's two event intervals of the same call (set_timing)
  batch_ms   `steps` calls between one pair of events, divided by `steps`
             (bench_crc, bench_bloom: back-to-back launches, no host gaps)
tools/bench_frame.py keeps its own host-clock loop (it switches to fewer steps
when a call takes over a second).

Output: a tool with one record calls emit(out, path) (the JSON line and the
file); a tool with one record per shape calls line(record) as each shape ends,
so a long run shows its progress, and write(all, path) once at the end.

Importing this module touches neither torch nor the library, so --help of
every tool works on a box without a GPU.
"""
import ctypes
import json
import os
import re
import subprocess
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_FLAGS = ["-O2", "-std=c++17", "-shared", "-fPIC"]  # the comparators are baselines: the flags are part of the figure
CPU_HEADER = "cpu_common.hpp"
MIX = 0x9E3779B97F4A7C15  # keys_of: second key half = first half * MIX (mod 2^64)
FILL_SEED = 0x6E616B65


def open_ctx():
    """(library handle, Context(0) bound to torch's current stream, that stream)."""
    import torch
    from nakevaleng_amd import _lib
    L = _lib.lib()
    ctx = _lib.Context(0)
    s = torch.cuda.current_stream()
    ctx.set_stream(s.cuda_stream)
    return L, ctx, s


def build_cpu(name, signatures, flags=(), src_dir=None, build_dir=None):
    """tools/cpu_<name>.cpp as build/cpu_<name>.so: compiled with g++ if the
    library is older than the source or the shared header, loaded, and every
    function of `signatures` ({function: (restype, argtypes)}) declared.
    `flags` adds -pthread (in front of the source) or -l<lib> (behind it)."""
    src_dir = src_dir or os.path.join(ROOT, "tools")
    src = os.path.join(src_dir, f"cpu_{name}.cpp")
    so = os.path.join(build_dir or os.path.join(ROOT, "build"), f"cpu_{name}.so")
    deps = [p for p in (src, os.path.join(src_dir, CPU_HEADER)) if os.path.exists(p)]
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in deps):
        os.makedirs(os.path.dirname(so), exist_ok=True)
        libs = [f for f in flags if f.startswith("-l")]
        subprocess.check_call(["g++", *CPU_FLAGS, *[f for f in flags if f not in libs], src, *libs, "-o", so])
    lib = ctypes.CDLL(so)
    for fn, (restype, argtypes) in signatures.items():
        getattr(lib, fn).restype = restype
        getattr(lib, fn).argtypes = argtypes
    return lib


def sclk():
    """The shader clock the box reports, in MHz, or None (read only)."""
    try:
        smi = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=30).stdout
        m = re.search(r"sclk.*?\((\d+)Mhz\)", smi)
        return int(m.group(1)) if m else None
    except Exception:
        return None


def _event_once(stream, fn):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def event_ms(stream, fn, warmup, steps, before=None):
    """ms of each of `steps` calls after `warmup`; `before` runs in front of
    every call, outside the timed pair."""
    ms = []
    for it in range(warmup + steps):
        if before:
            before()
        t = _event_once(stream, fn)
        if it >= warmup:
            ms.append(t)
    return ms


def alternating_ms(stream, fns, warmup, steps):
    """event_ms of several calls that alternate call by call: one list per call."""
    ms = [[] for _ in fns]
    for it in range(warmup + steps):
        for kept, fn in zip(ms, fns):
            t = _event_once(stream, fn)
            if it >= warmup:
                kept.append(t)
    return ms


def phase_ms(ctx, fn, warmup, steps):
    """(wall ms, first interval ms, second interval ms) of `steps` calls after
    `warmup`; fn synchronizes (in the library or itself), so the wall clock
    holds the whole call."""
    for _ in range(warmup):
        fn()
    ctx.set_timing(True)
    call, first, second = [], [], []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        call.append((time.perf_counter() - t0) * 1e3)
        a, b = ctx.last_timing()
        first.append(a)
        second.append(b)
    ctx.set_timing(False)
    return call, first, second


def batch_ms(stream, fn, warmup, steps):
    """ms per call of `steps` back-to-back calls between one pair of events."""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(steps):
        fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


_hip = None


def memcpy_ms(stream, dst, src, nbytes, warmup, steps):
    """event_ms of hipMemcpyDtoDAsync(dst, src, nbytes) on the stream: the
    comparator of every copy and writer kernel.  dst, src: device tensors."""
    global _hip
    if _hip is None:
        _hip = ctypes.CDLL("libamdhip64.so.7")
        _hip.hipMemcpyDtoDAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]

    def copy():
        rc = _hip.hipMemcpyDtoDAsync(dst.data_ptr(), src.data_ptr(), nbytes, stream.cuda_stream)
        if rc != 0:
            raise RuntimeError(f"hipMemcpyDtoDAsync -> {rc}")

    return event_ms(stream, copy, warmup, steps)


def median(samples):
    return float(np.median(samples))


def put(out, key, samples, digits):
    """out[key] = the median, out[key + "_min_max"] = [min, max], rounded to
    `digits`; returns the unrounded median."""
    med = median(samples)
    out[key] = round(med, digits)
    out[key + "_min_max"] = [round(min(samples), digits), round(max(samples), digits)]
    return med


def line(out):
    print(json.dumps(out), flush=True)


def write(out, path):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def emit(out, path):
    """The JSON line on stdout and the file."""
    line(out)
    write(out, path)


# ---- record synthesis

def keys_of(u):
    """16-byte keys of the uint64 array u: u big-endian, then u * MIX big-endian
    (ascending u = ascending key)."""
    k = np.empty((u.size, 16), np.uint8)
    k[:, :8] = u.astype(">u8").view(np.uint8).reshape(-1, 8)
    k[:, 8:] = (u * np.uint64(MIX)).astype(">u8").view(np.uint8).reshape(-1, 8)
    return k


def distinct_u64(rng, n):
    """n distinct uint64 below 2^63, ascending."""
    u = np.unique(rng.integers(0, 2**63, n, dtype=np.uint64))
    assert u.size == n, "a key was drawn twice: pick another seed"
    return u


def size_fields(key_bytes, value_bytes):
    """Bytes 14-30 of a record header: KeySize, ValueSize (little-endian uint64)."""
    return np.frombuffer(np.asarray([key_bytes, value_bytes], "<u8").tobytes(), np.uint8).copy()


def host_records(keys, value_bytes, values=None):
    """(n, 30 + key bytes + value_bytes) records as record.Serialize lays them
    out, of the (n, key bytes) keys: Timestamp 7, the size fields, the keys, the
    values (zeros if None); the rest of the header zero (no reader here looks
    at the Crc).  device_log's layout in host memory."""
    n, ks = keys.shape
    rec = np.zeros((n, 30 + ks + value_bytes), np.uint8)
    rec[:, 4] = 7
    rec[:, 14:30] = size_fields(ks, value_bytes)
    rec[:, 30:30 + ks] = keys
    if values is not None:
        rec[:, 30 + ks:] = values
    return rec


def host_table(rng, n, value_bytes=100):
    """(records, u): n records of strictly increasing keys keys_of(u) and
    random values."""
    u = distinct_u64(rng, n)
    return host_records(keys_of(u), value_bytes, np.frombuffer(rng.bytes(n * value_bytes), np.uint8)
                        .reshape(n, value_bytes)), u


def device_log(ctx, n, key_bytes, value_bytes, keys=None, seed=FILL_SEED):
    """n records of 30 + key_bytes + value_bytes bytes on the device, as one
    uint8 tensor: the bytes of nkv_fill_splitmix64_dev(seed) with the size
    fields set and, if given, the (n, key_bytes) host keys."""
    import torch
    from nakevaleng_amd import _lib
    rb = 30 + key_bytes + value_bytes
    d_log = torch.empty(n * rb, dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib().nkv_fill_splitmix64_dev(ctx.h, d_log.data_ptr(), n * rb, seed))
    ctx.sync()  # the context need not be on torch's stream
    v = d_log.view(n, rb)
    v[:, 14:30] = torch.from_numpy(size_fields(key_bytes, value_bytes)).cuda()
    if keys is not None:
        v[:, 30:30 + key_bytes] = torch.from_numpy(np.ascontiguousarray(keys)).cuda()
    return d_log
