"""The bench layer (tools/benchlib.py) and the drivers over it, without a GPU:
the figure writer against committed profiles, the comparator build, the shared
record synthesis, every driver's --help, and a guard against the helpers being
copied back into a driver.  One GPU test runs the smallest driver end to end."""
import glob
import json
import os
import re
import subprocess
import sys
import zlib

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = os.path.join(ROOT, "tools")
sys.path.insert(0, TOOLS)
import benchlib  # noqa: E402

from nakevaleng_amd import record  # noqa: E402

DRIVERS = sorted(glob.glob(os.path.join(TOOLS, "bench_*.py")))
COMPARATORS = sorted(glob.glob(os.path.join(TOOLS, "cpu_*.cpp")))


def profile(name):
    with open(os.path.join(ROOT, "profiles", name)) as f:
        return json.load(f)


def test_the_tools_are_all_here():
    assert len(DRIVERS) == 11 and len(COMPARATORS) == 9


# ---- put and median

def committed_figures():
    yield profile("memtable_bench.json")["mixes"][0], "add_ms", 4
    yield profile("sort_bench.json")["shapes"][0], "call_ms", 3
    yield profile("merge_bench.json"), "copy_ms", 3


@pytest.mark.parametrize("rec,key,digits", list(committed_figures()), ids=["memtable", "sort", "merge"])
def test_put_writes_what_the_inline_code_wrote(rec, key, digits):
    med, (lo, hi) = rec[key], rec[key + "_min_max"]
    d = min(med - lo, hi - med) / 2
    for samples in ([hi, med, lo], [hi, med - d, lo, med + d], [med] * 3 + [lo, hi]):
        out = {}
        got = benchlib.put(out, key, samples, digits)
        assert out == {key: med, key + "_min_max": [lo, hi]}
        # the drivers' inline code before the layer
        assert out[key] == round(float(np.median(samples)), digits)
        assert out[key + "_min_max"] == [round(min(samples), digits), round(max(samples), digits)]
        assert got == benchlib.median(samples) == float(np.median(samples))
        assert list(out) == [key, key + "_min_max"]


def test_put_rounds_and_returns_the_unrounded_median():
    out = {"kept": 1}
    got = benchlib.put(out, "x_ms", [0.12344, 0.12346, 0.5], 4)
    assert got == 0.12346 and out == {"kept": 1, "x_ms": 0.1235, "x_ms_min_max": [0.1234, 0.5]}
    assert isinstance(benchlib.median(np.asarray([1, 2], np.float32)), float)


def test_emit_line_and_file(tmp_path, capsys):
    path = os.path.join(str(tmp_path), "new", "dir", "x.json")
    out = {"a": [1, 2], "b": {"c": 0.5}}
    benchlib.emit(out, path)
    assert capsys.readouterr().out == json.dumps(out) + "\n"
    with open(path) as f:
        assert f.read() == json.dumps(out, indent=1) + "\n"


# ---- build_cpu

SRC = 'extern "C" int answer() { return %d; }\n'


def test_build_cpu_builds_once_and_rebuilds_when_stale(tmp_path, monkeypatch):
    import ctypes
    src_dir, build_dir = os.path.join(str(tmp_path), "src"), os.path.join(str(tmp_path), "out", "build")
    os.makedirs(src_dir)
    src = os.path.join(src_dir, "cpu_probe.cpp")
    with open(src, "w") as f:
        f.write(SRC % 41)
    calls = []
    real = subprocess.check_call
    monkeypatch.setattr(benchlib.subprocess, "check_call", lambda cmd, *a, **k: (calls.append(cmd), real(cmd, *a, **k)))
    sig = {"answer": (ctypes.c_int, [])}

    lib = benchlib.build_cpu("probe", sig, ["-pthread", "-lz"], src_dir=src_dir, build_dir=build_dir)
    so = os.path.join(build_dir, "cpu_probe.so")
    assert lib.answer() == 41 and lib.answer.restype is ctypes.c_int and os.path.exists(so)
    # today's command line: the fixed flags, -pthread in front of the source, -l behind it
    assert calls == [["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-pthread", src, "-lz", "-o", so]]

    os.utime(so, (os.path.getmtime(src) + 10,) * 2)  # the library newer than the source: no rebuild
    benchlib.build_cpu("probe", sig, src_dir=src_dir, build_dir=build_dir)
    assert len(calls) == 1

    os.utime(src, (os.path.getmtime(so) + 10,) * 2)  # the source moved forward: rebuild
    benchlib.build_cpu("probe", sig, src_dir=src_dir, build_dir=build_dir)
    assert calls[1:] == [["g++", "-O2", "-std=c++17", "-shared", "-fPIC", src, "-o", so]]

    hdr = os.path.join(src_dir, benchlib.CPU_HEADER)  # so does a newer shared header
    with open(hdr, "w") as f:
        f.write("// nothing\n")
    os.utime(hdr, (os.path.getmtime(so) + 10,) * 2)
    benchlib.build_cpu("probe", sig, src_dir=src_dir, build_dir=build_dir)
    assert len(calls) == 3


def test_build_cpu_raises_when_the_compiler_fails(tmp_path):
    src_dir = str(tmp_path)
    with open(os.path.join(src_dir, "cpu_broken.cpp"), "w") as f:
        f.write("this is not C++\n")
    with pytest.raises(subprocess.CalledProcessError):
        benchlib.build_cpu("broken", {}, src_dir=src_dir, build_dir=os.path.join(src_dir, "build"))
    assert not os.path.exists(os.path.join(src_dir, "build", "cpu_broken.so"))


def test_the_comparators_keep_their_flags(monkeypatch):
    """-pthread and -lz only where the tool had them before the layer: what
    each driver's cpu_lib() hands to build_cpu."""
    import importlib
    want = {"sort": [], "merge": [], "index": [], "frame": [], "lookup": ["-pthread"], "locate": ["-pthread"],
            "memtable": ["-pthread"], "sketch": ["-pthread"], "encode": ["-pthread", "-lz"]}
    seen = {}
    monkeypatch.setattr(benchlib, "build_cpu",
                        lambda name, signatures, flags=(): seen.update({name: (list(flags), signatures)}))
    for name in want:
        importlib.import_module(f"bench_{name}").cpu_lib()
    assert {name: flags for name, (flags, _) in seen.items()} == want
    for name, (_, signatures) in seen.items():  # every declared function is one the source defines
        with open(os.path.join(TOOLS, f"cpu_{name}.cpp")) as f:
            text = f.read()
        assert signatures and all(re.search(rf"\b{fn}\s*\(", text) for fn in signatures), name


# ---- the timing loops, on a stub of torch's events

class FakeTorch:
    """torch.cuda.Event / synchronize that write down what is done to them."""

    def __init__(self):
        fake, self.log, self.made = self, [], 0

        class Event:
            def __init__(self, enable_timing=False):
                assert enable_timing
                fake.made += 1
                self.id = fake.made

            def record(self, stream):
                fake.log.append(("record", self.id, stream))

            def elapsed_time(self, other):
                assert other.id == self.id + 1  # the pair made together
                return float(self.id)

        class cuda:
            pass

        cuda.Event = Event
        cuda.synchronize = lambda: self.log.append(("sync",))
        self.cuda = cuda


@pytest.fixture
def fake_torch(monkeypatch):
    fake = FakeTorch()
    monkeypatch.setitem(sys.modules, "torch", fake)
    return fake


@pytest.mark.parametrize("warmup,steps", [(0, 1), (1, 3), (5, 30)])
def test_event_ms_discipline(fake_torch, warmup, steps):
    log = fake_torch.log
    ms = benchlib.event_ms("s", lambda: log.append(("fn",)), warmup, steps, before=lambda: log.append(("before",)))
    assert len(ms) == steps  # the kept samples
    assert fake_torch.made == 2 * (warmup + steps)  # a fresh pair per call
    # the kept samples are the last `steps` pairs: the warm-up ones are dropped, not the late ones
    assert ms == [float(2 * it + 1) for it in range(warmup, warmup + steps)]
    want = []
    for it in range(warmup + steps):  # before() outside the pair, one synchronize after each call
        want += [("before",), ("record", 2 * it + 1, "s"), ("fn",), ("record", 2 * it + 2, "s"), ("sync",)]
    assert log == want
    log.clear()
    assert len(benchlib.event_ms("s", lambda: None, warmup, steps)) == steps and ("before",) not in log


def test_alternating_ms_takes_turns(fake_torch):
    log = fake_torch.log
    a, b = benchlib.alternating_ms("s", (lambda: log.append("a"), lambda: log.append("b")), 2, 3)
    assert len(a) == len(b) == 3
    assert [x for x in log if isinstance(x, str)] == ["a", "b"] * 5
    assert a == [9.0, 13.0, 17.0] and b == [11.0, 15.0, 19.0]  # pairs 5.., each call its own fresh pair
    assert log.count(("sync",)) == 10


def test_memcpy_ms_is_event_ms_of_the_copy(fake_torch, monkeypatch):
    calls = []

    class Hip:
        @staticmethod
        def hipMemcpyDtoDAsync(dst, src, n, stream):
            calls.append((dst, src, n, stream))
            return 0 if n else 1

    class T:
        def __init__(self, p):
            self.p = p

        def data_ptr(self):
            return self.p

    class S:
        cuda_stream = 77

    monkeypatch.setattr(benchlib, "_hip", Hip)
    assert len(benchlib.memcpy_ms(S, T(1), T(2), 64, 2, 4)) == 4
    assert calls == [(1, 2, 64, 77)] * 6 and fake_torch.made == 12
    with pytest.raises(RuntimeError):
        benchlib.memcpy_ms(S, T(1), T(2), 0, 0, 1)


class FakeCtx:
    def __init__(self, log):
        self.log, self.on, self.n = log, False, 0

    def set_timing(self, on):
        self.on = on
        self.log.append(("timing", on))

    def last_timing(self):
        assert self.on
        self.n += 1
        return 10.0 + self.n, 20.0 + self.n


@pytest.mark.parametrize("warmup,steps", [(0, 1), (2, 3)])
def test_phase_ms_discipline(warmup, steps):
    log = []
    ctx = FakeCtx(log)
    call, first, second = benchlib.phase_ms(ctx, lambda: log.append(("fn", ctx.on)), warmup, steps)
    assert len(call) == len(first) == len(second) == steps and all(c >= 0 for c in call)
    assert first == [11.0 + i for i in range(steps)] and second == [21.0 + i for i in range(steps)]
    # the timing events are switched on only after the warm-up, and off again
    assert log == [("fn", False)] * warmup + [("timing", True)] + [("fn", True)] * steps + [("timing", False)]


def test_batch_ms_is_one_pair_around_all_the_steps(fake_torch):
    log = fake_torch.log
    ms = benchlib.batch_ms("s", lambda: log.append(("fn",)), 2, 4)
    assert fake_torch.made == 2 and ms == 1.0 / 4
    assert log == [("fn",)] * 2 + [("sync",), ("record", 1, "s")] + [("fn",)] * 4 + [("record", 2, "s"), ("sync",)]


# ---- record synthesis

def test_keys_of_order_and_second_half():
    rng = np.random.default_rng(1)
    u = np.unique(np.concatenate([rng.integers(0, 2**63, 500, dtype=np.uint64),
                                  np.asarray([0, 1, 255, 256, 2**32 - 1, 2**32, 2**63 - 1], np.uint64)]))
    k = benchlib.keys_of(u)
    assert k.shape == (u.size, 16) and k.dtype == np.uint8
    as_bytes = [bytes(row) for row in k]
    assert as_bytes == sorted(as_bytes) and len(set(as_bytes)) == u.size
    for x, row in zip(u.tolist(), as_bytes):
        assert row[:8] == x.to_bytes(8, "big")
        assert row[8:] == ((x * benchlib.MIX) % 2**64).to_bytes(8, "big")


def parse_all(rec):
    """Every row through record.parse (the Crc field filled in first: the benches leave it zero)."""
    out = []
    for row in rec:
        buf = bytearray(row.tobytes())
        ks = int.from_bytes(buf[14:22], "little")
        buf[0:4] = (zlib.crc32(bytes(buf[30:])) & 0xFFFFFFFF).to_bytes(4, "little")
        r, end = record.parse(bytes(buf))
        assert end == len(buf) and (r.KeySize, len(r.Key)) == (ks, ks)
        out.append(r)
    return out


@pytest.mark.parametrize("vs", [100, 0, 7])
def test_host_table_records_parse_and_ascend(vs):
    rec, u = benchlib.host_table(np.random.default_rng(2), 257, vs)
    assert rec.shape == (257, 30 + 16 + vs) and (np.diff(u.astype(object)) > 0).all()
    recs = parse_all(rec)
    assert all(int.from_bytes(row[14:22].tobytes(), "little") == 16 for row in rec)
    assert all(int.from_bytes(row[22:30].tobytes(), "little") == vs for row in rec)
    assert all((r.KeySize, r.ValueSize, r.Timestamp, r.Status) == (16, vs, 7, 0) for r in recs)
    keys = [r.Key for r in recs]
    assert all(a < b for a, b in zip(keys, keys[1:])) and keys == [bytes(k) for k in benchlib.keys_of(u)]
    if vs:
        assert len({r.Value for r in recs}) > 1  # random values


@pytest.mark.parametrize("ks,vs", [(16, 100), (17, 4096), (1, 0)])
def test_host_mirror_of_device_log(ks, vs):
    """host_records lays out what device_log lays out: the same size fields at
    the same bytes, the keys behind the header."""
    n = 33
    keys = np.unique(np.random.default_rng(3).integers(0, 256, (n, ks), dtype=np.uint8), axis=0)  # rows ascending
    rec = benchlib.host_records(keys, vs)
    assert rec.shape == (keys.shape[0], 30 + ks + vs)
    assert bytes(benchlib.size_fields(ks, vs)) == ks.to_bytes(8, "little") + vs.to_bytes(8, "little")
    assert (rec[:, 14:22] == np.frombuffer(ks.to_bytes(8, "little"), np.uint8)).all()
    assert (rec[:, 22:30] == np.frombuffer(vs.to_bytes(8, "little"), np.uint8)).all()
    recs = parse_all(rec)
    got = [r.Key for r in recs]
    assert got == [bytes(k) for k in keys] and all(a < b for a, b in zip(got, got[1:]))
    assert all(r.ValueSize == vs and r.Value == bytes(vs) for r in recs)


# ---- the drivers

@pytest.mark.parametrize("tool", DRIVERS, ids=[os.path.basename(t) for t in DRIVERS])
def test_help_needs_no_gpu(tool):
    out = subprocess.run([sys.executable, tool, "--help"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.startswith("usage:"), out.stdout + out.stderr[-3000:]


def test_importing_the_layer_loads_neither_torch_nor_the_library():
    code = "import sys; sys.path.insert(0, %r); import benchlib; " \
           "assert 'torch' not in sys.modules and 'nakevaleng_amd._lib' not in sys.modules" % TOOLS
    assert subprocess.run([sys.executable, "-c", code], timeout=120).returncode == 0


def test_the_helpers_are_defined_once():
    for tool in DRIVERS:
        with open(tool) as f:
            text = f.read()
        assert "import benchlib" in text, tool
        for copied in ("def build_cpu", "rocm-smi", "hipMemcpyDtoDAsync.argtypes", "torch.cuda.Event(",
                       "json.dump", "np.median"):
            assert copied not in text, (tool, copied)
    for src in COMPARATORS:
        with open(src) as f:
            text = f.read()
        assert '#include "cpu_common.hpp"' in text, src
        for copied in (r"\ble64\s*\(const uint8_t\s*\*\s*\w+\)\s*\{", r"std::chrono::", r"std::thread\b",
                       r"\bmemcmp\s*\("):
            assert not re.search(copied, text), (src, copied)


# ---- on a device

def keys_under(x):
    if isinstance(x, dict):
        return set(x) | set().union(*[keys_under(v) for v in x.values()])
    if isinstance(x, list):
        return set().union(*[keys_under(v) for v in x])
    return set()


@pytest.mark.gpu
def test_bench_memtable_runs_small(tmp_path):
    """The smallest driver end to end in a child process: open_ctx, device_log,
    event_ms with a `before` hook, put and emit on a device.  The tool's own
    host verification gates the run."""
    path = os.path.join(str(tmp_path), "memtable.json")
    run = subprocess.run([sys.executable, os.path.join(TOOLS, "bench_memtable.py"), "--records", "4096", "--mixes",
                          "distinct,single", "--steps", "3", "--warmup", "1", "--no-cpu", "--out", path],
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr[-3000:]
    lines = [json.loads(x) for x in run.stdout.splitlines() if x.startswith("{")]
    with open(path) as f:
        written = json.load(f)
    committed = profile("memtable_bench.json")
    assert written == {"metric": committed["metric"], "mixes": lines}
    assert [m["mix"] for m in lines] == ["distinct", "single"]
    known = keys_under(committed["mixes"])
    figures = {k for k in known if k.endswith("_ms") and not k.startswith("cpu")}
    assert figures == {"add_ms", "find_ms", "sort_ms", "lookup_ms"}
    for m in lines:
        assert set(m) <= known, set(m) - known
        assert (m["records"], m["steps"], m["warmup"], m["verified_vs_host"]) == (4096, 3, 1, True)
        for k in figures:  # 3 kept samples: a median inside [min, max], all positive
            lo, hi = m[k + "_min_max"]
            assert 0 < lo <= m[k] <= hi, (k, m[k], lo, hi)
