"""GPU: "distinct contexts may be used concurrently" (include/nkv_merkle.h,
Thread safety) -- four host threads, each with its own context on the
context's own stream, run the device API at the same time.

All torch work (allocation, upload, one synchronize) happens on the main
thread before the workers start; a worker makes only C-ABI calls (ctypes
releases the GIL for each, so the calls overlap) and nkv_ctx_sync.  Every
worker runs three rounds of its own rotation of six entries into per-round
outputs (device outputs in tests/guarded.py buffers); afterwards the main
thread compares every output of every round with the oracle.  The cgo shim and
nkv_group_trees_from_values rely on this promise.
"""
import ctypes
import threading
import time

import numpy as np
import pytest

from tests.guarded import frozen, guarded

pytestmark = pytest.mark.gpu

WORKERS = 4
ROUNDS = 3
JOIN_S = 120
N_VALUES = 4097
N_HOST = 700
N_RECORDS = 4097
BLOOM_M, BLOOM_K, BLOOM_SEED = 2 * 32768 + 1, 7, 2**32 - 4

VARIANTS = {
    "defaults": [{}] * WORKERS,
    "mixed_options": [{"BUCKET": 0, "BLOOM_PATH": 0}, {"BUCKET": 1, "BLOOM_PATH": 1}, {"BUCKET": 2, "BLOOM_PATH": 2},
                      {"BUCKET": 1, "BLOOM_PATH": 0}],
}


def _packed(lens):
    off = np.zeros(len(lens), np.uint64)
    off[1:] = np.cumsum(lens[:-1])
    return off


def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


_plans = {}


def plan(oracle, w):
    """Worker w's inputs and the oracle's outputs for them (host side, cached)."""
    if w in _plans:
        return _plans[w]
    from nakevaleng_amd import record
    from tests.test_gpu_merge import expected, fuzz_runs, tables_of
    rng = np.random.default_rng(0x7EAD + w)
    p = {}
    lens = rng.integers(0, 201, N_VALUES).astype(np.uint64)
    off = _packed(lens)
    data = oracle.splitmix64_bytes(int(off[-1] + lens[-1]) + 1, 0x7EAD + w)
    p["values"] = (data, off, lens)
    p["nodes"] = oracle.tree_from_digests(oracle.leaf_hashes(data, off, lens))
    p["crc"] = np.asarray([oracle.crc32(data[int(o):int(o + l)]) for o, l in zip(off, lens)], np.uint32)
    hl = rng.integers(0, 201, N_HOST).astype(np.uint64)
    ho = _packed(hl)
    hd = oracle.splitmix64_bytes(int(ho[-1] + hl[-1]) + 1, 0x405 + w)
    p["host"] = (hd, ho, hl)
    p["host_nodes"] = oracle.tree_from_digests(oracle.leaf_hashes(hd, ho, hl))
    p["host_img"] = oracle.bfs_image(p["host_nodes"], N_HOST)
    recs = [record.New(rng.bytes(int(rng.integers(0, 40))), rng.bytes(int(rng.integers(0, 201))), timestamp=i)
            for i in range(N_RECORDS)]
    stream, sizes = record.data_table(recs)
    roff = _packed(np.ascontiguousarray(sizes, dtype=np.uint64))
    buf = np.frombuffer(stream, np.uint8).copy()
    voff, vlen = record.value_spans(stream, sizes)
    p["rec_nodes"] = oracle.tree_from_digests(oracle.leaf_hashes(buf, voff, vlen))
    p["rec_crc"] = oracle.record_crcs(buf, roff)[0]
    bad = 1000 + w
    buf[int(roff[bad]) + 2] ^= 0x04  # one stored Crc wrong, another record per worker
    p["records"] = (buf, roff)
    p["rec_stats"] = np.asarray([1, bad, 0], np.uint64)
    klen = np.asarray([r.KeySize for r in recs], np.uint64)
    p["bits"] = oracle.bloom_insert(buf, roff + np.uint64(30), klen, BLOOM_M, BLOOM_K, BLOOM_SEED)
    runs = fuzz_runs(rng, 3, nmax=120, vmax=300)
    p["tabs"] = tables_of(runs)
    p["merged"] = expected(runs)
    _plans[w] = p
    return p


class Worker:
    """One context, its uploaded inputs, its per-round outputs and the C calls
    of its rotation, all prepared on the main thread."""

    def __init__(self, _lib, oracle, w, opts):
        self.L = L = _lib.lib()
        self.w, self.p = w, plan(oracle, w)
        p = self.p
        self.ctx = _lib.Context(0)
        for k, v in opts.items():
            self.ctx.set_option(getattr(_lib, "NKV_OPT_" + k), v)
        h = self.ctx.h
        self.keep = []
        self.rc = []
        self.error = None

        def dev(*arrays):
            t = [_up(a) for a in arrays]
            self.keep += t
            return [x.data_ptr() for x in t]

        d_val = dev(*p["values"])
        d_rec = dev(*p["records"])
        rec_len = p["records"][0].size
        d_runs = []
        total = n_all = 0
        for data, off in p["tabs"]:
            d_runs.append((dev(np.frombuffer(data + b"\0", np.uint8), off if len(off) else np.zeros(1, np.uint64)),
                           len(data), len(off)))
            total += len(data)
            n_all += len(off)
        self.runs = (_lib.NkvRun * 3)(*[_lib.NkvRun(d[0] if n else None, nb, d[1] if n else None, n)
                                        for d, nb, n in d_runs])
        tot = 20 * L.nkv_total_nodes(N_VALUES)
        rtot = 20 * L.nkv_total_nodes(N_RECORDS)
        words = (BLOOM_M + 31) // 32 * 4
        hd, ho, hl = p["host"]
        self.out = []  # per round: name -> check() / host arrays
        self.calls = []  # per round: the six calls in this worker's order
        for r in range(ROUNDS):
            o = {}
            g = {name: guarded(nbytes, at, **kw) for name, nbytes, at, kw in [
                ("tree", tot, 4, {}), ("v_nodes", rtot, 12, {}), ("v_crc", 4 * N_RECORDS, 4, {}), ("v_stats", 24, 8, {}),
                ("m_out", total, 1 + 2 * r, {}), ("m_off", 8 * n_all, 8, {}), ("m_src", 8 * n_all, 0, {}),
                ("bits", words, 4, {"init": np.zeros(words, np.uint8)}), ("crc", 4 * N_VALUES, 12, {})]}
            o["checks"] = {k: v[1] for k, v in g.items()}
            o["host_nodes"] = np.zeros((L.nkv_total_nodes(N_HOST), 20), np.uint8)
            o["host_root"] = np.zeros(20, np.uint8)
            o["host_img"] = np.zeros(L.nkv_bfs_size(N_HOST), np.uint8)
            o["n_out"], o["out_len"] = ctypes.c_uint64(), ctypes.c_uint64()
            ptr = {k: v[0] for k, v in g.items()}
            six = [
                lambda ptr=ptr: L.nkv_tree_from_values_dev(h, *d_val, N_VALUES, ptr["tree"]),
                lambda ptr=ptr: L.nkv_tree_verify_records_dev(h, d_rec[0], rec_len, d_rec[1], N_RECORDS, ptr["v_nodes"],
                                                              ptr["v_crc"], ptr["v_stats"]),
                lambda ptr=ptr, o=o: L.nkv_merge_records_dev(h, self.runs, 3, ptr["m_out"], total, ptr["m_off"],
                                                             ptr["m_src"], ctypes.byref(o["n_out"]),
                                                             ctypes.byref(o["out_len"])),
                lambda ptr=ptr: L.nkv_bloom_insert_records_dev(h, d_rec[0], rec_len, d_rec[1], N_RECORDS, BLOOM_M,
                                                               BLOOM_K, BLOOM_SEED, ptr["bits"]),
                lambda ptr=ptr: L.nkv_crc32_dev(h, *d_val, N_VALUES, ptr["crc"]),
                lambda o=o: L.nkv_tree_from_values(h, _lib.p8(hd), _lib.p64(ho), _lib.p64(hl), N_HOST,
                                                   _lib.p8(o["host_root"]), _lib.p8(o["host_nodes"]),
                                                   _lib.p8(o["host_img"])),
            ]
            first = (w + 2 * r) % 6
            self.calls.append(six[first:] + six[:first])
            self.out.append(o)
        self.sync = lambda: L.nkv_ctx_sync(h)

    def freeze(self):
        self.intact = [frozen(t) for t in self.keep]

    def run(self, barrier):
        """The worker thread: C-ABI calls only."""
        try:
            barrier.wait(JOIN_S)
            for calls in self.calls:
                for call in calls:
                    self.rc.append(call())
            self.rc.append(self.sync())
        except BaseException as e:  # reported by the main thread
            self.error = e

    def verify(self):
        p = self.p
        assert self.error is None, self.error
        assert self.rc == [0] * (6 * ROUNDS + 1), (self.w, self.rc)
        want_stream, want_off, want_src = p["merged"]
        nbits = (BLOOM_M + 7) // 8
        for r, o in enumerate(self.out):
            c = o["checks"]
            where = (self.w, r)
            assert np.array_equal(c["tree"]().reshape(-1, 20), p["nodes"]), where
            assert np.array_equal(c["v_nodes"]().reshape(-1, 20), p["rec_nodes"]), where
            assert np.array_equal(c["v_crc"]().view(np.uint32), p["rec_crc"]), where
            assert np.array_equal(c["v_stats"]().view(np.uint64), p["rec_stats"]), where
            assert (o["n_out"].value, o["out_len"].value) == (len(want_off), len(want_stream)), where
            n, nb = len(want_off), len(want_stream)
            assert c["m_out"]()[:nb].tobytes() == want_stream, where
            assert np.array_equal(c["m_off"]().view(np.uint64)[:n], want_off), where
            assert np.array_equal(c["m_src"]().view(np.uint64)[:n], want_src), where
            bits = c["bits"]()
            assert np.array_equal(bits[:nbits], p["bits"]) and not bits[nbits:].any(), where
            assert np.array_equal(c["crc"]().view(np.uint32), p["crc"]), where
            assert np.array_equal(o["host_nodes"], p["host_nodes"]), where
            assert o["host_root"].tobytes() == p["host_nodes"][-1].tobytes(), where
            assert o["host_img"].tobytes() == p["host_img"], where
        for check in self.intact:
            check()


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_distinct_contexts_on_distinct_threads(nkv, oracle, variant):
    import torch
    _lib, _ = nkv
    workers, threads = [], []
    try:
        for w in range(WORKERS):
            workers.append(Worker(_lib, oracle, w, VARIANTS[variant][w]))
        torch.cuda.synchronize()
        for wk in workers:
            wk.freeze()
        barrier = threading.Barrier(WORKERS)
        threads = [threading.Thread(target=wk.run, args=(barrier,), daemon=True) for wk in workers]
        for t in threads:
            t.start()
        deadline = time.monotonic() + JOIN_S
        for t in threads:
            t.join(max(0.0, deadline - time.monotonic()))
        stuck = [i for i, t in enumerate(threads) if t.is_alive()]
        if stuck:
            pytest.exit(f"test_gpu_threads: workers {stuck} have not returned after {JOIN_S} s; "
                        "nothing more is started on the GPU in this run", returncode=3)
        torch.cuda.synchronize()
        for wk in workers:
            wk.verify()
    finally:
        if not any(t.is_alive() for t in threads):
            for wk in workers:
                wk.ctx.close()
