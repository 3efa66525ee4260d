"""GPU: the live memtable on the device (nkv_memtable_clear_dev / _add_dev /
_find_dev, memtable.Memtable, lsmtree.get_many(memtable=)) against
tests/live_memtable_ref.py: every byte of d_is_new, d_state, d_hit and d_status.
Outputs lie in guarded buffers of exactly their size at their minimum alignment
plus odd multiples (tests/guarded.py); inputs are snapshotted and compared after
every call.  The index's own bytes are opaque and never compared between runs.
add_closed / find_closed are the oracle here; tests/test_live_memtable_ref.py
holds them to the literal restatement."""
import numpy as np
import pytest

from nakevaleng_amd import record
from tests import live_memtable_ref as ref
from tests.guarded import frozen, guarded
from tests.test_live_memtable_ref import BOTH, CAP, THR, rec

pytestmark = pytest.mark.gpu

INVALID = 2  # NKV_ERR_INVALID
FILL = 0xA5
NONE = ref.NONE


def _torch():
    import torch
    return torch


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


def slots_for(n):
    s = 2
    while s < 2 * n:
        s *= 2
    return s


def offsets_of(sizes):
    off = np.zeros(len(sizes), np.uint64)
    if len(sizes) > 1:
        off[1:] = np.cumsum(np.asarray(sizes, np.uint64)[:-1])
    return off


def pack_keys(keys, at=0):
    """(bytes with `at` bytes in front, offsets, lengths) of query keys packed back to back."""
    klen = np.fromiter((len(k) for k in keys), dtype=np.uint64, count=len(keys))
    koff = offsets_of(klen) + np.uint64(at)
    return np.frombuffer(bytes(at) + b"".join(keys) + b"\0", np.uint8), koff, klen


class Dev:
    """One memtable on the device over a log that is already there: p_log /
    p_off are device addresses, off the offsets on the host, nbytes the log's
    length.  `keep` holds the tensors the addresses point into."""

    def __init__(self, nkv, p_log, p_off, off, nbytes, slots, keep=(), intact=(), index_at=8, state_at=8):
        self._lib, self.ctx = nkv
        self.L = self._lib.lib()
        self.p_log, self.p_off, self.off, self.nbytes, self.N = p_log, p_off, off, nbytes, len(off)
        self.slots, self.keep, self.intact = slots, keep, list(intact)
        self.p_index, self.index_check = guarded(8 * slots, index_at, fill=FILL)
        self.p_state, self.state_check = guarded(32, state_at, fill=FILL)
        assert self.L.nkv_memtable_index_bytes(slots) == 8 * slots
        assert self.L.nkv_memtable_clear_dev(self.ctx.h, self.p_index, slots, self.p_state) == 0
        self.ctx.sync()
        assert (self.index_check() == 0xFF).all()
        assert self.state() == [0, 0, 0, NONE]

    @classmethod
    def of(cls, nkv, records, slots=None, log_at=0, **kw):
        data, sizes = record.data_table(records)
        off = offsets_of(sizes)
        buf = np.zeros(log_at + max(len(data), 1), np.uint8)
        buf[log_at:log_at + len(data)] = np.frombuffer(data, np.uint8)
        d_log, d_off = _dev(buf), _dev(off if len(off) else np.zeros(1, np.uint64))
        return cls(nkv, d_log.data_ptr() + log_at, d_off.data_ptr(), off, len(data),
                   slots or slots_for(len(records)), keep=(d_log, d_off), intact=(frozen(d_log), frozen(d_off)), **kw)

    def state(self):
        return self.state_check().view(np.uint64).tolist()

    def log_len(self, n):
        return int(self.off[n]) if n < self.N else self.nbytes

    def add(self, n_done, n, rule=(0, 0, 0), new_at=1, err_at=4, with_new=True, with_err=True, slots=None,
            log_len=None):
        """(rc, d_is_new bytes, d_state words, d_err) of one nkv_memtable_add_dev."""
        torch = _torch()
        p_new, new_check = guarded(max(n - n_done, 0), new_at, fill=FILL)
        p_err, err_check = guarded(4, err_at, fill=FILL)
        torch.cuda.synchronize()
        rc = self.L.nkv_memtable_add_dev(self.ctx.h, self.p_log, self.log_len(n) if log_len is None else log_len,
                                         self.p_off, n_done, n, self.p_index, self.slots if slots is None else slots, rule[0], rule[1],
                                         rule[2], self.p_state, p_new if with_new else None,
                                         p_err if with_err else None)
        torch.cuda.synchronize()
        for f in self.intact:
            f()
        self.index_check()
        return rc, new_check(), self.state(), err_check()

    def find(self, keys, n=None, table_id=0, overlay=0, preset=None, key_at=0, hit_at=8, status_at=1):
        """(hit words, status bytes, d_err word) of one nkv_memtable_find_dev;
        preset = (hit words, status bytes) the outputs hold beforehand."""
        torch = _torch()
        q = len(keys)
        kb, koff, klen = pack_keys(keys, key_at)
        d_keys, d_koff, d_klen = _dev(kb), _dev(koff if q else np.zeros(1, np.uint64)), \
            _dev(klen if q else np.zeros(1, np.uint64))
        ins = [frozen(t) for t in (d_keys, d_koff, d_klen)]
        index_before = self.index_check()
        p_hit, hit_check = guarded(8 * q, hit_at, fill=FILL,
                                   init=None if preset is None else np.asarray(preset[0], np.uint64))
        p_st, st_check = guarded(q, status_at, fill=FILL,
                                 init=None if preset is None else np.asarray(preset[1], np.uint8))
        p_err, err_check = guarded(4, 4, fill=FILL)
        torch.cuda.synchronize()
        n = self.state()[2] if n is None else n
        rc = self.L.nkv_memtable_find_dev(self.ctx.h, self.p_log, self.log_len(n), self.p_off, n, self.p_index,
                                          self.slots, d_keys.data_ptr(), d_koff.data_ptr(), d_klen.data_ptr(), q,
                                          table_id, overlay, p_hit, p_st, p_err)
        torch.cuda.synchronize()
        assert rc == 0
        for f in ins + self.intact:
            f()
        assert np.array_equal(self.index_check(), index_before)  # find writes no index byte
        err = err_check()
        if q == 0:
            assert (err == FILL).all()  # q = 0 writes nothing
            return np.zeros(0, np.uint64), np.zeros(0, np.uint8), 0
        return hit_check().view(np.uint64), st_check(), int(err.view(np.uint32)[0])


def check_add(dev, records, n_done, n, rule, trace=None, **kw):
    trace = trace or ref.add_closed(records, *rule)
    rc, is_new, state, err = dev.add(n_done, n, rule, **kw)
    assert rc == 0 and int(err.view(np.uint32)[0]) == 0
    assert is_new.tolist() == [int(x) for x in trace.is_new[n_done:n]]
    assert state == trace.state(n_done, n)
    return trace


def check_find(dev, records, keys, table_id=0, **kw):
    hit, status, err = dev.find(keys, table_id=table_id, **kw)
    want_hit, want_status = ref.find_closed(records, keys, table_id)
    assert err == 0
    assert hit.tolist() == want_hit and status.tolist() == want_status


def distinct_keys(rng, n, lo=0, hi=40):
    keys, seen = [], set()
    while len(keys) < n:
        k = rng.bytes(int(rng.integers(lo, hi + 1)))
        if k not in seen:
            seen.add(k)
            keys.append(k)
    return keys


def log_from(rng, keys, vmax=200):
    """One write per entry of `keys`, Values of 0..vmax bytes, one in ten a tombstone."""
    return [rec(k, rng.bytes(int(v)), status=int(t), ts=int(ts)) for k, v, t, ts in
            zip(keys, rng.integers(0, vmax + 1, len(keys)), rng.random(len(keys)) < 0.1,
                rng.integers(-3, 4, len(keys)))]


def absent_keys(rng, records, count):
    have = {r.Key for r in records}
    out = [k for k in distinct_keys(rng, 2 * count, 1, 40) if k not in have][:count // 2]
    # absent keys that share a long prefix with a present one: one byte longer, one shorter, last byte changed
    for r in records[:count]:
        for k in (r.Key + b"\0", r.Key[:-1], r.Key[:-1] + bytes([(r.Key[-1] + 1) % 256]) if r.Key else b"\1"):
            if k not in have:
                out.append(k)
    return out


# ---------------------------------------------------------------------------
# counts and load

@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257, 4096, 4097])
def test_distinct_keys(nkv, n):
    """n = 4096 in 8192 slots: load exactly one half, real probe chains."""
    rng = np.random.default_rng(0x6D74 + n)
    log = log_from(rng, distinct_keys(rng, n))
    dev = Dev.of(nkv, log)
    assert dev.slots == slots_for(n) and n <= dev.slots // 2
    check_add(dev, log, 0, n, (BOTH, n // 2 + 1, 10**12), new_at=1 + 2 * (n % 8))
    keys = [r.Key for r in log]
    check_find(dev, log, keys[::-1] + absent_keys(rng, log, 40), key_at=n % 5)


@pytest.mark.parametrize("nkeys", [1, 16])
def test_hot_keys(nkv, nkeys):
    """One key (every lane on one slot) and 16 keys written 4097 times."""
    rng = np.random.default_rng(0x686F74 + nkeys)
    pool = distinct_keys(rng, nkeys, 1, 24)
    n = 4097
    log = log_from(rng, [pool[j] for j in rng.integers(0, nkeys, n)] if nkeys > 1 else pool * n, vmax=60)
    dev = Dev.of(nkv, log)
    check_add(dev, log, 0, n, (THR, 0, 3 * 90))
    check_find(dev, log, pool + pool + absent_keys(rng, log, 8))


@pytest.mark.parametrize("log_at", range(8))
def test_key_lengths_at_every_alignment(nkv, log_at):
    """Keys of 0..40 bytes, the empty key included; the log starts log_at bytes
    past a 256-byte boundary and the Values are ragged, so every key length
    meets every start alignment over the eight cases; so do the queries."""
    rng = np.random.default_rng(0x616C + log_at)
    keys = [rng.bytes(length) for length in range(41)]
    keys = keys + [keys[j] for j in rng.integers(0, 41, 30)]  # and overwrites
    log = log_from(rng, keys, vmax=7)
    dev = Dev.of(nkv, log, log_at=log_at)
    check_add(dev, log, 0, len(log), (CAP, 41, 0))
    check_find(dev, log, keys[:41] + absent_keys(rng, log, 20), key_at=log_at)


@pytest.mark.parametrize("shared", [8, 16, 39])
def test_keys_that_share_a_prefix(nkv, shared):
    rng = np.random.default_rng(0x7072 + shared)
    stem = rng.bytes(shared)
    keys = [stem + bytes([b]) for b in range(70)] + [stem]
    keys += [keys[j] for j in rng.integers(0, len(keys), 60)]
    log = log_from(rng, keys)
    dev = Dev.of(nkv, log)
    check_add(dev, log, 0, len(log), (BOTH, 5, 10**9))
    check_find(dev, log, keys[:71] + [stem + bytes([200]), stem[:-1], stem + b"\0\0"])


# ---------------------------------------------------------------------------
# incremental adds

def test_batches_equal_one_batch_and_runs_agree(nkv):
    rng = np.random.default_rng(0x696E63)
    pool = distinct_keys(rng, 1500)
    log = log_from(rng, [pool[j] for j in rng.integers(0, len(pool), 4097)])
    rule = (BOTH, 700, 10**12)
    trace = ref.add_closed(log, *rule)
    queries = pool[:300] + absent_keys(rng, log, 30)
    answers = []
    for batches in ([(0, 4097)], [(0, 1), (1, 65), (65, 4097)], [(0, 1), (1, 65), (65, 4097)]):
        dev = Dev.of(nkv, log, slots=16384)
        got_new = []
        for n_done, n in batches:
            rc, is_new, state, err = dev.add(n_done, n, rule)
            assert rc == 0 and int(err.view(np.uint32)[0]) == 0
            assert state == trace.state(n_done, n)
            got_new += is_new.tolist()
            if n == 65:  # a find between two adds sees exactly the writes so far
                check_find(dev, log[:65], queries[:50], n=65)
        hit, status, err = dev.find(queries)
        answers.append((got_new, dev.state()[:3], hit.tolist(), status.tolist(), err))
    assert answers[0][0] == [int(x) for x in trace.is_new]
    assert answers[0][2:] == (*ref.find_closed(log, queries), 0)
    assert answers[0] == answers[1] == answers[2]


def test_no_new_write_sets_flush_at_only(nkv):
    log = [rec(b"a", b"1"), rec(b"b", b"2")]
    dev = Dev.of(nkv, log)
    check_add(dev, log, 0, 2, (CAP, 2, 0))
    assert dev.state() == [2, 64, 2, 1]
    rc, is_new, state, err = dev.add(2, 2, (CAP, 2, 0))
    assert rc == 0 and is_new.size == 0 and state == [2, 64, 2, NONE] and int(err.view(np.uint32)[0]) == 0


# ---------------------------------------------------------------------------
# find

def test_find_cases(nkv):
    log = [rec(b"a", b"1", ts=9), rec(b"b", b"2"), rec(b"a", b"", status=1, ts=3), rec(b"b", b"3", ts=0),
           rec(b"c", b"x", status=1), rec(b"c", b"y"), rec(b"", b"empty key"), rec(b"d" * 40, b"")]
    dev = Dev.of(nkv, log)
    check_add(dev, log, 0, len(log), (0, 0, 0))
    keys = [b"a", b"b", b"c", b"", b"d" * 40, b"d" * 39, b"d" * 39 + b"e", b"zz", b"a", b"a", b"c"]
    for table_id in (0, 31):
        check_find(dev, log, keys, table_id=table_id)
        check_find(dev, log, [], table_id=table_id)  # q = 0
    hit, status, _ = dev.find(keys)
    assert status.tolist()[:3] == [ref.TOMBSTONE, ref.LIVE, ref.LIVE] and hit.tolist()[:3] == [2, 3, 5]


@pytest.mark.parametrize("hit_at,status_at", [(8, 1), (24, 3), (8 * 7, 0)])
def test_overlay_leaves_absent_entries_as_they_were(nkv, hit_at, status_at):
    rng = np.random.default_rng(0x6F76)
    log = log_from(rng, distinct_keys(rng, 100, 1, 20))
    dev = Dev.of(nkv, log)
    check_add(dev, log, 0, 100, (0, 0, 0))
    keys = [r.Key for r in log[:40]] + absent_keys(rng, log, 40)
    q = len(keys)
    preset = (rng.integers(0, 2**63, q, dtype=np.uint64), rng.integers(0, 256, q, dtype=np.uint8))
    hit, status, err = dev.find(keys, table_id=31, overlay=1, preset=preset, hit_at=hit_at, status_at=status_at)
    want_hit, want_status = ref.find_closed(log, keys, 31)
    for i in range(q):
        if want_status[i] == ref.ABSENT:
            assert (hit[i], status[i]) == (preset[0][i], preset[1][i])
        else:
            assert (hit[i], status[i]) == (want_hit[i], want_status[i])
    assert err == 0


# ---------------------------------------------------------------------------
# the flush point: the hand cases of tests/test_live_memtable_ref.py, with the
# point in the first batch, in a later batch and nowhere

def _flush_cases():
    first = rec(b"k", b"v" * 10)
    five = [rec(bytes([i]), b"") for i in range(5)]
    six = [rec(bytes([i]), b"v" * 70) for i in range(6)]
    tomb = [rec(b"a", b"1"), rec(b"b", b"2"), rec(b"a", b"", status=1), rec(b"c", b"3")]
    return {
        "overwrite-longer": ([first, rec(b"k", b"v" * 500), rec(b"j", b"")], (THR, 0, 72)),
        "overwrite-shorter": ([first, rec(b"k", b""), rec(b"j", b"")], (THR, 0, 72)),
        "capacity-equality": (five, (CAP, 3, 0)),
        "capacity-overwrite-at-capacity": (five[:3] + [rec(bytes([0]), b"x")], (CAP, 3, 0)),
        "capacity-passed": (five, (CAP, 1, 0)),
        "threshold-only": (six, (THR, 2, 250)),
        "both": (six, (BOTH, 2, 450)),
        "neither": (six, (0, 2, 250)),
        "nowhere": (six, (BOTH, 7, 10**6)),
        "tombstone-latest": (tomb, (BOTH, 3, 10**6)),
    }


@pytest.mark.parametrize("name", sorted(_flush_cases()))
def test_flush_point(nkv, name):
    log, rule = _flush_cases()[name]
    trace = ref.add_literal(log, *rule)
    assert trace == ref.add_closed(log, *rule)
    n = len(log)
    for cut in range(0, n):  # one batch (cut 0), then every split into two
        dev = Dev.of(nkv, log, slots=16)
        if cut:
            check_add(dev, log, 0, cut, rule, trace)
        check_add(dev, log, cut, n, rule, trace)
        check_find(dev, log, [r.Key for r in log] + [b"none"])


# ---------------------------------------------------------------------------
# refusals

def _refused(dev, *args, **kw):
    before = (dev.index_check().copy(), dev.state())
    rc, is_new, state, err = dev.add(*args, **kw)
    assert (is_new == FILL).all()
    assert np.array_equal(dev.index_check(), before[0]) and state == before[1]
    return rc, err


def test_add_refuses_a_wrong_indexed_count(nkv):
    log = [rec(bytes([i]), b"v") for i in range(8)]
    dev = Dev.of(nkv, log)
    check_add(dev, log, 0, 4, (BOTH, 10, 2048))
    for n_done in (3, 5, 0):
        rc, err = _refused(dev, n_done, 8)
        assert rc == 0 and int(err.view(np.uint32)[0]) & 2
    rc, err = _refused(dev, 3, 8, with_err=False)  # no d_err: the call synchronizes and reports it
    assert rc == INVALID and (err == FILL).all()
    check_add(dev, log, 4, 8, (BOTH, 10, 2048))  # and the memtable is still usable


def test_add_refuses_a_record_past_the_log_and_a_gap(nkv):
    log = [rec(bytes([i]), b"value") for i in range(6)]
    dev = Dev.of(nkv, log)
    rc, err = _refused(dev, 0, 6, log_len=dev.nbytes - 1)  # the last record reaches past the log
    assert rc == 0 and int(err.view(np.uint32)[0]) & 1
    rc, err = _refused(dev, 0, 6, log_len=dev.nbytes + 1)  # bytes behind the last record
    assert rc == 0 and int(err.view(np.uint32)[0]) & 1
    # a gap between records: the offsets of a log with one record taken out of the middle
    data, sizes = record.data_table(log)
    off = offsets_of(sizes)
    gap = np.delete(off, 2)
    d_log, d_off = _dev(np.frombuffer(data, np.uint8)), _dev(gap)
    dev = Dev(nkv, d_log.data_ptr(), d_off.data_ptr(), gap, len(data), 16, keep=(d_log, d_off),
              intact=(frozen(d_log), frozen(d_off)))
    rc, err = _refused(dev, 0, 5)
    assert rc == 0 and int(err.view(np.uint32)[0]) & 1
    # and a batch that does not start where the indexed records end
    dev = Dev(nkv, d_log.data_ptr(), d_off.data_ptr(), gap, len(data), 16, keep=(d_log, d_off))
    rc, is_new, state, err = dev.add(0, 2, log_len=int(off[2]))
    assert rc == 0 and state[:3] == [2, 72, 2]
    rc, err = _refused(dev, 2, 5)
    assert rc == 0 and int(err.view(np.uint32)[0]) & 1


def test_add_refuses_bad_arguments_with_nothing_written(nkv):
    log = [rec(bytes([i]), b"") for i in range(9)]
    dev = Dev.of(nkv, log, slots=16)
    for kw in ({"slots": 12}, {"slots": 0}, {"slots": 1}):
        rc, err = _refused(dev, 0, 4, **kw)
        assert rc == INVALID and (err == FILL).all()
    rc, err = _refused(dev, 0, 9)  # n > slots / 2
    assert rc == INVALID and (err == FILL).all()
    rc, err = _refused(dev, 5, 4)  # n_done > n
    assert rc == INVALID and (err == FILL).all()
    L, h = dev.L, dev.ctx.h
    assert L.nkv_memtable_add_dev(h, None, dev.nbytes, dev.p_off, 0, 4, dev.p_index, 16, 0, 0, 0, dev.p_state, None,
                                  None) == INVALID
    assert L.nkv_memtable_add_dev(h, dev.p_log, dev.nbytes, dev.p_off, 0, 4, None, 16, 0, 0, 0, dev.p_state, None,
                                  None) == INVALID
    assert L.nkv_memtable_add_dev(h, dev.p_log, dev.nbytes, dev.p_off, 0, 4, dev.p_index, 16, 0, 0, 0, None, None,
                                  None) == INVALID
    assert L.nkv_memtable_clear_dev(h, dev.p_index, 12, dev.p_state) == INVALID
    assert L.nkv_memtable_find_dev(h, dev.p_log, dev.nbytes, dev.p_off, 0, dev.p_index, 12, None, None, None, 0, 0, 0,
                                   None, None, None) == INVALID
    assert L.nkv_memtable_find_dev(h, dev.p_log, dev.nbytes, dev.p_off, 0, dev.p_index, 16, None, None, None, 0, 32,
                                   0, None, None, None) == INVALID
    dev.ctx.sync()
    assert (dev.index_check() == 0xFF).all() and dev.state() == [0, 0, 0, NONE]
    check_add(dev, log, 0, 8, (0, 0, 0))  # n = slots / 2 is taken


def test_find_flags_a_record_outside_the_log(nkv):
    """A log_len cut short behind the add: the probe of the record that now
    reaches outside counts as no match, d_err says so, nothing past it is read."""
    log = [rec(b"first", b"v"), rec(b"last-key", b"")]
    dev = Dev.of(nkv, log)
    check_add(dev, log, 0, 2, (0, 0, 0))
    dev.nbytes -= 3  # the last record's key no longer fits
    hit, status, err = dev.find([b"first", b"last-key"])
    assert err == 1 and hit.tolist() == [0, NONE] and status.tolist() == [ref.LIVE, ref.ABSENT]


# ---------------------------------------------------------------------------
# the buffer contract at other alignments (every test above uses the minimum)

@pytest.mark.parametrize("index_at,state_at,new_at,err_at", [(8, 8, 0, 4), (24, 40, 3, 12), (8 * 5, 8 * 3, 7, 4 * 5)])
def test_outputs_at_odd_multiples_of_their_alignment(nkv, index_at, state_at, new_at, err_at):
    rng = np.random.default_rng(0x6275)
    pool = distinct_keys(rng, 90)
    log = log_from(rng, [pool[j] for j in rng.integers(0, 90, 300)])
    dev = Dev.of(nkv, log, index_at=index_at, state_at=state_at)
    trace = check_add(dev, log, 0, 130, (BOTH, 50, 5000), new_at=new_at, err_at=err_at)
    check_add(dev, log, 130, 300, (BOTH, 50, 5000), trace, new_at=new_at, err_at=err_at)
    rc, is_new, state, err = dev.add(300, 300, with_new=False)  # no d_is_new, no write
    assert rc == 0 and state == trace.state(300, 300)
    check_find(dev, log, pool + absent_keys(rng, log, 10), hit_at=8 * 3, status_at=5)


# ---------------------------------------------------------------------------
# end to end: memtable.Memtable and lsmtree.get_many(memtable=)

def _puts(rng, n, pool):
    keys = [pool[j] for j in rng.integers(0, len(pool), n)]
    return keys, [rng.bytes(int(v)) for v in rng.integers(0, 120, n)], rng.integers(1, 1000, n).astype(np.int64), \
        (rng.random(n) < 0.15).astype(np.uint8)


def test_memtable_flush_equals_flush_puts(nkv):
    from nakevaleng_amd import lsmtree, memtable
    rng = np.random.default_rng(0x653265)
    keys, values, ts, status = _puts(rng, 700, distinct_keys(rng, 200, 0, 30))
    records = [rec(k, v, status=int(s), ts=int(t)) for k, v, t, s in zip(keys, values, ts, status)]
    rule = (BOTH, 150, 20000)
    trace = ref.add_closed(records, *rule)
    mt = memtable.Memtable(1000, 1 << 17, *rule)
    assert mt.slots == 2048 and mt.count() == (0, 0) and not mt.should_flush()
    for lo, hi in ((0, 1), (1, 300), (300, 700)):
        is_new, flush_at = mt.put_many(keys[lo:hi], values[lo:hi], ts[lo:hi], status[lo:hi])
        assert is_new.tolist() == trace.is_new[lo:hi]
        assert flush_at == (None if trace.flush_at(lo, hi) == NONE else trace.flush_at(lo, hi))
        assert mt.count() == (trace.count[hi - 1], trace.memusage[hi - 1])
        assert mt.should_flush() == trace.should_flush[hi - 1]
    found = mt.find_many(keys[:50] + [b"no such key"])
    want = ref.find_literal(records, keys[:50] + [b"no such key"])
    assert found == want and found[-1] is None
    with pytest.raises(ValueError):
        mt.put_many([b"k"] * 301, [b""] * 301)
    kw = dict(seed=7, summary_page_size=3)
    got = mt.flush(**kw)
    want = lsmtree.flush_puts(keys, values, ts, status, **kw)
    assert got["table"][0] == want["table"][0] and np.array_equal(got["table"][1], want["table"][1])
    for what in ("root", "image", "index", "summary"):
        assert got[what] == want[what], what
    assert bytes(got["filter"].Contents) == bytes(want["filter"].Contents)
    assert np.array_equal(got["sources"], want["sources"])
    assert mt.count() == (0, 0) and mt.n == 0 and mt.find_many([keys[0]]) == [None]
    # add_log: the same log as WAL replay would hand it over
    is_new, flush_at = mt.add_log(want["log"])
    assert is_new.tolist() == trace.is_new
    assert flush_at == (None if trace.flush_at() == NONE else trace.flush_at())
    assert mt.find_many(keys[:50]) == ref.find_literal(records, keys[:50])


def test_get_many_asks_the_memtable_first(nkv):
    from nakevaleng_amd import lsmtree, memtable
    from tests import lookup_ref
    from tests.memtable_ref import flush_closed
    rng = np.random.default_rng(0x676574)
    pool = distinct_keys(rng, 120, 1, 24)
    disk_logs = [log_from(rng, [pool[j] for j in rng.integers(0, 80, 60)], vmax=50),
                 log_from(rng, [pool[j] for j in rng.integers(20, 100, 60)], vmax=50)]
    disk = [record.data_table(flush_closed(log)[0]) for log in disk_logs]
    model_tables = [lookup_ref.table_of(stream, sizes, 3) for stream, sizes in disk]
    resident = [lsmtree.upload_table(t) for t in disk]
    on_disk = {r.Key: r for log in reversed(disk_logs) for r in flush_closed(log)[0]}  # table 0 answers first
    live_on_disk = [k for k, r in on_disk.items() if not r.IsDeleted()]
    only_mem = pool[100:110]
    both, dead = live_on_disk[:10], live_on_disk[10:20]  # the memtable wins; tombstoned in the memtable
    mem_keys = only_mem + both + dead + both[:3]
    mem_vals = [rng.bytes(int(v)) for v in rng.integers(0, 50, len(mem_keys))]
    mem_status = np.asarray([0] * 20 + [1] * 10 + [0] * 3, np.uint8)
    mt = memtable.Memtable(64, 1 << 14, 0)
    mt.put_many(mem_keys, mem_vals, 5, mem_status)
    mem_records = [rec(k, v, status=int(s), ts=5) for k, v, s in zip(mem_keys, mem_vals, mem_status)]
    only_disk = [k for k in live_on_disk[20:40]]
    queries = only_mem + only_disk + both + dead + pool[110:] + [b"", only_mem[0]]
    want = [ref.get_model(mem_records, model_tables, k) for k in queries]
    got, stages, hits = lsmtree.get_many(resident, queries, stages=True, memtable=mt)
    assert got == [v for _, v in want]
    assert stages.shape == (len(queries), 2)
    for k, g, h in zip(queries, got, hits):
        if k in only_mem or k in both:
            assert g is not None and int(h) >> 32 == 2  # the log is listed behind the two tables
        if k in dead:
            assert g is None and int(h) >> 32 == 2  # not found, though table 0 or 1 holds it live
        if k in only_disk:
            assert g == on_disk[k].Value and int(h) >> 32 < 2
    assert lsmtree.get_many(resident, queries) == [lookup_ref.get(model_tables, k).value
                                                   if lookup_ref.get(model_tables, k).status == ref.LIVE else None
                                                   for k in queries]  # without a memtable nothing changes
    # no table at all: the memtable alone; and an empty memtable beside the tables
    assert lsmtree.get_many([], queries, memtable=mt) == [v for _, v in (ref.get_model(mem_records, [], k)
                                                                         for k in queries)]
    mt.clear()
    assert lsmtree.get_many(resident, queries, memtable=mt) == lsmtree.get_many(resident, queries)
    assert lsmtree.get_many([], queries[:3], memtable=mt) == [None] * 3
