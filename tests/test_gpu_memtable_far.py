"""GPU: the live memtable over a log whose records lie more than 4 GiB apart.

The add requires a dense log, so the distance comes from one record whose Value
is far.GIANT_VALUE (2^32 + 5) bytes long, as in the merge's giant case
(tests/far.py): the records behind it start past 2^32, and every address the
kernels form -- a record's header, a key compared in place, a Status -- needs
the full 64-bit offset.  The one allocation of far.ALLOC bytes is never filled
as a whole: only the bytes in front of the giant Value and those behind it are
uploaded, and no kernel of the memtable reads a Value.  The log lies inside
that allocation from its first byte on, so an address built from a wrapped
32-bit offset would read wrong bytes inside it, never unmapped memory.

Each case is held to tests/live_memtable_ref.py (memusage includes the giant
TotalSize) and to its near twin: the same writes with a 5-byte Value in an
ordinary small tensor, whose Add and Find answers must be the same.
"""
import numpy as np
import pytest

from nakevaleng_amd.record import Record
from tests import far
from tests import live_memtable_ref as ref
from tests.test_gpu_memtable import Dev, _dev, _torch
from tests.test_live_memtable_ref import BOTH, rec

pytestmark = pytest.mark.gpu

RULE = (BOTH, 9, 1 << 33)  # the capacity fires; the threshold lies above even the giant record


@pytest.fixture(scope="module")
def big():
    """The one big allocation.  Never filled as a whole; a failed allocation fails the tests."""
    torch = _torch()
    buf = torch.empty(far.ALLOC, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    yield buf
    del buf
    torch.cuda.empty_cache()


def giant(key, status=0, value_size=far.GIANT_VALUE):
    """A record whose Value is not materialised: ToBytes() is its header and key."""
    return Record(0, 7, status, 0, len(key), value_size, key, b"")


def small(rng, keys):
    return [rec(k, rng.bytes(int(v)), status=int(t)) for k, v, t in
            zip(keys, rng.integers(0, 60, len(keys)), rng.random(len(keys)) < 0.2)]


def _cases():
    rng = np.random.default_rng(0x66617236)
    pool = [rng.bytes(int(n)) for n in (0, 1, 7, 8, 9, 16, 17, 40, 33, 12, 5, 24)]
    before = small(rng, pool[:6])
    after = small(rng, pool[3:] + [b"giant-key"] + pool[:4])
    return {
        # records on both sides of the giant one; its key is overwritten 4 GiB further on
        "giant-in-the-middle": (before, giant(b"giant-key"), after, 0),
        # the giant record first, a tombstone, and the log 3 bytes past a 256-byte boundary
        "giant-first": ([], giant(pool[4], status=1), small(rng, pool + pool[2:6]), 3),
    }


@pytest.mark.parametrize("name", sorted(_cases()))
def test_records_4_gib_apart(nkv, big, name):
    torch = _torch()
    before, g, after, log_at = _cases()[name]
    records = before + [g] + after
    head = b"".join(r.ToBytes() for r in before + [g])
    tail = b"".join(r.ToBytes() for r in after)
    sizes = np.asarray([r.TotalSize() for r in records], np.uint64)
    off = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.uint64)
    nbytes = int(sizes.sum())
    base, tail_at = 256 + log_at, 256 + log_at + len(head) + far.GIANT_VALUE
    assert int(off[len(before) + 1]) > far.G32 and tail_at + len(tail) == base + nbytes <= far.ALLOC
    big[base:base + len(head)].copy_(torch.from_numpy(np.frombuffer(head, np.uint8).copy()))
    big[tail_at:tail_at + len(tail)].copy_(torch.from_numpy(np.frombuffer(tail, np.uint8).copy()))
    d_off = _dev(off)
    torch.cuda.synchronize()

    def unchanged():
        assert big[base:base + len(head)].cpu().numpy().tobytes() == head
        assert big[tail_at:tail_at + len(tail)].cpu().numpy().tobytes() == tail

    n = len(records)
    queries = sorted({r.Key for r in records}) + [b"giant-ke", b"giant-key\0", b"absent"]
    trace = ref.add_closed(records, *RULE)
    want = ref.find_closed(records, queries, 31)
    assert trace.memusage[-1] > far.G32

    dev = Dev(nkv, big.data_ptr() + base, d_off.data_ptr(), off, nbytes, 64, keep=(d_off,), intact=(unchanged,))
    rc, is_new, state, err = dev.add(0, n, RULE)
    assert rc == 0 and int(err.view(np.uint32)[0]) == 0
    assert is_new.tolist() == [int(x) for x in trace.is_new] and state == trace.state(0, n)
    hit, status, err = dev.find(queries, table_id=31)
    assert err == 0 and (hit.tolist(), status.tolist()) == want

    # the near twin: the same writes, the giant Value 5 bytes long
    twin = before + [rec(g.Key, bytes(5), status=g.Status)] + after
    near = Dev.of(nkv, twin, slots=64, log_at=log_at)
    rc, near_new, near_state, err = near.add(0, n, RULE)
    assert rc == 0 and int(err.view(np.uint32)[0]) == 0
    assert near_new.tolist() == is_new.tolist()
    assert near_state[0] == state[0] and near_state[2:] == state[2:]
    assert near_state[1] + far.GIANT_VALUE - 5 == state[1]
    near_hit, near_status, err = near.find(queries, table_id=31)
    assert err == 0 and near_hit.tolist() == hit.tolist() and near_status.tolist() == status.tolist()
