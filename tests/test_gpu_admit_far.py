"""GPU: nkv_admit_dev over requests whose users, keys and stored buckets lie
more than 4 GiB apart inside one allocation.

The three kinds of item of request i -- its user, its key, its stored image --
are dealt to the three islands of tests/far.py in rotation (kind k of request i
goes to island (i + k) % 3), so the users of any 64 consecutive requests, their
keys and their images each span more than 4 GiB, and a user compared in place
with the first request of its group usually sits in another island.  users,
keys and buckets are one blob of far.ALLOC bytes; every address the kernels form
needs the full 64-bit offset.  Only the islands are uploaded; an address built
from a wrapped 32-bit offset would still land inside the allocation and read
wrong bytes, never unmapped memory.

Each case is held to tests/admit_ref.py and to its near twin: the same items at
their compact offsets in a small tensor."""
import numpy as np
import pytest

from tests import admit_ref as ref
from tests import far
from tests.test_gpu_admit import (LIVE, START, _dev, _torch, expect, keys_of, run, stored_dict, stored_of, times_of,
                                  users_of)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def big():
    """The one big allocation.  Never filled as a whole; a failed allocation fails the tests."""
    torch = _torch()
    buf = torch.empty(far.ALLOC, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 256 == 0
    yield buf
    del buf
    torch.cuda.empty_cache()


def layout(requests, stored):
    """(compact bytes, islands, {kind: compact offsets per request}, lengths)."""
    items, slot = [], {}
    for i, ((user, key, _), (_, img)) in enumerate(zip(requests, stored)):
        triple = (user, key, img or b"")
        for kind in sorted(range(3), key=lambda k: (k + i) % 3):  # position p in the triple = island p
            slot[(i, kind)] = len(items)
            items.append(triple[kind])
    lens = np.asarray([len(x) for x in items], np.uint64)
    off, ranges = far.deal(lens, (np.arange(len(items)) * 13 + 5) % 64, 3, 64)
    compact = np.full(ranges[-1][1], 0xEE, np.uint8)
    for x, o in zip(items, off):
        compact[int(o):int(o) + len(x)] = np.frombuffer(x, np.uint8)
    islands = [(s, e, far.BASES[k]) for k, (s, e) in enumerate(ranges)]
    idx = {kind: np.asarray([slot[(i, kind)] for i in range(len(requests))]) for kind in range(3)}
    return compact, islands, idx, off, lens


@pytest.mark.parametrize("n", [65, 1025])
def test_users_keys_and_buckets_4_gib_apart(nkv, big, n):
    torch = _torch()
    rng = np.random.default_rng(0x61646D60 + n)
    Max, R = 3, 2
    requests = list(zip(users_of("hot", n, rng), keys_of(n, rng), times_of(n, rng, R)))
    stored = stored_of(requests, rng)
    compact, islands, idx, off, lens = layout(requests, stored)
    dev_off, uploads = far.place(off, lens, islands)
    assert max(e for _, e, _ in islands) < (1 << 24) and far.BASES[2] + (1 << 24) <= far.ALLOC
    for db, sl in uploads:
        big[db:db + sl.stop - sl.start].copy_(torch.from_numpy(compact[sl].copy()))
    live = np.asarray([s == LIVE for s, _ in stored])
    # every 64 consecutive requests' users span more than 4 GiB, and so do their keys
    for kind in (0, 1):
        o = dev_off[idx[kind]].astype(np.int64)
        assert all(o[a:a + 64].max() - o[a:a + 64].min() > far.G32 for a in range(0, n - 63, 64))

    def pointers(base, offs, total, keep):
        arrays = [_dev(offs[idx[kind]]) for kind in (0, 1)]
        boff = np.where(live, offs[idx[2]], np.uint64(1 << 62)).astype(np.uint64)
        arrays.append(_dev(boff))
        keep.extend(arrays)

        def hook(f):
            f.update(users=base, users_len=total, uoff=arrays[0].data_ptr(), keys=base, keys_len=total,
                     koff=arrays[1].data_ptr(), buckets=base, boff=arrays[2].data_ptr())
        return hook

    keep = []
    want = ref.admit_literal(requests, START, Max, R, stored_dict(requests, stored))
    rc, err, got = run(nkv, requests, START, Max, R, stored,
                       override=pointers(big.data_ptr(), dev_off, far.ALLOC, keep))
    assert (rc, err) == (0, 0)
    expect(got, want, n)
    for db, sl in uploads:  # the islands are unchanged
        assert np.array_equal(big[db:db + sl.stop - sl.start].cpu().numpy(), compact[sl])

    d_compact = _dev(compact)
    rc, err, near = run(nkv, requests, START, Max, R, stored,
                        override=pointers(d_compact.data_ptr(), off, compact.size, keep))
    assert (rc, err) == (0, 0)
    assert all(np.array_equal(near[k], got[k]) for k in got)
