"""CPU: the far layouts of tests/far.py are what tests/test_gpu_far.py takes
them for -- far where they say far, on the intended side of the intended guard
where they say threshold, inside the allocation, and free of overlaps.  The
guards are evaluated here as csrc/sha1_feed_dev.hpp writes them, over the placed
addresses, independently of the flip distances far.py derives."""
import numpy as np
import pytest

from tests import far

M32 = 0xFFFFFFFF


def _groups(n):
    return [slice(g, min(g + 64, n)) for g in range(0, n, 64)]


def _check_ranges(ranges, limit=far.ALLOC):
    """Inside [0, limit) and pairwise disjoint (empty ranges never overlap)."""
    r = sorted((int(a), int(b)) for a, b in ranges if b > a)
    assert r[0][0] >= 0 and max(b for _, b in r) <= limit
    for (_, e0), (s1, _) in zip(r, r[1:]):
        assert e0 <= s1


def _check_allocation_rule(addr, lens):
    """far.py's allocation rule: a wave that spans 4 GiB has its lowest address
    at least 2^32 + the longest value before the allocation's end, whichever
    64 values the library groups (the lowest address of such a wave is below
    the highest address minus 2^32)."""
    addr = np.asarray(addr, np.int64)
    lowest_of_a_far_wave = int(addr.max()) - far.G32  # an upper bound
    if lowest_of_a_far_wave >= int(addr.min()):
        assert lowest_of_a_far_wave + far.G32 + int(np.max(lens)) + 64 <= far.ALLOC
    assert int((addr + np.asarray(lens, np.int64)).max()) <= far.ALLOC


def _pair_guard(addr, nmax):  # rel + 64ull * (uint64_t(nmax) + 1ull) <= 0xFFFFFFFFull, rel over p & ~63
    a = np.asarray(addr, np.int64) & ~63
    return bool(np.all((a - a.min()) + 64 * (nmax + 1) <= M32))


def _shift_guard(addr, nmax):  # the same over sa = p - o, o = p & 63 shared by the wave
    o = np.asarray(addr, np.int64) & 63
    assert (o == o[0]).all() and o[0] != 0
    return _pair_guard(addr, nmax)


def _ring_vc_guard(addr, nfull):  # relk[k] + lastk[k] + 16ull <= 0xFFFFFFFFull, every role
    addr, nfull = np.asarray(addr, np.int64), np.asarray(nfull, np.int64)
    has = nfull > 0
    wb = addr[has].min()
    wb_nfull = nfull[has & (addr == wb)].max()
    ok = True
    for dq in range(4):
        relk = np.where(has, addr - wb, 0) + 16 * dq
        lastk = 64 * (np.where(has, nfull, wb_nfull) - 1)
        ok &= bool(np.all(relk + lastk + 16 <= M32))
    return ok


@pytest.mark.parametrize("case", far.value_cases(), ids=lambda c: c.name)
def test_value_layouts(case):
    addr, uploads = case.placed()
    addr, lens = addr.astype(np.int64), case.lens.astype(np.int64)
    _check_ranges(list(zip(addr, addr + lens)))
    _check_ranges([(b, b + s.stop - s.start) for b, s in uploads])
    _check_allocation_rule(addr, lens)
    # the islands keep every value's offset modulo 64, so the near twin takes the same stage
    assert np.array_equal(addr % 64, case.off.astype(np.int64) % 64)
    if case.far:
        for g in _groups(case.n):
            if g.stop - g.start >= 2:
                assert addr[g].max() - addr[g].min() > far.G32
    if case.guard:
        head = slice(0, case.nfull_head or case.n)
        nfull = lens[head] // 64
        if case.guard == "ring_vc":
            held = _ring_vc_guard(addr[head], nfull)
        else:
            assert (nfull == nfull[0]).all()
            held = (_pair_guard if case.guard == "pair" else _shift_guard)(addr[head], int(nfull[0]))
        assert held == case.near_side
    if case.nfull_head:
        # the sort is by compression count, longest first: the head is the queue's first group
        comp = (lens + 8) // 64 + 1
        assert case.nfull_head <= 64 and comp[:case.nfull_head].min() > comp[case.nfull_head:].max()


def test_value_cases_cover_both_sides_of_every_guard():
    sides = {(c.guard, c.near_side) for c in far.value_cases() if c.guard}
    assert sides == {(g, s) for g in ("pair", "shift", "ring_vc") for s in (True, False)}
    names = [c.name for c in far.value_cases()]
    assert len(set(names)) == len(names)


def test_flip_distances_are_adjacent():
    for nmax in (1, 2, 3, 200, 1 << 20):
        near, first_far = far.pair_flip(nmax)
        assert first_far - near == 64 and near % 64 == 0
        assert _pair_guard([0, near], nmax) and not _pair_guard([0, first_far], nmax)
        assert far.shift_flip(nmax) == (near, first_far)
        near, first_far = far.ring_vc_flip(nmax)
        assert first_far == near + 1
        assert _ring_vc_guard([0, near], [nmax, nmax]) and not _ring_vc_guard([0, first_far], [nmax, nmax])


def test_the_near_wrap_case_wraps_in_32_bits():
    """ring_vc-near-wrap: the wave is near, and the far value's rel + 64 c
    leaves 32 bits at the first block past the shortest value."""
    case = next(c for c in far.value_cases() if c.name == "ring_vc-near-wrap")
    addr, _ = case.placed()
    rel = int(addr[1]) - int(addr[0])
    assert int(addr[0]) == int(addr[:3].min()) and rel + 48 + 16 == M32  # the last 16-byte request still fits
    assert rel + 48 + 64 > M32  # the same role one block on: past 32 bits
    assert int(case.lens[2]) // 64 == 200 and int(addr[0]) < int(addr[2]) < int(addr[1])


@pytest.mark.parametrize("case", far.strided_cases(), ids=lambda c: c.name)
def test_strided_layouts(case):
    addr = case.base + case.stride * np.arange(case.n, dtype=np.int64)
    assert case.stride >= case.L
    _check_allocation_rule(addr, np.full(case.n, case.L, np.int64))
    if case.far:
        full = [g for g in _groups(case.n) if g.stop - g.start == 64] or [slice(0, case.n)]
        for g in full:
            assert addr[g].max() - addr[g].min() > far.G32
    assert case.near_stride() % 64 == case.stride % 64 and case.near_stride() >= case.L


def test_strided_threshold_figures():
    t = far.strided_flip()
    span = 63 * t["stride"]
    addr = 64 + t["stride"] * np.arange(64, dtype=np.int64)
    assert t["stride"] % 64 == 0
    assert _pair_guard(addr, t["last_near_len"] // 64) and not _pair_guard(addr, t["first_far_len"] // 64)
    assert t["first_far_len"] == t["last_near_len"] + 1
    # the highest 32-bit offset the strided fallthrough would form: role q = 3 of value 63, last block
    top = lambda L: span + 48 + 64 * (L // 64 - 1)
    assert top(t["first_far_len"]) <= M32 < top(t["wrap_len"]) and top(t["wrap_len"] - 64) <= M32
    lens = {c.L for c in far.strided_cases() if c.name.startswith("threshold")}
    assert lens == {t["last_near_len"], t["first_far_len"], t["wrap_len"]}


@pytest.mark.parametrize("case", far.record_cases(), ids=lambda c: c.name)
def test_record_layouts(case):
    lay = case.layout
    addr, uploads = lay.placed()
    addr, size = addr.astype(np.int64), lay.lens.astype(np.int64)
    assert np.array_equal(size, 30 + case.ks.astype(np.int64) + case.vs.astype(np.int64))
    _check_ranges(list(zip(addr, addr + size)))
    _check_ranges([(b, b + s.stop - s.start) for b, s in uploads])
    _check_allocation_rule(addr, size)
    voff = addr + 30 + case.ks.astype(np.int64)
    for g in _groups(case.n):
        assert voff[g].max() - voff[g].min() > far.G32
    assert (addr[np.arange(case.n) % 3 != 0] >= far.G32).all()


def test_giant_table_ranges():
    _check_ranges(far.giant_ranges())
    assert far.GIANT_VALUE > far.G32
