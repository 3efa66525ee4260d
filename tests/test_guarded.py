"""CPU: tests/guarded.py bites.  Fake "entries" (plain numpy writes through the
payload's address) that write one byte before the payload, one byte past it,
or exactly the payload: the first two must fail check(), the third must pass
and return what was written.  The same for frozen()."""
import ctypes

import numpy as np
import pytest

from tests.guarded import GUARD, frozen, guarded


def _window(ptr, before, nbytes):
    """numpy view of the nbytes bytes that start `before` bytes in front of ptr."""
    return np.frombuffer((ctypes.c_uint8 * nbytes).from_address(ptr - before), np.uint8)


SHAPES = [(1, 0), (20, 4), (64, 13), (4099, 7), (0, 1)]


@pytest.mark.parametrize("nbytes,offset", SHAPES)
def test_exact_write_passes(nbytes, offset):
    ptr, check = guarded(nbytes, offset, device="cpu")
    want = (np.arange(nbytes) * 7 + 3).astype(np.uint8)
    _window(ptr, 0, max(nbytes, 1))[:nbytes] = want
    assert np.array_equal(check(), want)


@pytest.mark.parametrize("nbytes,offset", SHAPES)
def test_one_byte_before_fails(nbytes, offset):
    ptr, check = guarded(nbytes, offset, device="cpu")
    _window(ptr, 1, nbytes + 1)[:] = 0x11
    with pytest.raises(AssertionError, match="before the payload, nearest 1 B"):
        check()


@pytest.mark.parametrize("nbytes,offset", SHAPES)
def test_one_byte_past_fails(nbytes, offset):
    ptr, check = guarded(nbytes, offset, device="cpu")
    _window(ptr, 0, nbytes + 1)[:] = 0x11
    with pytest.raises(AssertionError, match="past the payload, first 0 B"):
        check()


def test_far_edges_of_the_guards_are_watched():
    """The first byte of the leading guard and the last of the trailing one."""
    for at in (-(GUARD + 5), 40 + GUARD - 1):
        ptr, check = guarded(40, 5, device="cpu")
        _window(ptr + at, 0, 1)[0] = 0
        with pytest.raises(AssertionError):
            check()
        ptr, check = guarded(40, 5, device="cpu")
        check()


def test_a_write_of_the_fill_value_is_the_only_blind_spot():
    """A stray write is seen unless it stores the fill byte itself, so callers
    that can produce 0xA5 pick another fill."""
    ptr, check = guarded(8, 0, fill=0x3C, device="cpu")
    _window(ptr, 1, 1)[0] = 0xA5
    with pytest.raises(AssertionError):
        check()


def test_init_is_the_payload_and_guards_stay():
    init = np.arange(24, dtype=np.uint8)
    ptr, check = guarded(24, 12, device="cpu", init=init)
    assert np.array_equal(_window(ptr, 0, 24), init)
    assert (_window(ptr, 12 + GUARD, 12 + GUARD) == 0xA5).all()
    assert np.array_equal(check(), init)


def test_frozen():
    import torch
    t = torch.arange(100, dtype=torch.int64)
    intact = frozen(t)
    intact()
    t[99] += 1 << 56  # the very last byte
    with pytest.raises(AssertionError, match="first at byte 799"):
        intact()
    t = torch.zeros(5, dtype=torch.uint8)
    intact = frozen(t)
    t[0] = 1
    with pytest.raises(AssertionError, match="first at byte 0"):
        intact()
