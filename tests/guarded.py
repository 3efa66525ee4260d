"""Output buffers with guards, and input snapshots, for the device-pointer API.

guarded(nbytes, offset) carves a payload out of the middle of one larger
allocation:

    [ 256 guard | offset guard | nbytes payload | >= 256 guard ]

Every guard byte holds `fill`.  The guards lie inside the allocation, so a
kernel that writes a few bytes before or past its documented output changes a
guard byte (and check() fails) without ever leaving the allocation.  torch's
allocations start at 256-byte multiples or better, so `offset` is the
payload's address modulo 256: it places an output at its minimum alignment.

The upload of a device buffer is followed by a device-wide synchronize, so an
entry may write it from any stream right away.

frozen(tensor) snapshots an input; the returned function asserts later that
the tensor still holds the same bytes.
"""
import numpy as np

GUARD = 256


def _bytes_of(t):
    return t.detach().cpu().contiguous().view(-1).numpy().view(np.uint8).copy()


def guarded(nbytes, offset, fill=0xA5, device="cuda", init=None):
    """(payload address, check).  check() asserts that every guard byte still
    equals `fill` and returns the payload's bytes (a numpy copy).  `init`
    (bytes-like of nbytes, optional) is what the payload holds at first, else
    `fill` as well."""
    import torch
    nbytes, offset = int(nbytes), int(offset)
    assert nbytes >= 0 and offset >= 0
    lo = GUARD + offset
    hi = lo + nbytes
    size = (hi + GUARD + 15) & ~15
    host = np.full(size, fill, np.uint8)
    if init is not None:
        src = np.frombuffer(bytes(init), np.uint8) if not isinstance(init, np.ndarray) else init.reshape(-1).view(np.uint8)
        assert src.size == nbytes
        host[lo:hi] = src
    buf = torch.from_numpy(host).to(device)
    if device != "cpu":
        torch.cuda.synchronize()  # the caller's entry runs on another stream than this upload
    assert buf.data_ptr() % GUARD == 0 or device == "cpu"

    def check():
        got = _bytes_of(buf)
        before = np.flatnonzero(got[:lo] != fill)
        after = np.flatnonzero(got[hi:] != fill)
        assert before.size == 0, f"{before.size} guard bytes changed before the payload, nearest {lo - int(before[-1])} B in front"
        assert after.size == 0, f"{after.size} guard bytes changed past the payload, first {int(after[0])} B past its end"
        return got[lo:hi]

    check.buffer = buf  # keeps the allocation alive as long as check is held
    return buf.data_ptr() + lo, check


def frozen(tensor):
    """Snapshot `tensor` now; the returned function asserts it is byte-identical."""
    snap = _bytes_of(tensor)

    def intact():
        now = _bytes_of(tensor)
        diff = np.flatnonzero(now != snap)
        assert diff.size == 0, f"input modified: {diff.size} bytes differ, first at byte {int(diff[0])}"

    return intact
