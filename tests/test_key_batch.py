"""The query batch of the get paths (nakevaleng_amd/_dev.py pack_keys): what
get_many, locate_many and Memtable.find_many upload as keys / koff / klen.
Pure numpy, no GPU."""
import numpy as np

from nakevaleng_amd._dev import pack_keys


def _check(keys):
    want = [bytes(k) for k in keys]
    blob, koff, klen = pack_keys(keys)
    assert isinstance(blob, bytes)
    assert koff.dtype == np.uint64 and klen.dtype == np.uint64
    assert koff.shape == klen.shape == (len(want),)
    assert klen.tolist() == [len(k) for k in want]
    assert koff.tolist() == [sum(len(k) for k in want[:i]) for i in range(len(want))]
    assert blob == (b"".join(want) or b"\0")
    for i, k in enumerate(want):  # every key is where its offset and length say
        assert blob[int(koff[i]):int(koff[i]) + int(klen[i])] == k
    return blob, koff, klen


def test_one_empty_key():
    blob, koff, klen = _check([b""])
    assert blob == b"\0" and koff.tolist() == [0] and klen.tolist() == [0]


def test_empty_keys_around_one_byte():
    blob, koff, klen = _check([b"", b"a", b""])
    assert blob == b"a" and koff.tolist() == [0, 0, 1] and klen.tolist() == [0, 1, 0]


def test_bytearray_and_memoryview_keys():
    blob, _, klen = _check([bytearray(b"key-1"), memoryview(b"k2"), b"", memoryview(bytearray(b"\x00\xff"))])
    assert blob == b"key-1k2\x00\xff" and klen.tolist() == [5, 2, 0, 2]


def test_65_keys_of_mixed_lengths():
    rng = np.random.default_rng(65)
    lens = [0, 1, 7, 8, 9, 17, 300]
    keys = [rng.integers(0, 256, lens[i % len(lens)], dtype=np.uint8).tobytes() for i in range(65)]
    _, koff, klen = _check(keys)
    assert int(koff[-1] + klen[-1]) == sum(len(k) for k in keys)


def test_no_keys():
    blob, koff, klen = pack_keys([])
    assert blob == b"\0" and koff.size == 0 and klen.size == 0
