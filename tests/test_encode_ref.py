"""tests/encode_ref.py, the record encoder's reference, against a pinned vector
and against nakevaleng_amd/record.py's New / ToBytes.  No device is needed."""
import numpy as np

from nakevaleng_amd import record
from tests.encode_ref import encode_many_ref, encode_ref


def test_pinned_vector():
    """CRC-32/IEEE of "123456789" is the standard check value 0xCBF43926."""
    want = bytes.fromhex("2639f4cb" "0807060504030201" "01" "07" "0400000000000000" "0500000000000000") + b"123456789"
    assert encode_ref(b"1234", b"56789", 0x0102030405060708, 1, 7) == want
    assert len(want) == 30 + 9


def test_agrees_with_record_py_on_a_ragged_batch():
    rng = np.random.default_rng(0x656E)
    keys = [rng.bytes(int(k)) for k in rng.integers(0, 34, 200)]
    vals = [rng.bytes(int(v)) for v in rng.integers(0, 300, 200)]
    ts = rng.integers(-2**63, 2**63 - 1, 200, dtype=np.int64)
    recs = [record.New(k, v, int(t)) for k, v, t in zip(keys, vals, ts)]
    stream, sizes = record.data_table(recs)
    got, off, crc = encode_many_ref(keys, vals, ts)
    assert got == stream
    assert np.array_equal(np.diff(np.append(off, np.uint64(len(got)))), sizes)
    assert crc.tolist() == [r.Crc for r in recs]
    # Status and TypeInfo, which record.New leaves 0
    r = record.New(b"k", b"v", 5)
    r.Status, r.TypeInfo = 1, 0xFF
    assert encode_ref(b"k", b"v", 5, 1, 0xFF) == r.ToBytes()


def test_the_empty_record():
    got = encode_ref(b"", b"", 0)
    assert got == bytes(30)
    assert record.New(b"", b"", 0).ToBytes() == got


def test_pack_puts_checks_lengths():
    import pytest
    with pytest.raises(ValueError):
        record.pack_puts([b"a"], [b"x", b"y"])
    with pytest.raises(ValueError):
        record.pack_puts([b"a", b"b"], [b"x", b"y"], timestamps=[1])
    with pytest.raises(ValueError):
        record.pack_puts([b"a", b"b"], [b"x", b"y"], status=[1, 2, 3])
    p = record.pack_puts([b"ab", b"", b"c"], [b"", b"xyz", b"w"], timestamps=7, status=1)
    assert p["koff"].tolist() == [0, 2, 2] and p["voff"].tolist() == [0, 0, 3]
    assert p["ts"] is None and p["ts_all"] == 7 and p["status"].tolist() == [1, 1, 1] and p["type"] is None
