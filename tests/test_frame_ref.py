"""CPU: the two host statements of the framing rule (tests/frame_ref.py) held to
each other -- the literal Deserialize loop over a byte reader and the closed
form the header states -- on hand cases and on the last record cut at every
byte.  The hand cases are the GPU tests' too (tests/test_gpu_frame.py)."""
import struct

import numpy as np
import pytest

from nakevaleng_amd import record
from tests.frame_ref import NONE, deserialize_loop, frame_closed, sizes_of


def rec(key, val, ts=7):
    return record.New(key, val, timestamp=ts).ToBytes()


def raw(ks, vs, body=b""):
    """A header that claims ks / vs whatever follows it."""
    return struct.pack("<IqBBQQ", 0, 0, 0, 0, ks, vs) + body


def table(n, rng, kmax=12, vmax=40):
    return [rec(rng.bytes(int(k)), rng.bytes(int(v)))
            for k, v in zip(rng.integers(0, kmax + 1, n), rng.integers(0, vmax + 1, n))]


def offsets_of(parts, base=0):
    out, p = [], base
    for b in parts:
        out.append(p)
        p += len(b)
    return out


def _hand_cases():
    rng = np.random.default_rng(0x6672)
    cases = {}
    t = table(7, rng)
    whole = b"".join(t)
    starts = offsets_of(t)
    cases["empty_stream"] = (b"", None)
    cases["one_byte"] = (b"\0", None)
    cases["29_bytes"] = (bytes(29), None)
    cases["30_zero_bytes"] = (bytes(30), None)  # one record with an empty key and an empty value
    cases["31_zero_bytes"] = (bytes(31), None)
    cases["empty_records"] = (rec(b"", b"") * 5 + rec(b"k", b"") + rec(b"", b"v"), None)
    cases["one_segment"] = (whole, None)
    cases["one_listed_segment"] = (whole, [0])
    cases["record_per_segment"] = (whole, starts)
    cases["bytes_before_first_segment"] = (b"\xff" * 11 + whole, [11])
    cases["empty_segments"] = (whole, [0, 0, starts[2], starts[2], starts[2], starts[5], len(whole), len(whole)])
    cases["only_empty_segments"] = (b"", [0, 0, 0])
    cases["short_segment"] = (whole[:starts[3]] + bytes(17) + whole[starts[3]:],
                              [0, starts[3], starts[3] + 17])
    # a record that fits the stream but crosses its segment's end is a tail
    cases["crosses_segment_end"] = (whole, [0, starts[4] + 33])
    # sizes that do not fit: Go's make would panic on the huge ones
    cases["huge_key_size"] = (t[0] + raw(2**63, 0) + t[1], None)
    cases["huge_value_size"] = (t[0] + raw(3, 2**64 - 1, b"abc") + t[1], None)
    cases["sizes_wrap_together"] = (t[0] + raw(2**63, 2**63, bytes(40)), None)
    cases["value_one_byte_short"] = (t[0] + raw(2, 5, b"kkvvvv"), None)
    # decoys: a value that holds a whole table; a value whose bytes frame a
    # wild record that ends exactly on a true record start, on a segment end
    # and on the stream's end
    cases["nested_table"] = (rec(b"outer", whole) + t[0] + rec(b"again", whole + whole), None)
    wild = raw(0, len(t[1]))  # the end of a value, read as a header: its record ends where t[1] does
    cases["wild_lands_on_record"] = (rec(b"a", b"\1" * 9 + wild) + t[1] + t[2], None)
    cases["wild_lands_on_segment_end"] = (rec(b"a", wild) + t[1] + t[2], [0, 31 + len(wild) + len(t[1])])
    cases["wild_lands_on_stream_end"] = (rec(b"a", wild) + t[1], None)
    return cases


HAND_CASES = _hand_cases()


def same(a, b):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert a[3] == b[3]


@pytest.mark.parametrize("name", sorted(HAND_CASES))
def test_hand_cases_agree(name):
    stream, seg = HAND_CASES[name]
    got = frame_closed(stream, seg)
    same(deserialize_loop(stream, seg), got)
    off, first, seg_len, stats = got
    S = 1 if seg is None else len(seg)
    assert first.size == S + 1 and seg_len.size == S and first[-1] == off.size == stats[0]
    assert stats[1] == int(seg_len.sum())
    assert int(sizes_of(stream, off).sum()) == stats[1]


def test_hand_cases_say_what_they_claim():
    n = lambda name: frame_closed(*HAND_CASES[name])[3]
    assert n("empty_stream") == [0, 0, 0, NONE]
    assert n("29_bytes") == [0, 0, 1, 0]
    assert n("30_zero_bytes") == [1, 30, 0, NONE]
    assert n("31_zero_bytes") == [1, 30, 1, 0]
    assert n("one_segment") == [7, len(HAND_CASES["one_segment"][0]), 0, NONE]
    assert n("record_per_segment")[0] == 7 and n("bytes_before_first_segment")[0] == 7
    assert n("empty_segments") == [7, len(HAND_CASES["one_segment"][0]), 0, NONE]
    assert n("short_segment")[2:] == [1, 1]
    assert n("crosses_segment_end")[2:] == [2, 0]  # the cut record, and its rest read as a header
    assert n("huge_key_size")[0] == 1 and n("huge_value_size")[0] == 1 and n("sizes_wrap_together")[0] == 1
    assert n("nested_table") == [3, len(HAND_CASES["nested_table"][0]), 0, NONE]
    for name in ("wild_lands_on_record", "wild_lands_on_segment_end", "wild_lands_on_stream_end"):
        assert n(name)[2] == 0


@pytest.mark.parametrize("segmented", [False, True], ids=["last_segment", "middle_segment"])
def test_last_record_cut_at_every_byte(segmented):
    """The last record of a segment cut after 0 .. size - 1 of its bytes: the
    records in front stay, the cut one is the tail (none when cut at 0)."""
    rng = np.random.default_rng(0x637574)
    front, last, behind = table(3, rng), rec(b"the-key", b"the value of it"), table(2, rng)
    for cut in range(len(last)):
        head = b"".join(front) + last[:cut]
        stream, seg = (head + b"".join(behind), [0, len(head)]) if segmented else (head, None)
        got = frame_closed(stream, seg)
        same(deserialize_loop(stream, seg), got)
        assert got[3][0] == 3 + (2 if segmented else 0)
        assert got[3][2:] == ([1, 0] if cut else [0, NONE])
        assert int(got[2][0]) == len(head) - cut
