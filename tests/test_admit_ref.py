"""tests/admit_ref.py against itself and the host class: the literal engine loop
equals the closed form on seeded random sequences, the ToBytes layout is pinned
by a hand-written vector, and nakevaleng_amd/tokenbucket.py's TokenBucket is
held to the literal statement by statement.  No GPU."""
import numpy as np
import pytest

from tests import admit_ref as ref


def random_case(rng, n, users=6, start=b"$", illegal=0.15, same_second=0.6):
    """(requests, stored): several users, keys legal and not, times with steps of
    0, 1, R, R + 1 and more; stored buckets with Tokens <= 0, above Max, a
    Timestamp in the past, at the edge and in the future, their own Max and R."""
    pool = [rng.bytes(int(k)) for k in rng.integers(0, 12, users)]
    R, Max = int(rng.integers(1, 5)), int(rng.integers(1, 7))
    t, requests = 1000, []
    for _ in range(n):
        s = rng.random()
        t += 0 if s < same_second else int(rng.choice([1, R, R + 1, int(rng.integers(0, 15))]))
        user = pool[int(rng.integers(0, len(pool)))]
        key = (start if rng.random() < illegal else b"k") + rng.bytes(int(rng.integers(len(start), 9)))
        requests.append((user, key, t))
    stored = {}
    for u in pool:
        kind = int(rng.integers(0, 5))
        m, r = int(rng.integers(1, 7)), int(rng.integers(1, 5))
        if kind == 1:
            stored[u] = (m, int(rng.integers(-4, 1)), 1000 - int(rng.integers(0, 10)), r)
        elif kind == 2:
            stored[u] = (m, m + int(rng.integers(1, 4)), 1000 + int(rng.integers(0, 12)), r)  # the future
        elif kind == 3:
            stored[u] = (m, int(rng.integers(0, m + 1)), 1000 - r - 1 + int(rng.integers(0, 3)), r)  # the edge
    return requests, stored, Max, R


@pytest.mark.parametrize("seed", range(40))
def test_literal_equals_closed_form(seed):
    rng = np.random.default_rng(0x61646D00 + seed)
    start = b"$" if seed % 2 else b"$#!"
    seen = set()
    for n in (0, 1, 7, 60, 200, 400):
        requests, stored, Max, R = random_case(rng, n, start=start)
        lit = ref.admit_literal(requests, start, Max, R, stored)
        closed = ref.admit_closed(requests, start, Max, R, stored)
        assert lit == closed
        seen |= set(lit.verdict)
    assert seen == {ref.ILLEGAL, ref.ALLOWED, ref.THROTTLED}  # the sequences reach every answer


def test_no_key_means_no_islegal_step():
    requests = [(b"u", None, 5), (b"u", None, 5), (b"v", None, 6)]
    assert ref.admit_literal(requests, b"$", 1, 1) == ref.admit_closed(requests, b"$", 1, 1)
    assert ref.admit_literal(requests, b"$", 1, 1).verdict == [ref.ALLOWED, ref.THROTTLED, ref.ALLOWED]


def test_to_bytes_layout():
    """MaxTokens, Tokens, Timestamp, ResetInterval as four little-endian u64 (tokenbucket.go:67-74)."""
    want = bytes([100, 0, 0, 0, 0, 0, 0, 0,
                  0xFD, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF,  # Tokens -3
                  0x00, 0xF1, 0x53, 0x65, 0, 0, 0, 0,  # 1700000000
                  0x3C, 0x01, 0, 0, 0, 0, 0, 0])  # 316
    tb = ref.TokenBucket(100, -3, 1700000000, 316)
    assert tb.ToBytes() == want and len(want) == 32
    assert ref.TokenBucket.FromBytes(want).tuple() == (100, -3, 1700000000, 316)
    from nakevaleng_amd.tokenbucket import TokenBucket
    assert TokenBucket(100, -3, 1700000000, 316).to_bytes() == want
    assert TokenBucket.from_bytes(want).to_bytes() == want and TokenBucket.from_bytes(want).Tokens == -3


def test_islegal_matches_every_byte_and_panics_on_a_short_key():
    eng = ref.Engine(b"$#!")
    assert not eng.IsLegal(b"$#!") and not eng.IsLegal(b"$#!x") and eng.IsLegal(b"$#?") and eng.IsLegal(b"x#!")
    with pytest.raises(IndexError):
        eng.IsLegal(b"$#")
    with pytest.raises(IndexError):
        ref.admit_closed([(b"u", b"ab", 0)], b"$#!")


def test_engine_prologue_writes_the_bucket_before_the_record():
    eng = ref.Engine(b"$", 2, 1)
    eng.clock[0] = 50
    assert eng.Put(b"u", b"k1", b"v1") and eng.Put(b"u", b"k2", b"v2")
    assert not eng.Put(b"u", b"k3", b"v3") and eng.waits == [1]  # throttled: nothing written
    assert not eng.Put(b"u", b"$u", b"x")  # illegal: before any bucket is read
    assert [r.Key for r in eng.log] == [b"$u", b"k1", b"$u", b"k2"]
    assert [ref.TokenBucket.FromBytes(eng.log[i].Value).tuple() for i in (0, 2)] == [(2, 1, 50, 1), (2, 0, 50, 1)]
    assert all(r.Timestamp == 50 for r in eng.log)
    eng.clock[0] = 52  # 52 - 50 > 1: a reset
    rec, found = eng.Get(b"u", b"k1")
    assert found and rec.Value == b"v1" and eng.log[-1].Key == b"$u"
    assert ref.TokenBucket.FromBytes(eng.log[-1].Value).tuple() == (2, 1, 52, 1)


@pytest.mark.parametrize("seed", range(10))
def test_host_class_follows_the_literal(seed):
    from nakevaleng_amd import tokenbucket as tbm
    rng = np.random.default_rng(0x61646D80 + seed)
    Max, R = int(rng.integers(1, 6)), int(rng.integers(1, 4))
    t = [int(rng.integers(0, 100))]
    lit = ref.TokenBucket.New(Max, R, lambda: t[0])
    host = tbm.TokenBucket.new(Max, R, t[0])
    assert host.to_bytes() == lit.ToBytes()
    if seed % 3 == 0:  # a stored bucket with its own fields
        img = ref.TokenBucket(Max, int(rng.integers(-3, Max + 3)), t[0] + int(rng.integers(-5, 6)), R).ToBytes()
        lit, host = ref.TokenBucket.FromBytes(img), tbm.TokenBucket.from_bytes(img)
    for _ in range(200):
        t[0] += int(rng.choice([0, 0, 0, 1, R, R + 1]))
        assert host.has_enough_tokens(t[0]) == lit.HasEnoughTokens(lambda: t[0])
        assert host.to_bytes() == lit.ToBytes()


def test_host_class_validates_like_the_reference():
    from nakevaleng_amd import tokenbucket as tbm
    with pytest.raises(ValueError, match="maxTokens must be a positive number, but 0 was given"):
        tbm.TokenBucket.new(0, 1, 0)
    with pytest.raises(ValueError, match="resetInterval must be a positive number, but -2 was given"):
        tbm.validate_params(3, -2)
    with pytest.raises(ValueError):
        ref.TokenBucket.New(0, 1, lambda: 0)
    with pytest.raises(ValueError):
        tbm.TokenBucket.from_bytes(bytes(31))
