"""GPU: the engine's admission on the device (nkv_admit_dev,
tokenbucket.admit_many, engine.put_many / get_many) against tests/admit_ref.py:
every byte of d_verdict, d_bucket, d_wait, d_group and d_last is held to the
literal engine loop fed one request at a time.  Outputs lie in guarded buffers
of exactly their size at their minimum promised alignment (tests/guarded.py);
inputs are snapshotted and compared after every call.

Sizes: 0, 1, 63, 64, 65 (the wave combine of the grouping), 1023, 1024, 1025
(the sort's tile edge), 2049 and 5000 (one and several merge passes)."""
import struct

import numpy as np
import pytest

from tests import admit_ref as ref
from tests import live_memtable_ref as mref
from tests.guarded import frozen, guarded

pytestmark = pytest.mark.gpu

INVALID = 2  # NKV_ERR_INVALID
FILL = 0xA5
LIVE, TOMBSTONE, ABSENT = 1, 2, 0
SIZES = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2049, 5000]
MIXES = ["one", "distinct", "hot", "lastbyte", "length"]
START = b"$#!"  # a multi-byte InternalStart
BAD_IMAGE = ref.TokenBucket(0, 0, 0, 0).ToBytes()  # MaxTokens 0: refused (bit 3) wherever it is read


def _torch():
    import torch
    return torch


def _dev(a):
    a = np.ascontiguousarray(a).view(np.uint8)
    return _torch().from_numpy((a if a.size else np.zeros(8, np.uint8)).copy()).cuda()


def pack(items, at, share):
    """(blob, off, len): item i at blob + off[i], the blob starting with `at`
    filler bytes and one more between spans, so spans begin at odd and even
    addresses alike.  share: equal items use one span (repeated spans)."""
    parts, off, where, pos = [b"\xEE" * at], [], {}, at
    for it in items:
        if share and it in where:
            off.append(where[it])
            continue
        where[it] = pos
        off.append(pos)
        parts.append(it + b"\xEE")
        pos += len(it) + 1
    return (np.frombuffer(b"".join(parts) + b"\xEE", np.uint8), np.asarray(off, np.uint64),
            np.fromiter((len(it) for it in items), np.uint64, count=len(items)))


def run(nkv, requests, start=START, Max=100, R=1, stored=None, ts_all=None, share=False, user_at=1, key_at=3,
        outputs=("bucket", "wait", "group", "last"), with_err=True, override=None, bucket_at=8):
    """One nkv_admit_dev.  requests: (user, key or None, now); stored: per request
    (status byte, 32-byte image or None) or None; override(fields): a hook that
    edits the struct's fields (a dict) before the call.  Returns (rc, err word
    or None, dict of output bytes as the buffers hold them afterwards)."""
    _lib, ctx = nkv
    torch = _torch()
    n = len(requests)
    ub, uoff, ulen = pack([r[0] for r in requests], user_at, share)
    keep = {"users": _dev(ub), "uoff": _dev(uoff), "ulen": _dev(ulen)}
    f = {"users": keep["users"].data_ptr(), "users_len": ub.size, "uoff": keep["uoff"].data_ptr(),
         "ulen": keep["ulen"].data_ptr(), "keys": None, "keys_len": 0, "koff": None, "klen": None, "ts": None,
         "ts_all": 0, "buckets": None, "boff": None, "bstatus": None, "n": n}
    if n == 0 or requests[0][1] is not None:
        kb, koff, klen = pack([r[1] for r in requests], key_at, share)
        keep.update(keys=_dev(kb), koff=_dev(koff), klen=_dev(klen))
        f.update(keys=keep["keys"].data_ptr(), keys_len=kb.size, koff=keep["koff"].data_ptr(),
                 klen=keep["klen"].data_ptr())
    if ts_all is None:
        keep["ts"] = _dev(np.asarray([r[2] for r in requests], np.int64))
        f["ts"] = keep["ts"].data_ptr()
    else:
        f["ts_all"] = ts_all
    if stored is not None:
        images, boff = [b"\xEE" * 5], []  # images at odd addresses
        for status, img in stored:
            boff.append(5 + 33 * (len(images) - 1) if img is not None else 1 << 62)
            if img is not None:
                images.append(img + b"\xEE")
        keep.update(buckets=_dev(np.frombuffer(b"".join(images), np.uint8)), boff=_dev(np.asarray(boff, np.uint64)),
                    bstatus=_dev(np.asarray([s for s, _ in stored], np.uint8)))
        f.update(buckets=keep["buckets"].data_ptr(), boff=keep["boff"].data_ptr(),
                 bstatus=keep["bstatus"].data_ptr())
    if override:
        override(f)
    req = _lib.NkvRequests(*(f[name] for name, _ in _lib.NkvRequests._fields_))
    ins = [frozen(t) for t in keep.values()]
    sizes = {"verdict": (n, 1), "bucket": (32 * n, bucket_at), "wait": (8 * n, 8), "group": (8 * n, 8), "last": (n, 1)}
    bufs = {k: guarded(*sizes[k], fill=FILL) for k in ("verdict",) + tuple(outputs)}
    p_err, err_check = guarded(4, 4, fill=FILL)
    torch.cuda.synchronize()
    rc = _lib.lib().nkv_admit_dev(ctx.h, req, start, len(start), Max, R, bufs["verdict"][0],
                                  *(bufs[k][0] if k in bufs else None for k in ("bucket", "wait", "group", "last")),
                                  p_err if with_err else None)
    torch.cuda.synchronize()
    for intact in ins:
        intact()
    err = err_check()
    out = {k: check() for k, (_, check) in bufs.items()}
    return rc, (int(err.view(np.uint32)[0]) if with_err and n and rc == 0 else None), out


def expect(out, want, n):
    """Every byte of every output given."""
    assert out["verdict"].tolist() == want.verdict
    if "bucket" in out:
        assert out["bucket"].tobytes() == want.image()
    if "wait" in out:
        assert out["wait"].view(np.int64).tolist() == want.wait
    if "group" in out:
        assert out["group"].view(np.uint64).tolist() == want.group
    if "last" in out:
        assert out["last"].tolist() == want.last


def untouched(out):
    assert all((v == FILL).all() for v in out.values())


def stored_dict(requests, stored):
    """user -> image as the literal engine finds it: the LIVE entry of the user's first legal request."""
    if stored is None:
        return None
    d, seen = {}, set()
    for (user, key, _), (status, img) in zip(requests, stored):
        if (key is not None and key[:len(START)] == START) or user in seen:
            continue
        seen.add(user)
        if status == LIVE:
            d[user] = img
    return d


def users_of(mix, n, rng):
    if mix == "one":
        return [b"the-only-user"] * n
    if mix == "distinct":
        return [struct.pack("<I", i) + b"-distinct" for i in range(n)]
    if mix == "hot":  # a few hot users (the empty one among them) among many
        pool = [rng.bytes(int(k)) for k in rng.integers(1, 24, 200)]
        hot = [b"", b"hot-user-with-a-long-name", b"h"]
        return [hot[int(rng.integers(0, 3))] if rng.random() < 0.6 else pool[int(rng.integers(0, 200))]
                for _ in range(n)]
    if mix == "lastbyte":  # equal but for the last byte, behind equal 8-byte prefixes
        return [b"same-prefix-0123" + bytes([int(c)]) for c in rng.integers(0, 8, n)]
    assert mix == "length"  # equal but for the length, the empty user included
    return [b"A" * int(k) for k in rng.integers(0, 20, n)]


def keys_of(n, rng):
    """Legal and illegal keys interleaved: the start itself, the start with a
    tail, a key matching all but the start's last byte, one exactly as long."""
    kinds = [lambda: b"key-" + rng.bytes(int(rng.integers(0, 9))), lambda: START, lambda: START + rng.bytes(4),
             lambda: START[:-1] + b"?" + rng.bytes(3), lambda: START[:-1] + b"?", lambda: b"?" + START[1:]]
    return [kinds[int(k)]() if rng.random() < 0.3 else kinds[0]() for k in rng.integers(0, len(kinds), n)]


def times_of(n, rng, R):
    steps = np.where(rng.random(n) < 0.96, 0, rng.choice([1, R, R + 1, 3 * R + 2], n))
    return (1000 + np.cumsum(steps)).tolist()


def stored_of(requests, rng):
    """Per request what a lookup of start ++ user answered: the same for every
    request of a user.  Kinds: nothing, a tombstone, and live buckets with their
    own MaxTokens / ResetInterval, Tokens 0, negative and above Max, Timestamps
    behind, at the edge and ahead of the batch's first second."""
    per_user = {}
    for user, _, _ in requests:
        if user in per_user:
            continue
        kind = int(rng.integers(0, 7))
        m, r = int(rng.integers(1, 9)), int(rng.integers(1, 5))
        per_user[user] = [(ABSENT, None), (TOMBSTONE, None),
                          (LIVE, ref.TokenBucket(m, 0, 1000, r).ToBytes()),
                          (LIVE, ref.TokenBucket(m, -int(rng.integers(1, 5)), 1000 - r, r).ToBytes()),
                          (LIVE, ref.TokenBucket(m, m + 3, 1000 + int(rng.integers(0, 9)), r).ToBytes()),
                          (LIVE, ref.TokenBucket(m, int(rng.integers(0, m + 1)), 1000 - r - 1, r).ToBytes()),
                          (LIVE, ref.TokenBucket(m, m, 990, r).ToBytes())][kind]
    return [per_user[user] for user, _, _ in requests]


@pytest.mark.parametrize("mix", MIXES)
@pytest.mark.parametrize("n", SIZES)
def test_every_output_byte(nkv, n, mix):
    rng = np.random.default_rng(0x61646D10 + 31 * n + MIXES.index(mix))
    Max, R = int(rng.integers(1, 5)), int(rng.integers(1, 4))
    requests = list(zip(users_of(mix, n, rng), keys_of(n, rng), times_of(n, rng, R)))
    stored = stored_of(requests, rng) if n % 2 else None
    rc, err, out = run(nkv, requests, START, Max, R, stored, share=bool(n % 3), user_at=1 + n % 4, key_at=n % 5)
    assert rc == 0
    if n == 0:
        return untouched(out)  # n = 0 writes nothing
    assert err == 0
    want = ref.admit_literal(requests, START, Max, R, stored_dict(requests, stored))
    expect(out, want, n)
    if n >= 1023:
        assert {ref.ILLEGAL, ref.ALLOWED} <= set(want.verdict)
    if n >= 1023 and mix in ("one", "hot"):
        assert ref.THROTTLED in want.verdict


@pytest.mark.parametrize("n", [65, 1025])
def test_one_time_for_the_batch(nkv, n):
    rng = np.random.default_rng(0x61646D20 + n)
    requests = [(u, k, 77) for u, k in zip(users_of("hot", n, rng), keys_of(n, rng))]
    rc, err, out = run(nkv, requests, START, 3, 2, ts_all=77)
    assert (rc, err) == (0, 0)
    expect(out, ref.admit_literal(requests, START, 3, 2), n)


@pytest.mark.parametrize("n", [64, 1025, 2049])
def test_every_request_a_reset(nkv, n):
    """One user, every request more than R after the one before: n windows of one request."""
    R = 2
    requests = [(b"u", b"key", 10 + (R + 1) * i) for i in range(n)]
    stored = [(LIVE, ref.TokenBucket(1, 0, 10 - R - 1, R).ToBytes())] * n  # the first request resets as well
    rc, err, out = run(nkv, requests, START, 1, R, stored)
    assert (rc, err) == (0, 0)
    want = ref.admit_literal(requests, START, 1, R, stored_dict(requests, stored))
    assert want.verdict == [ref.ALLOWED] * n
    expect(out, want, n)


def test_a_reset_at_the_tile_edge(nkv):
    """One user: resets at sorted positions 1023, 1024 and 1025 and 2048, between windows of hundreds."""
    R, Max, n = 3, 1000, 2100
    t, times = 50, []
    for i in range(n):
        if i in (1023, 1024, 1025, 2048):
            t += R + 1
        times.append(t)
    requests = [(b"edge", b"key", x) for x in times]
    rc, err, out = run(nkv, requests, START, Max, R)
    assert (rc, err) == (0, 0)
    want = ref.admit_literal(requests, START, Max, R)
    assert want.verdict[1022:1026] == [ref.THROTTLED, ref.ALLOWED, ref.ALLOWED, ref.ALLOWED]
    expect(out, want, n)


def test_window_edge_r_against_r_plus_1(nkv):
    """t - Timestamp == R is still the old window, R + 1 a reset (tokenbucket.go:52 is a strict >)."""
    R = 5
    img = ref.TokenBucket(4, 0, 100, R).ToBytes()
    requests = [(b"at-r", b"key", 100 + R), (b"past-r", b"key", 100 + R + 1), (b"at-r", b"key", 100 + R + 1)]
    stored = [(LIVE, img)] * 3
    rc, err, out = run(nkv, requests, START, 9, 9, stored)
    assert (rc, err) == (0, 0)
    want = ref.admit_literal(requests, START, 9, 9, stored_dict(requests, stored))
    assert want.verdict == [ref.THROTTLED, ref.ALLOWED, ref.ALLOWED] and want.wait == [0 + R - R, 0, 0]
    expect(out, want, 3)


@pytest.mark.parametrize("Max", [1, 5, 64, 1024])
def test_rank_max_minus_1_against_max(nkv, Max):
    """In one window the request of rank Max - 1 takes the last token and rank Max is throttled;
    after the reset the same again."""
    n = 2 * (Max + 2)
    requests = [(b"u", b"key", 20 if i < Max + 2 else 22) for i in range(n)]
    rc, err, out = run(nkv, requests, START, Max, 1)
    assert (rc, err) == (0, 0)
    want = ref.admit_literal(requests, START, Max, 1)
    assert want.verdict == ([ref.ALLOWED] * Max + [ref.THROTTLED] * 2) * 2
    expect(out, want, n)


def test_only_the_first_legal_entry_is_read(nkv):
    """A user's stored bucket is the entry of its first LEGAL request: every
    other entry, and boff where bstatus is not LIVE, is never read.  The unread
    LIVE entries hold a bucket the call would refuse (MaxTokens 0)."""
    good = ref.TokenBucket(2, 1, 40, 7).ToBytes()
    requests = [(b"a", START + b"x", 41), (b"a", b"key", 41), (b"b", b"key", 41), (b"a", b"key", 42),
                (b"b", b"key", 42), (b"c", b"key", 43), (b"d", b"key", 43), (b"a", b"key", 44)]
    stored = [(LIVE, BAD_IMAGE), (LIVE, good), (TOMBSTONE, None), (LIVE, BAD_IMAGE), (LIVE, BAD_IMAGE),
              (ABSENT, None), (3, None), (LIVE, BAD_IMAGE)]
    rc, err, out = run(nkv, requests, START, 5, 1, stored)
    assert (rc, err) == (0, 0)
    want = ref.admit_literal(requests, START, 5, 1, {b"a": good})
    assert want.verdict == [0, 1, 1, 2, 1, 1, 1, 2]
    expect(out, want, len(requests))


def test_no_keys_means_every_request_is_legal(nkv):
    rng = np.random.default_rng(0x61646D30)
    requests = [(u, None, t) for u, t in zip(users_of("length", 300, rng), times_of(300, rng, 2))]
    rc, err, out = run(nkv, requests, START, 2, 2)
    assert (rc, err) == (0, 0)
    expect(out, ref.admit_literal(requests, START, 2, 2), 300)


def test_outputs_are_optional_but_the_verdict(nkv):
    rng = np.random.default_rng(0x61646D31)
    requests = list(zip(users_of("hot", 130, rng), keys_of(130, rng), times_of(130, rng, 1)))
    want = ref.admit_literal(requests, START, 2, 1)
    for outputs in ((), ("bucket",), ("wait", "last"), ("group",)):
        rc, err, out = run(nkv, requests, START, 2, 1, outputs=outputs)
        assert (rc, err) == (0, 0) and set(out) == {"verdict", *outputs}
        expect(out, want, 130)


@pytest.mark.parametrize("bucket_at", [8, 16, 24, 0])
def test_bucket_images_at_8_and_16_byte_alignment(nkv, bucket_at):
    """d_bucket is promised 8-byte alignment; at 16 the image goes out as two 16-byte stores."""
    rng = np.random.default_rng(0x61646D32)
    requests = list(zip(users_of("hot", 1025, rng), keys_of(1025, rng), times_of(1025, rng, 1)))
    rc, err, out = run(nkv, requests, START, 2, 1, bucket_at=bucket_at)
    assert (rc, err) == (0, 0)
    expect(out, ref.admit_literal(requests, START, 2, 1), 1025)


@pytest.mark.parametrize("n,cut", [(130, 64), (2100, 1025)])
def test_two_batches_chained_equal_one(nkv, n, cut):
    """The second batch's stored buckets are the first one's d_bucket entries where d_last is set."""
    rng = np.random.default_rng(0x61646D40 + n)
    Max, R = 3, 2
    requests = list(zip(users_of("hot", n, rng), keys_of(n, rng), times_of(n, rng, R)))
    stored = stored_of(requests, rng)
    rc, err, whole = run(nkv, requests, START, Max, R, stored)
    assert (rc, err) == (0, 0)
    rc, err, a = run(nkv, requests[:cut], START, Max, R, stored[:cut])
    assert (rc, err) == (0, 0)
    final = {requests[i][0]: a["bucket"][32 * i:32 * i + 32].tobytes() for i in np.flatnonzero(a["last"])}
    chained = [(LIVE, final[u]) if u in final else s for (u, _, _), s in zip(requests[cut:], stored[cut:])]
    rc, err, b = run(nkv, requests[cut:], START, Max, R, chained)
    assert (rc, err) == (0, 0)
    for k in ("verdict", "bucket", "wait"):
        assert np.array_equal(np.concatenate([a[k], b[k]]), whole[k]), k
    expect(whole, ref.admit_literal(requests, START, Max, R, stored_dict(requests, stored)), n)


def _base(n=70):
    return [(b"user%d" % (i % 5), b"key%d" % i, 100 + i // 10) for i in range(n)]


def test_verdict_short_key(nkv):
    requests = _base()
    requests[33] = (b"user3", START[:-1], 103)  # one byte shorter than start: the reference panics
    rc, err, out = run(nkv, requests)
    assert (rc, err) == (0, 2)
    untouched(out)


def test_verdict_decreasing_time(nkv):
    requests = _base()
    requests[64] = (b"user4", b"key64", 105)  # behind 106: decreasing across two users (and two waves)
    assert requests[63][2] == 106
    rc, err, out = run(nkv, requests)
    assert (rc, err) == (0, 4)
    untouched(out)
    for bad in (-1, 1 << 62):
        rc, err, out = run(nkv, _base(), ts_all=bad)
        assert (rc, err) == (0, 4)
        untouched(out)
    rc, err, out = run(nkv, _base(), ts_all=(1 << 62) - 1)
    assert (rc, err) == (0, 0)


def test_verdict_span_outside_its_blob(nkv):
    def user_len(f):
        f["users_len"] -= 3  # the last user's span now ends one byte past the blob

    def key_off(f):
        f["keys_len"] = 4  # nearly every key lies outside

    for hook in (user_len, key_off):
        rc, err, out = run(nkv, _base(), override=hook)
        assert (rc, err) == (0, 1)
        untouched(out)


def test_verdict_stored_bucket_out_of_range(nkv):
    for img in (BAD_IMAGE, ref.TokenBucket(1, 1, 0, 0).ToBytes(), ref.TokenBucket(1, 1, -1, 1).ToBytes(),
                ref.TokenBucket(1 << 62, 1, 0, 1).ToBytes(), ref.TokenBucket(1, 1, 1 << 62, 1).ToBytes()):
        requests = _base()
        stored = [(ABSENT, None)] * len(requests)
        stored[2] = (LIVE, img)  # user2's first request
        rc, err, out = run(nkv, requests, stored=stored)
        assert (rc, err) == (0, 8)
        untouched(out)
    # Tokens may be anything, and the largest fields pass
    stored[2] = (LIVE, ref.TokenBucket((1 << 62) - 1, -(1 << 63), (1 << 62) - 1, (1 << 62) - 1).ToBytes())
    rc, err, out = run(nkv, requests, stored=stored)
    assert (rc, err) == (0, 0)
    expect(out, ref.admit_literal(requests, START, 100, 1, stored_dict(requests, stored)), len(requests))


def test_without_d_err_the_call_answers_itself(nkv):
    requests = _base()
    rc, _, out = run(nkv, requests, with_err=False)
    assert rc == 0
    expect(out, ref.admit_literal(requests, START, 100, 1), len(requests))
    requests[5] = (b"user0", b"$", 100)
    rc, _, out = run(nkv, requests, with_err=False)
    assert rc == INVALID
    untouched(out)


def test_refused_before_any_launch(nkv):
    _lib, ctx = nkv
    requests = _base(8)

    def refused(**kw):
        rc, _, out = run(nkv, requests, **kw)
        assert rc == INVALID
        untouched(out)

    refused(start=b"")
    refused(start=b"x" * 65)
    for bad in (0, -1, 1 << 62):
        refused(Max=bad)
        refused(R=bad)
    refused(override=lambda f: f.update(n=1 << 31))
    refused(override=lambda f: f.update(uoff=None))
    refused(override=lambda f: f.update(ulen=None))
    refused(override=lambda f: f.update(users=None))
    refused(override=lambda f: f.update(keys=None))
    refused(override=lambda f: f.update(klen=None))
    refused(override=lambda f: f.update(bstatus=f["uoff"]))  # stored buckets: not NULL together
    refused(override=lambda f: f.update(buckets=f["users"], boff=f["uoff"]))
    req = _lib.NkvRequests()
    L = _lib.lib()
    assert L.nkv_admit_dev(ctx.h, None, b"$", 1, 100, 1, None, None, None, None, None, None) == INVALID
    assert L.nkv_admit_dev(ctx.h, req, None, 1, 100, 1, None, None, None, None, None, None) == INVALID
    assert L.nkv_admit_dev(ctx.h, req, b"$", 1, 100, 1, None, None, None, None, None, None) == 0  # n = 0
    req.n = 1
    assert L.nkv_admit_dev(ctx.h, req, b"$", 1, 100, 1, None, None, None, None, None, None) == INVALID


def test_admit_many_defaults_and_stored_forms(nkv):
    from nakevaleng_amd import tokenbucket as tbm
    users = [b"u", b"v", b"u", b"w", b"u"]
    keys = [b"k1", b"$v", b"k2", b"k3", b"k4"]
    old = tbm.TokenBucket(2, 1, 1000, 1)
    got = tbm.admit_many(users, keys, 1000, stored={b"u": old, b"w": old.to_bytes()})
    want = ref.admit_literal(list(zip(users, keys, [1000] * 5)), b"$", 100, 1,
                             {b"u": old.to_bytes(), b"w": old.to_bytes()})
    assert got.verdict.tolist() == want.verdict == [1, 0, 2, 1, 2]
    assert got.bucket.tobytes() == want.image() and got.wait.tolist() == want.wait
    assert got.group.tolist() == want.group and got.last.tolist() == [bool(x) for x in want.last]
    got = tbm.admit_many(users, None, [5, 5, 6, 6, 8], max_tokens=1, reset_interval=2,
                         stored=[None, None, None, old, None])
    want = ref.admit_literal(list(zip(users, [None] * 5, [5, 5, 6, 6, 8])), b"$", 1, 2, {b"w": old.to_bytes()})
    assert got.verdict.tolist() == want.verdict and got.bucket.tobytes() == want.image()
    assert tbm.admit_many([], [], 0).verdict.size == 0
    with pytest.raises(_lib_error(nkv)):
        tbm.admit_many([b"u"], [b""], 0)  # a key shorter than start


def _lib_error(nkv):
    return nkv[0].NkvError


RULE = (3, 9, 600)  # both rules: capacity 9, threshold 600 bytes


def _engine_batches(rng):
    """Two batches over four users; a throttled and an illegal request in each."""
    users = [b"ana", b"bo", b"", b"cy"]
    b1 = [(users[i % 4], b"key-%02d" % (i % 7), b"value-%d" % i, 500) for i in range(13)]
    b1[4] = (b"ana", b"$ana", b"forged bucket", 500)  # illegal
    b2 = [(users[int(rng.integers(0, 4))], b"key-%02d" % (99 if i == 10 else i % 7),
           rng.bytes(int(rng.integers(0, 30))), 500 + i // 4) for i in range(12)]
    b2[7] = (b"bo", b"$", b"", b2[7][3])
    return b1, b2


def test_engine_put_many_writes_what_the_engine_writes(nkv):
    from nakevaleng_amd import engine
    from nakevaleng_amd.memtable import Memtable
    rng = np.random.default_rng(0x61646D50)
    mt = Memtable(256, 1 << 16, *RULE)
    eng = ref.Engine(b"$", 2, 1)
    done = 0
    for batch in _engine_batches(rng):
        want = []
        for user, key, val, now in batch:
            eng.clock[0] = now
            before = len(eng.log)
            ok = eng.Put(user, key, val)
            want.append(ref.ALLOWED if ok else (ref.ILLEGAL if key[:1] == b"$" else ref.THROTTLED))
            assert len(eng.log) - before == (2 if ok else 0)
        verdict, is_new, flush_at = engine.put_many(mt, (), [b[0] for b in batch], [b[1] for b in batch],
                                                    [b[2] for b in batch], [b[3] for b in batch], max_tokens=2)
        assert verdict.tolist() == want and {0, 1, 2} <= set(want)
        trace = mref.add_closed(eng.log, *RULE)
        n = len(eng.log)
        assert mt.d_log[:mt.log_len].cpu().numpy().tobytes() == b"".join(r.ToBytes() for r in eng.log)
        assert is_new.tolist() == trace.is_new[done:n]
        assert mt.count() == (trace.count[-1], trace.memusage[-1]) and mt.n == n
        assert flush_at == (None if trace.flush_at(done, n) == mref.NONE else trace.flush_at(done, n))
        done = n
    # the second batch read the first one's buckets back from the memtable: "ana" spent both tokens at 500
    assert ref.TokenBucket.FromBytes(eng.store[b"$ana"].Value).Timestamp >= 500


def test_engine_get_many_reads_what_the_engine_reads(nkv):
    from nakevaleng_amd import engine
    from nakevaleng_amd.memtable import Memtable
    rng = np.random.default_rng(0x61646D51)
    mt = Memtable(256, 1 << 16, *RULE)
    eng = ref.Engine(b"$", 2, 1)
    b1, b2 = _engine_batches(rng)
    for user, key, val, now in b1:
        eng.clock[0] = now
        eng.Put(user, key, val)
    engine.put_many(mt, (), [b[0] for b in b1], [b[1] for b in b1], [b[2] for b in b1], 500, max_tokens=2)
    done = len(eng.log)
    want_v, want_vals = [], []
    for user, key, _, now in b2:
        eng.clock[0] = now
        before = len(eng.log)
        rec, found = eng.Get(user, key)
        admitted = len(eng.log) > before
        want_v.append(ref.ALLOWED if admitted else (ref.ILLEGAL if key[:1] == b"$" else ref.THROTTLED))
        want_vals.append(rec.Value if found else None)
    verdict, values, is_new, flush_at = engine.get_many(mt, (), [b[0] for b in b2], [b[1] for b in b2],
                                                        [b[3] for b in b2], max_tokens=2)
    assert verdict.tolist() == want_v and {0, 1, 2} <= set(want_v)
    assert values == want_vals and any(v is not None for v in values)
    trace = mref.add_closed(eng.log, *RULE)
    assert mt.d_log[:mt.log_len].cpu().numpy().tobytes() == b"".join(r.ToBytes() for r in eng.log)
    assert is_new.tolist() == trace.is_new[done:] and mt.count() == (trace.count[-1], trace.memusage[-1])
    assert flush_at == (None if trace.flush_at(done) == mref.NONE else trace.flush_at(done))
