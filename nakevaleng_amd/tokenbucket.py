"""The reference's rate limiter (ds/tokenbucket/tokenbucket.go) and the engine's
admission step over a batch of requests on the device (nkv_admit_dev).

TokenBucket is one bucket on the host, method for method: new, validate_params,
has_enough_tokens(now), to_bytes, from_bytes.  Where the reference calls
time.Now().Unix() the caller passes `now`.

admit_many() is the step CoreEngine.Put, Get and Delete run first
(coreeng.go:63-75, 184-199, 223-234) for n requests in arrival order: IsLegal of
the key, then the user's bucket.  It answers what the n requests would have been
answered one after the other; include/nkv_merkle.h states the contract,
csrc/admit_dev.hpp the closed form.  There is no host fallback: without the
library or a device it raises.
"""
from __future__ import annotations

import ctypes
import struct
import time
from typing import NamedTuple, Optional, Sequence

import numpy as np

from . import _lib
from ._dev import pack_keys, u8, up

ILLEGAL, ALLOWED, THROTTLED = _lib.NKV_ADMIT_ILLEGAL, _lib.NKV_ADMIT_ALLOWED, _lib.NKV_ADMIT_THROTTLED
_IMG = struct.Struct("<QQQQ")
_M64 = 2**64 - 1


def validate_params(max_tokens: int, reset_interval: int) -> None:
    """tokenbucket.ValidateParams (tokenbucket.go:35-46); the error texts are the reference's."""
    if max_tokens <= 0:
        raise ValueError(f"maxTokens must be a positive number, but {max_tokens} was given")
    if reset_interval <= 0:
        raise ValueError(f"resetInterval must be a positive number, but {reset_interval} was given")


class TokenBucket:
    """tokenbucket.TokenBucket (tokenbucket.go:11-16)."""

    __slots__ = ("MaxTokens", "Tokens", "Timestamp", "ResetInterval")

    def __init__(self, MaxTokens: int, Tokens: int, Timestamp: int, ResetInterval: int):
        self.MaxTokens, self.Tokens, self.Timestamp, self.ResetInterval = (int(MaxTokens), int(Tokens),
                                                                           int(Timestamp), int(ResetInterval))

    @classmethod
    def new(cls, max_tokens: int, reset_interval: int, now: Optional[int] = None) -> "TokenBucket":
        """tokenbucket.New (tokenbucket.go:19-31); now None = int(time.time())."""
        validate_params(max_tokens, reset_interval)
        return cls(max_tokens, max_tokens, int(time.time()) if now is None else now, reset_interval)

    def has_enough_tokens(self, now: Optional[int] = None) -> bool:
        """HasEnoughTokens (tokenbucket.go:51-64) at time `now`."""
        now = int(time.time()) if now is None else int(now)
        if now - self.Timestamp > self.ResetInterval:
            self.Timestamp = now
            self.Tokens = self.MaxTokens - 1
            return True
        if self.Tokens > 0:
            self.Tokens -= 1
            return True
        return False

    def to_bytes(self) -> bytes:
        """ToBytes (tokenbucket.go:67-74): four little-endian u64."""
        return _IMG.pack(self.MaxTokens & _M64, self.Tokens & _M64, self.Timestamp & _M64, self.ResetInterval & _M64)

    @classmethod
    def from_bytes(cls, b) -> "TokenBucket":
        """FromBytes (tokenbucket.go:76-83): the first 32 bytes, as int64."""
        b = bytes(b)
        if len(b) < 32:
            raise ValueError(f"a bucket image is 32 bytes, got {len(b)}")  # the reference's slice panics
        return cls(*(x - 2**64 if x >= 2**63 else x for x in _IMG.unpack(b[:32])))

    def __eq__(self, o) -> bool:
        return isinstance(o, TokenBucket) and self.to_bytes() == o.to_bytes()

    def __repr__(self) -> str:
        return f"TokenBucket({self.MaxTokens}, {self.Tokens}, {self.Timestamp}, {self.ResetInterval})"


class Admission(NamedTuple):
    """Per request: verdict (uint8: ILLEGAL, ALLOWED, THROTTLED), bucket (n x 32
    uint8: the ToBytes image after the request), wait (int64 seconds to go of a
    throttled one), group (uint64: arrival index of the user's first legal
    request, 2^64 - 1 for an illegal one), last (bool: the user's last legal
    request of the batch, whose image is the user's final state)."""
    verdict: np.ndarray
    bucket: np.ndarray
    wait: np.ndarray
    group: np.ndarray
    last: np.ndarray


def _ptr(t):
    return None if t is None else t.data_ptr()


def admit_dev(n: int, d_users, users_len: int, d_uoff, d_ulen, d_keys=None, keys_len: int = 0, d_koff=None,
              d_klen=None, d_ts=None, ts_all: int = 0, d_buckets=None, d_boff=None, d_bstatus=None, start: bytes = b"$",
              max_tokens: int = 100, reset_interval: int = 1, device=None):
    """nkv_admit_dev over device arrays (torch uint8 tensors or None), on the
    current stream of the device.  Returns the five outputs as device tensors
    (verdict, bucket, wait, group, last as bytes); raises NkvError naming the
    verdict bits when the batch is refused."""
    import torch
    from .lsmtree import rank_device
    dev_index = rank_device(device)
    ctx = _lib.default_context(dev_index)
    dev = torch.device("cuda", dev_index)
    start = bytes(start)
    outs = [u8(dev, k * n) for k in (1, 32, 8, 8, 1)]
    d_err = u8(dev, 4)
    req = _lib.NkvRequests(_ptr(d_users), users_len, _ptr(d_uoff), _ptr(d_ulen), _ptr(d_keys), keys_len, _ptr(d_koff),
                           _ptr(d_klen), _ptr(d_ts), ts_all, _ptr(d_buckets), _ptr(d_boff), _ptr(d_bstatus), n)
    stream = torch.cuda.current_stream(dev)
    with ctx.on_stream(stream.cuda_stream):
        _lib.check(_lib.lib().nkv_admit_dev(ctx.h, ctypes.byref(req), start, len(start), max_tokens, reset_interval,
                                            *(t.data_ptr() for t in outs), d_err.data_ptr()), "admit")
        if n:
            err = int(d_err.cpu().numpy().view(np.uint32)[0])  # synchronizes the stream
            if err:
                what = ", ".join(name for bit, name in _lib.ADMIT_VERDICTS.items() if err & bit)
                raise _lib.NkvError(_lib.NKV_ERR_INVALID, f"admit refused (verdict {err}: {what})")
    return outs


def _stored_per_request(users, stored):
    """stored as one entry per request: None, or the Value found live under start ++ user."""
    if stored is None:
        return None
    if isinstance(stored, dict):
        stored = [stored.get(u) for u in users]
    stored = list(stored)
    if len(stored) != len(users):
        raise ValueError(f"admit_many: {len(stored)} stored buckets for {len(users)} requests")
    out = []
    for b in stored:
        if isinstance(b, TokenBucket):
            b = b.to_bytes()
        if b is not None and len(b) < 32:
            raise ValueError(f"a bucket image is 32 bytes, got {len(b)}")
        out.append(None if b is None else bytes(b)[:32])
    return out


def admit_many(users: Sequence[bytes], keys: Optional[Sequence[bytes]], now, start: bytes = b"$",
               max_tokens: int = 100, reset_interval: int = 1, stored=None, device=None) -> Admission:
    """The admission of n requests (users[i], keys[i], now[i]) in arrival order.
    keys None: no IsLegal step.  now: one int for the batch, or n non-decreasing
    ints (seconds).  start, max_tokens and reset_interval default to the
    reference's configuration (coreconf.go:40-45: InternalStart "$", 100 tokens,
    1 second).  stored: None (every bucket fresh), a dict user -> bucket, or one
    entry per request: what get(start ++ user) found live (a 32-byte Value or a
    TokenBucket), None where it found nothing or a tombstone; only the entry of
    a user's first legal request matters.  A stored bucket brings its own
    MaxTokens and ResetInterval."""
    import torch
    from .lsmtree import rank_device
    users = [bytes(u) for u in users]
    n = len(users)
    if keys is not None and len(keys) != n:
        raise ValueError(f"admit_many: {n} users and {len(keys)} keys")
    start = bytes(start)
    if not 1 <= len(start) <= 64:
        raise ValueError("admit_many: start is 1..64 bytes")
    validate_params(max_tokens, reset_interval)
    per_request = _stored_per_request(users, stored)
    if n == 0:
        return Admission(np.zeros(0, np.uint8), np.zeros((0, 32), np.uint8), np.zeros(0, np.int64),
                         np.zeros(0, np.uint64), np.zeros(0, bool))
    if np.ndim(now) == 0:
        ts, ts_all = None, int(now)
    else:
        ts, ts_all = np.ascontiguousarray(now, dtype=np.int64), 0
        if ts.shape != (n,):
            raise ValueError(f"admit_many: {ts.size} times for {n} requests")
    dev = torch.device("cuda", rank_device(device))
    ublob, uoff, ulen = pack_keys(users)
    d = {"d_users": up(dev, np.frombuffer(ublob, np.uint8)), "d_uoff": up(dev, uoff), "d_ulen": up(dev, ulen)}
    users_len = len(ublob)
    keys_len = 0
    if keys is not None:
        kblob, koff, klen = pack_keys(keys)
        keys_len = len(kblob)
        d.update(d_keys=up(dev, np.frombuffer(kblob, np.uint8)), d_koff=up(dev, koff), d_klen=up(dev, klen))
    if ts is not None:
        d["d_ts"] = up(dev, ts)
    if per_request is not None:
        live = [b is not None for b in per_request]
        boff = np.zeros(n, np.uint64)
        boff[1:] = np.cumsum(np.asarray(live[:-1], np.uint64) * np.uint64(32))
        blob = b"".join(b for b in per_request if b is not None) or bytes(32)
        d.update(d_buckets=up(dev, np.frombuffer(blob, np.uint8)), d_boff=up(dev, boff),
                 d_bstatus=up(dev, np.where(live, _lib.NKV_GET_LIVE, _lib.NKV_GET_ABSENT).astype(np.uint8)))
    outs = admit_dev(n, users_len=users_len, keys_len=keys_len, ts_all=ts_all, start=start, max_tokens=max_tokens,
                     reset_interval=reset_interval, device=device, **d)
    verdict, bucket, wait, group, last = (t.cpu().numpy() for t in outs)
    return Admission(verdict[:n].copy(), bucket[:32 * n].reshape(n, 32).copy(), wait[:8 * n].view(np.int64).copy(),
                     group[:8 * n].view(np.uint64).copy(), last[:n].astype(bool))
