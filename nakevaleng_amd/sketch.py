"""ds/hll- and ds/cmsketch-shaped mirrors over the device sketches (csrc/sketch.hip).

Reference: ds/hll/hll.go and ds/cmsketch/cmsketch.go, the two typed values of
the reference's engine (WrapperEngine.PutHLL / PutCMS, wrappereng.go:57-83).

  hll.New(precision)          New(precision) -> HLL (fields M, P, Reg)
  (*HLL).Add / Estimate       HLL.Add / AddMany / Estimate / EstimateStandard
  cmsketch.New(eps, delta)    NewCMS(epsilon, delta, seed) -> CountMinSketch
                              (fields M, K, HashSeeds, Contents)
  Insert / Query              Insert / InsertMany / Query / QueryMany

Adds and inserts are deferred and hashed in one device batch when the sketch is
next read (Reg, Contents, Estimate, Query, EncodeToDict), the batching the
filter mirror does for Insert.  The gob encodings (EncodeToBytes /
DecodeFromBytes) are host serialization and out of scope; EncodeToDict gives
the encoded fields.

Estimate() is hll.go:75-92 taken literally, quirk included: its sum adds
math.Pow(float64(-val), 2.0) with val a uint8, so -val wraps modulo 256 and the
term is (256 - val)^2, not 2^-val.  In effect the reference's estimate is
linear counting (M ln(M / empty)) while empty registers remain and a
meaningless small number after that (0.0118 for 20,000 keys at P = 10), NaN for
an empty HLL.  EstimateStandard() sums 2^-Reg with the same alpha and
corrections and is the usable one.

Deviations: cmsketch.New accepts epsilon = 0, delta = 0 and delta = 1, which
give +Inf conversions or K = 0; NewCMS raises unless 0 < epsilon <= 1 and
0 < delta < 1.  The reference draws the first seed from the clock; here `seed`
may be given.
"""
from __future__ import annotations

import ctypes
import time
from typing import List, Optional, Sequence

import numpy as np

from nakevaleng_amd import _lib
from nakevaleng_amd.bloomfilter import _pack

HLL_MIN_PRECISION = _lib.NKV_HLL_MIN_PRECISION
HLL_MAX_PRECISION = _lib.NKV_HLL_MAX_PRECISION


class HLLError(ValueError):
    pass


class CMSError(ValueError):
    pass


def _vp(a: np.ndarray):
    return a.ctypes.data_as(ctypes.c_void_p)


class HLL:
    def __init__(self, M: int, P: int, Reg: Optional[bytes] = None, ctx=None):
        if not HLL_MIN_PRECISION <= P <= HLL_MAX_PRECISION or M != 1 << P:
            raise HLLError(f"an HLL of precision {P} holds {1 << P if 0 <= P < 64 else '?'} registers, not {M}")
        self.M, self.P = int(M), int(P)
        self._reg = np.frombuffer(bytes(Reg), np.uint8).copy() if Reg is not None else np.zeros(self.M, np.uint8)
        if self._reg.size != self.M:
            raise HLLError(f"Reg holds {self._reg.size} registers, M is {self.M}")
        self._pending: List[bytes] = []
        self._ctx = ctx

    def _flush(self) -> None:
        if not self._pending:
            return
        ctx = self._ctx or _lib.default_context()
        data, off, lens = _pack(self._pending)
        _lib.check(_lib.lib().nkv_hll_add(ctx.h, _vp(data), _vp(off), _vp(lens), len(self._pending), self.P,
                                          _vp(self._reg)), "HLL.Add")
        self._pending.clear()

    def Add(self, data: bytes) -> None:  # hll.go:43-62
        self._pending.append(bytes(data))

    def AddMany(self, elements: Sequence[bytes]) -> None:
        self._pending.extend(bytes(e) for e in elements)

    @property
    def Reg(self) -> bytes:
        self._flush()
        return self._reg.tobytes()

    def _estimate(self, mode: int) -> float:
        self._flush()
        out = ctypes.c_double(0.0)
        _lib.check(_lib.lib().nkv_hll_estimate(_vp(self._reg), self.P, mode, ctypes.byref(out)), "HLL.Estimate")
        return out.value

    def Estimate(self) -> float:
        """(*HLL).Estimate, hll.go:75-92, literally: linear counting while empty
        registers remain, a meaningless small number after that, NaN when empty
        (the module docstring says why).  Use EstimateStandard() for a count."""
        return self._estimate(_lib.NKV_HLL_ESTIMATE_REFERENCE)

    def EstimateStandard(self) -> float:
        """The HyperLogLog estimate the reference meant: alpha M^2 / sum of
        2^-Reg, with the reference's alpha and its two range corrections."""
        return self._estimate(_lib.NKV_HLL_ESTIMATE_STANDARD)

    def EncodeToDict(self) -> dict:
        return {"M": self.M, "P": self.P, "Reg": self.Reg}


def New(precision: int, ctx=None) -> HLL:
    """hll.New (hll.go:30-40)."""
    if precision < HLL_MIN_PRECISION or precision > HLL_MAX_PRECISION:
        raise HLLError(f"precision must be between {HLL_MIN_PRECISION} and {HLL_MAX_PRECISION}, "
                       f"but {precision} was given")
    return HLL(1 << precision, precision, ctx=ctx)


def cms_params(epsilon: float, delta: float):
    """(M, K) as calculateM / calculateK (cmsketch.go:18-24)."""
    m, k = ctypes.c_uint32(0), ctypes.c_uint32(0)
    rc = _lib.lib().nkv_cms_params(epsilon, delta, ctypes.byref(m), ctypes.byref(k))
    if rc == _lib.NKV_ERR_INVALID:
        raise CMSError(f"epsilon must lie in (0, 1] and delta in (0, 1), but {epsilon:f} and {delta:f} were given")
    _lib.check(rc)
    return m.value, k.value


class CountMinSketch:
    def __init__(self, M: int, K: int, HashSeeds: Sequence[int], Contents=None, ctx=None):
        self.M, self.K, self.HashSeeds = int(M), int(K), [int(s) for s in HashSeeds]
        if self.M < 1 or self.K < 1 or self.M * self.K > 2**31 - 1 or len(self.HashSeeds) != self.K:
            raise CMSError(f"a Count-Min Sketch needs M >= 1, K >= 1, K M <= 2^31 - 1 and K seeds (M = {M}, K = {K})")
        if any(s != (self.HashSeeds[0] + j) & 0xFFFFFFFF for j, s in enumerate(self.HashSeeds)):
            raise CMSError("HashSeeds must be consecutive (createHashFunctions, cmsketch.go:28-38)")
        if Contents is None:
            self._table = np.zeros((self.K, self.M), np.uint32)
        else:
            self._table = np.ascontiguousarray(Contents, dtype=np.uint32).reshape(self.K, self.M).copy()
        self._pending: List[bytes] = []
        self._ctx = ctx

    def _flush(self) -> None:
        if not self._pending:
            return
        ctx = self._ctx or _lib.default_context()
        data, off, lens = _pack(self._pending)
        _lib.check(_lib.lib().nkv_cms_insert(ctx.h, _vp(data), _vp(off), _vp(lens), len(self._pending), self.M,
                                             self.K, self.HashSeeds[0], _vp(self._table)), "CountMinSketch.Insert")
        self._pending.clear()

    def Insert(self, element: bytes) -> None:  # cmsketch.go:76-87
        self._pending.append(bytes(element))

    def InsertMany(self, elements: Sequence[bytes]) -> None:
        self._pending.extend(bytes(e) for e in elements)

    @property
    def Contents(self) -> np.ndarray:
        """The K x M table of uint32 counters (a copy)."""
        self._flush()
        return self._table.copy()

    def QueryMany(self, elements: Sequence[bytes]) -> np.ndarray:
        """Query (cmsketch.go:91-111) for a batch: the minimum of each element's K counters."""
        self._flush()
        out = np.zeros(len(elements), np.uint32)
        if len(elements) == 0:
            return out
        ctx = self._ctx or _lib.default_context()
        data, off, lens = _pack([bytes(e) for e in elements])
        _lib.check(_lib.lib().nkv_cms_query(ctx.h, _vp(data), _vp(off), _vp(lens), len(elements), self.M, self.K,
                                            self.HashSeeds[0], _vp(self._table), _vp(out)), "CountMinSketch.Query")
        return out

    def Query(self, element: bytes) -> int:
        return int(self.QueryMany([element])[0])

    def EncodeToDict(self) -> dict:
        return {"M": self.M, "K": self.K, "HashSeeds": list(self.HashSeeds), "Contents": self.Contents.tolist()}


def NewCMS(epsilon: float, delta: float, seed: Optional[int] = None, ctx=None) -> CountMinSketch:
    """cmsketch.New (cmsketch.go:53-73); seed defaults to uint(time.Now().Unix())
    like createHashFunctions."""
    if epsilon < 0.0 or epsilon > 1.0:
        raise CMSError(f"epsilon must be between (0, 1), but {epsilon:f} was given")
    if delta < 0.0 or delta > 1.0:
        raise CMSError(f"delta must be between (0, 1), but {delta:f} was given")
    m, k = cms_params(epsilon, delta)
    t = (int(time.time()) if seed is None else seed) & 0xFFFFFFFF
    return CountMinSketch(m, k, [(t + i) & 0xFFFFFFFF for i in range(k)], ctx=ctx)
