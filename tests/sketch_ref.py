"""Literal Python restatement of the reference's two sketches, over
oracle.murmur3_32 (spaolacci/murmur3 Sum32, restated in oracle/bloom_oracle.c).

  ds/hll/hll.go            HLLRef: Add (:43-62), emptyCount (:64-72), Estimate
                           (:75-92), plus EstimateStandard (the sum of 2^-Reg
                           with the same alpha and corrections)
  ds/cmsketch/cmsketch.go  calculateM / calculateK (:18-24), CMSRef: Insert
                           (:76-87), Query (:91-111)

Go's float semantics are kept where Python's differ: x / 0.0 is +Inf and the
logarithm of a negative number is NaN, neither raises.

The *_many functions are the same updates over a whole batch with numpy
(murmur3_32_many hashes ragged keys grouped by length); tests/test_sketch_ref.py
holds them to the per-key classes, and the GPU tests use them for batches that
one ctypes call per key would make slow.
"""
from __future__ import annotations

import math

import numpy as np

from oracle import oracle_c

HLL_MIN_PRECISION = 4
HLL_MAX_PRECISION = 16


def _div(a: float, b: float) -> float:
    """Go's float64 a / b."""
    if b == 0.0:
        return math.nan if a == 0.0 or math.isnan(a) else math.copysign(math.inf, a)
    return a / b


def _log(x: float) -> float:
    """Go's math.Log."""
    if math.isnan(x) or x < 0.0:
        return math.nan
    if x == 0.0:
        return -math.inf
    return math.log(x)


def trailing_zeros32(x: int) -> int:
    """math/bits.TrailingZeros32: 32 for x == 0."""
    return 32 if x == 0 else (x & -x).bit_length() - 1


class HLLRef:
    def __init__(self, precision: int):  # hll.go:30-40
        if precision < HLL_MIN_PRECISION or precision > HLL_MAX_PRECISION:
            raise ValueError(f"precision must be between {HLL_MIN_PRECISION} and {HLL_MAX_PRECISION}, "
                             f"but {precision} was given")
        self.M = int(math.pow(2, float(precision)))
        self.P = precision
        self.Reg = [0] * self.M

    def Add(self, data: bytes) -> None:  # hll.go:43-62
        i = oracle_c.murmur3_32(data, 0)
        idx = i >> (32 - self.P)
        val = (1 + trailing_zeros32(i)) & 0xFF  # uint8(...)
        if self.Reg[idx] < val:
            self.Reg[idx] = val

    def emptyCount(self) -> int:  # hll.go:64-72
        return sum(1 for val in self.Reg if val == 0)

    def _estimate(self, term) -> float:
        total = 0.0
        for val in self.Reg:
            total = total + term(val)
        alpha = 0.7213 / (1.0 + 1.079 / float(self.M))
        estimation = _div(alpha * math.pow(float(self.M), 2.0), total)
        empty = self.emptyCount()
        if estimation < 2.5 * float(self.M):  # small range correction
            if empty > 0:
                estimation = float(self.M) * _log(float(self.M) / float(empty))
        elif estimation > math.pow(2.0, 32.0) / 30.0:  # large range correction
            estimation = -math.pow(2.0, 32.0) * _log(1.0 - estimation / math.pow(2.0, 32.0))
        return estimation

    def Estimate(self) -> float:
        """hll.go:75-92: val is a uint8, so float64(-val) is float64((256 - val) % 256)."""
        return self._estimate(lambda val: math.pow(float((-val) & 0xFF), 2.0))

    def EstimateStandard(self) -> float:
        return self._estimate(lambda val: math.pow(2.0, -float(val)))


def calculateM(epsilon: float) -> int:  # cmsketch.go:18-20
    return int(math.ceil(math.e / epsilon))


def calculateK(delta: float) -> int:  # cmsketch.go:22-24
    return int(math.ceil(math.log(1 / delta)))


def cms_new_accepted(epsilon: float, delta: float) -> bool:
    """The arguments nkv_cms_params accepts (the documented deviation: the
    reference also takes epsilon = 0, delta = 0 and delta = 1)."""
    return 0.0 < epsilon <= 1.0 and 0.0 < delta < 1.0 and calculateM(epsilon) <= 2**32 - 1


class CMSRef:
    def __init__(self, M: int, K: int, seed0: int):
        self.M, self.K = M, K
        self.HashSeeds = [(seed0 + i) & 0xFFFFFFFF for i in range(K)]  # cmsketch.go:28-38
        self.Contents = [[0] * M for _ in range(K)]

    def Insert(self, element: bytes) -> None:  # cmsketch.go:76-87
        for i, seed in enumerate(self.HashSeeds):
            index = oracle_c.murmur3_32(element, seed) % (self.M & 0xFFFFFFFF)
            self.Contents[i][index] = (self.Contents[i][index] + 1) & 0xFFFFFFFF

    def Query(self, element: bytes) -> int:  # cmsketch.go:91-111
        lo = 0
        for i, seed in enumerate(self.HashSeeds):
            index = oracle_c.murmur3_32(element, seed) % (self.M & 0xFFFFFFFF)
            tmp = self.Contents[i][index]
            if i == 0:
                lo = tmp
            elif tmp < lo:
                lo = tmp
        return lo


# ---------------------------------------------------------------------------
# the same over batches

def _rotl(x: np.ndarray, r: int) -> np.ndarray:
    return (x << np.uint32(r)) | (x >> np.uint32(32 - r))


def murmur3_32_many(data: np.ndarray, off: np.ndarray, ln: np.ndarray, seed: int) -> np.ndarray:
    """MurmurHash3_x86_32(data[off[i] : off[i] + ln[i]], seed) for every i."""
    data = np.ascontiguousarray(data, np.uint8)
    off, ln = np.asarray(off, np.int64), np.asarray(ln, np.int64)
    out = np.empty(ln.size, np.uint32)
    c1, c2 = np.uint32(0xcc9e2d51), np.uint32(0x1b873593)
    for L in np.unique(ln):
        L = int(L)
        sel = np.flatnonzero(ln == L)
        kb = data[off[sel][:, None] + np.arange(L, dtype=np.int64)[None, :]].astype(np.uint32)
        h = np.full(sel.size, seed & 0xFFFFFFFF, np.uint32)
        nb = L // 4
        for b in range(nb):
            q = kb[:, 4 * b:4 * b + 4]
            k = q[:, 0] | (q[:, 1] << np.uint32(8)) | (q[:, 2] << np.uint32(16)) | (q[:, 3] << np.uint32(24))
            k = _rotl(k * c1, 15) * c2
            h = _rotl(h ^ k, 13) * np.uint32(5) + np.uint32(0xe6546b64)
        if L & 3:
            k = np.zeros(sel.size, np.uint32)
            for t in range(L & 3):
                k |= kb[:, 4 * nb + t] << np.uint32(8 * t)
            h = h ^ (_rotl(k * c1, 15) * c2)
        h = h ^ np.uint32(L & 0xFFFFFFFF)
        h ^= h >> np.uint32(16)
        h = h * np.uint32(0x85ebca6b)
        h ^= h >> np.uint32(13)
        h = h * np.uint32(0xc2b2ae35)
        h ^= h >> np.uint32(16)
        out[sel] = h
    return out


def hll_add_many(reg, data, off, ln, P: int) -> np.ndarray:
    """Reg after Add of every key, starting from `reg` (2^P bytes; not modified)."""
    reg = np.array(reg, np.uint8).reshape(-1).copy()
    assert reg.size == 1 << P
    if len(ln) == 0:
        return reg
    h = murmur3_32_many(data, off, ln, 0)
    low = (h & (~h + np.uint32(1))).astype(np.float64)  # the lowest set bit: a power of two, exact
    tz = np.where(h == 0, 32, np.log2(np.where(h == 0, 1.0, low))).astype(np.int64)
    np.maximum.at(reg, (h >> np.uint32(32 - P)).astype(np.int64), (1 + tz).astype(np.uint8))
    return reg


def cms_indices(data, off, ln, M: int, K: int, seed0: int) -> np.ndarray:
    """(K, n) counter index of every key in every row."""
    return np.stack([murmur3_32_many(data, off, ln, seed0 + i) % np.uint32(M) for i in range(K)]) if len(ln) \
        else np.zeros((K, 0), np.uint32)


def cms_insert_many(table, data, off, ln, seed0: int, idx=None) -> np.ndarray:
    """Contents (K x M uint32) after Insert of every key, starting from `table`
    (not modified); idx: cms_indices of the same arguments, when already made."""
    table = np.array(table, np.uint32).copy()
    K, M = table.shape
    if idx is None:
        idx = cms_indices(data, off, ln, M, K, seed0)
    for i in range(K):
        table[i] += np.bincount(idx[i].astype(np.int64), minlength=M).astype(np.uint32)  # wraps at 2^32
    return table


def cms_query_many(table, data, off, ln, seed0: int, idx=None) -> np.ndarray:
    table = np.asarray(table, np.uint32)
    K, M = table.shape
    if idx is None:
        idx = cms_indices(data, off, ln, M, K, seed0)
    return np.min(np.stack([table[i][idx[i].astype(np.int64)] for i in range(K)]), axis=0).astype(np.uint32) \
        if len(ln) else np.zeros(0, np.uint32)
