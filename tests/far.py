"""Layouts that put the values of one wave more than 4 GiB apart (host only:
numpy, no torch), shared by tests/test_gpu_far.py and tests/test_far_layout.py.

The leaf kernels address a wave's 64 values as 32-bit offsets from a
wave-uniform base where they can and take 64-bit addresses when the values lie
too far apart (the guards quoted at *_flip below, csrc/sha1_feed_dev.hpp).  A case
here is a COMPACT layout -- one small contiguous host array, what the oracle
hashes and what the near twin uploads -- plus ISLANDS that map ranges of it to
places gigabytes apart inside one big device allocation of ALLOC bytes.

Allocation rule.  Every value of every case lies inside that one allocation,
and the allocation reaches at least 2^32 + the longest value past the lowest
address of any wave whose values span 4 GiB (islands 0 and 1 end below
2^32 + 32 MiB; a wave that lies in island 2 alone is a near wave).  A 32-bit
offset that wrapped would therefore still land inside the allocation: a wrong
address reads wrong bytes, never unmapped memory.  tests/test_far_layout.py
checks it for every case.
"""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache
from typing import List, Sequence, Tuple

import numpy as np

G32 = 1 << 32
ALLOC = 9 << 30  # bytes of the one device buffer tests/test_gpu_far.py allocates
BASES = (0, G32 + (1 << 24), 2 * G32 + (1 << 24))  # device base of islands 0, 1, 2
RAGGED = (0, 1, 63, 64, 65, 200, 4050, 4096, 20000)  # the issue's ragged lengths
FILLER = 20  # a value of one compression and no full block: sorts behind every value with a full block


# ---------------------------------------------------------------------------
# where the guards flip

def pair_flip(nmax: int) -> Tuple[int, int]:
    """(last near, first far) distance between the 64-byte-aligned addresses
    (p & ~63) of the wave's lowest and highest value, sha1_blocks_pair:
        rel + 64ull * (uint64_t(nmax) + 1ull) <= 0xFFFFFFFFull
    rel is a multiple of 64, so the last near one is 2^32 - 64 (nmax + 2)."""
    return G32 - 64 * (nmax + 2), G32 - 64 * (nmax + 1)


def shift_flip(nmax: int) -> Tuple[int, int]:
    """The same for sha1_blocks_shift's LDS-DMA stage, over the segment starts
    sa = p - (p & 63):
        rel + 64ull * (uint64_t(nmax) + 1ull) <= 0xFFFFFFFFull"""
    return pair_flip(nmax)


def ring_vc_flip(nj: int) -> Tuple[int, int]:
    """(last near, first far) byte distance of a value of nj >= 1 full blocks
    from the wave base (the lowest address of a value with a full block),
    ring_vc_blocks:
        relk[k] = (nj ? aj - wb : 0ull) + 16u * dq;     dq = lane & 3
        lastk[k] = 64u * ((nj ? nj : wb_nfull) - 1u);
        near = relk[k] + lastk[k] + 16ull <= 0xFFFFFFFFull       for every role
    The role with dq = 3 adds 48, the last full block 64 (nj - 1), and the
    16-byte request has to end inside the buffer descriptor's 0xFFFFFFFF bytes."""
    last = 0xFFFFFFFF - 16 - 48 - 64 * (nj - 1)
    return last, last + 1


def strided_flip() -> dict:
    """The strided threshold (k_leaf MODE 0 under LOAD 11 with 64-byte aligned
    values): the smallest slack 64 k, k >= 2, for which 63 stride = 2^32 - 64 k
    has a stride that is a multiple of 64; then the block counts at which
    sha1_blocks_pair's guard (pair_flip: 63 stride + 64 (nmax + 1) <= 2^32 - 1)
    flips, and the first at which a 32-bit sum of the fallthrough's offsets
        off0 + k * kstep + 64u * b = 63 stride + 16 q + 64 b,  q <= 3, b <= nmax - 1
    passes 2^32."""
    k = next(k for k in range(2, 65) if (G32 // 64 - k) % 63 == 0)
    stride = (G32 - 64 * k) // 63
    span = 63 * stride
    near_nmax = max(m for m in range(1, 64) if span + 64 * (m + 1) <= 0xFFFFFFFF)
    wrap_nmax = next(m for m in range(1, 64) if span + 48 + 64 * (m - 1) >= G32)
    return {"stride": stride, "last_near_len": 64 * near_nmax + 63, "first_far_len": 64 * (near_nmax + 1),
            "wrap_len": 64 * wrap_nmax}


# ---------------------------------------------------------------------------
# compact layout -> far layout

def _up(x: int, a: int) -> int:
    return (x + a - 1) // a * a


def deal(lens: Sequence[int], mods=0, nisl: int = 3, align: int = 64):
    """Compact layout under the dealing rule: value i goes to island i % nisl
    (any 64 consecutive values then touch every island), at the next free place
    of that island whose offset is mods[i] modulo align.  Island k's values are
    compact range k.  Returns (compact offsets, [(start, end) of each range])."""
    n = len(lens)
    mods = np.broadcast_to(np.asarray(mods, np.int64), (n,))
    cur = [0] * nisl
    pos = np.zeros(n, np.int64)
    for i in range(n):
        k = i % nisl
        p = cur[k] + (int(mods[i]) - cur[k]) % align
        pos[i] = p
        cur[k] = p + int(lens[i])
    size = [_up(c, 128) + 128 for c in cur]  # no value touches its range's end
    start = np.concatenate([[0], np.cumsum(size)[:-1]]).astype(np.int64)
    off = pos + start[np.arange(n) % nisl]
    return off.astype(np.uint64), [(int(s), int(s + z)) for s, z in zip(start, size)]


def place(off_compact, lens, islands):
    """Map a compact layout to a far one.  islands = [(compact_start,
    compact_end, device_base)]: every value inside compact range k keeps its
    place relative to device_base[k].  Returns (device offsets, [(device_base,
    slice of the compact array) to upload])."""
    off = np.asarray(off_compact, np.uint64)
    lens = np.asarray(lens, np.uint64)
    out = np.zeros(off.size, np.uint64)
    done = np.zeros(off.size, bool)
    for cs, ce, db in islands:
        m = (off >= np.uint64(cs)) & (off + lens <= np.uint64(ce)) & ~done
        out[m] = off[m] - np.uint64(cs) + np.uint64(db)
        done |= m
    assert done.all(), "a value lies in no island"
    return out, [(int(db), slice(int(cs), int(ce))) for cs, ce, db in islands]


@dataclass
class Case:
    """Values (or whole records) at compact offsets `off`, `lens` bytes each."""
    name: str
    lens: np.ndarray
    off: np.ndarray  # compact
    islands: List[Tuple[int, int, int]]
    far: bool = True  # every 64 consecutive values in input order span more than 4 GiB
    guard: str = ""  # threshold cases: "pair" / "shift" / "ring_vc"
    near_side: bool = False  # threshold cases: the guard must hold (last near) or fail (first far)
    nfull_head: int = 0  # ring_vc cases: the first this-many values are the wave the guard is about

    @property
    def n(self) -> int:
        return int(self.lens.size)

    @property
    def compact_bytes(self) -> int:
        return max(e for _, e, _ in self.islands)

    def placed(self):
        return place(self.off, self.lens, self.islands)


def _case(name, lens, mods=0, nisl=3, align=64, bases=BASES, **kw) -> Case:
    lens = np.asarray(lens, np.uint64)
    off, ranges = deal(lens, mods, nisl, align)
    return Case(name, lens, off, [(s, e, bases[k]) for k, (s, e) in enumerate(ranges)], **kw)


def _mixed(n: int) -> np.ndarray:
    return (np.arange(n) * 13 + 5) % 64


def _threshold(name, lens, mods, dist, aligned64: bool, **kw) -> Case:
    """Two islands; value 0 (first of island 0) is the wave's lowest value,
    value `hi` (the last value with a full block in island 1) its highest, and
    island 1's base puts them exactly `dist` apart: between the addresses
    rounded down to 64 (pair, shift) or the addresses themselves (ring_vc)."""
    lens = np.asarray(lens, np.uint64)
    off, ranges = deal(lens, mods, 2)
    full = np.nonzero(lens >= 64)[0]
    hi = int(full[full % 2 == 1][-1])
    lo_pos = int(off[0]) - ranges[0][0]
    hi_pos = int(off[hi]) - ranges[1][0]
    if aligned64:
        lo_pos, hi_pos = lo_pos & ~63, hi_pos & ~63
    base1 = BASES[0] + lo_pos + dist - hi_pos
    assert base1 % 64 == 0, "island bases keep the values' offsets modulo 64"
    return Case(name, lens, off, [(ranges[0][0], ranges[0][1], BASES[0]), (ranges[1][0], ranges[1][1], base1)],
                far=False, **kw)


@lru_cache(maxsize=None)
def value_cases() -> Tuple[Case, ...]:
    """nkv_leaf_hash_dev / nkv_tree_from_values_dev."""
    out = []
    for n in (2, 64):
        # one group: the one wave is the whole batch whatever order the library picks
        out.append(_case(f"aligned-n{n}", [200] * n, 0))  # pair refused
        out.append(_case(f"shift46-n{n}", [200] * n, 46))  # shift's stage refused: register segments
        out.append(_case(f"mixed-n{n}", [200] * n, _mixed(n)))  # pair refused, unaligned sources
        out.append(_case(f"ragged-n{n}", [RAGGED[(i + i // 3) % len(RAGGED)] for i in range(n)], _mixed(n)))
        # full blocks in island 0 only: the far lanes' DMA roles re-read the wave base's value
        out.append(_case(f"far-no-block-n{n}", [200 if i % 3 == 0 else 30 for i in range(n)], _mixed(n)))
    # a batch of n <= 64 runs in input order through k_leaf; the work-queue
    # kernel (ring_vc_blocks) takes sorted batches of more than 64.  The sort is
    # by compression count, longest first, so 64 fillers behind 64 values with
    # at least two compressions leave those 64 as the queue's first group.
    fill = [FILLER] * 64
    rag = [RAGGED[(i + i // 3) % len(RAGGED)] for i in range(64)]
    out.append(_case("ragged-queue", [x if x >= 56 else 4050 for x in rag] + fill, _mixed(128), nfull_head=64))
    out.append(_case("far-no-block-queue", [200 if i % 3 == 0 else 63 for i in range(64)] + fill, _mixed(128),
                     nfull_head=64))
    # thresholds: two islands exactly at the last near / first far distance
    nmax = 3
    for side, near in (("near", True), ("far", False)):
        d = pair_flip(nmax)[0 if near else 1]
        out.append(_threshold(f"pair-{side}", [64 * nmax + 8] * 64, _mixed(64), d, True, guard="pair",
                              near_side=near))
        d = shift_flip(nmax)[0 if near else 1]
        out.append(_threshold(f"shift-{side}", [64 * nmax + 8] * 64, 46, d, True, guard="shift", near_side=near))
        d = ring_vc_flip(nmax)[0 if near else 1]
        mods = _mixed(128).copy()
        mods[63] = (int(mods[0]) + d) % 64
        out.append(_threshold(f"ring_vc-{side}", [64 * nmax + 7] * 64 + fill, mods, d, False, guard="ring_vc",
                              near_side=near, nfull_head=64))
    # ring_vc's clamped near form at its edge: a 64-byte value at the wave base,
    # one at the last near distance, one of 200 blocks between, the rest short.
    # Past block 0 the far value's rel + 64 c passes 2^32 while the wave is near.
    d = ring_vc_flip(1)[0]
    mods = _mixed(130).copy()
    mods[1] = (int(mods[0]) + d) % 64
    out.append(_threshold("ring_vc-near-wrap", [64, 64, 64 * 200] + [FILLER] * 127, mods, d, False, guard="ring_vc",
                          near_side=True, nfull_head=3))
    # breadth: 65 waves, above the auto gate's 4096, lengths at most 400 bytes
    rng = np.random.default_rng(0x66617231)
    out.append(_case("breadth-uniform", [400] * 4160, _mixed(4160)))
    out.append(_case("breadth-ragged", rng.integers(0, 401, 4160), rng.integers(0, 64, 4160)))
    return tuple(out)


# ---------------------------------------------------------------------------
# strided

S0 = (1 << 26) + (1 << 22)  # 68 MiB: 63 strides pass 2^32
STRIDED_LENS = (0, 63, 64, 200, 4050, 4096)
STRIDED_PLACES = ((0, S0), (0, S0 + 16), (0, S0 + 1), (46, S0), (46, S0 + 46))


@dataclass(frozen=True)
class Strided:
    name: str
    base: int  # offset of value 0 in the device buffer
    stride: int
    L: int
    n: int
    far: bool = True  # the full waves span more than 4 GiB
    loads: Tuple[int, ...] = (4, 11)

    def near_stride(self) -> int:
        """The compact twin's stride: the same residue modulo 64, just past the value."""
        return _up(self.L, 64) + 64 + self.stride % 64


@lru_cache(maxsize=None)
def strided_cases() -> Tuple[Strided, ...]:
    out = [Strided(f"b{b}-s0+{s - S0}-len{L}", b, s, L, 130) for b, s in STRIDED_PLACES for L in STRIDED_LENS]
    t = strided_flip()
    for what in ("last_near_len", "first_far_len", "wrap_len"):
        out.append(Strided(f"threshold-{what}-{t[what]}", 64, t["stride"], t[what], 64, far=False, loads=(11,)))
    out.append(Strided("stride-2^32+64", 0, G32 + 64, 200, 3))
    out.append(Strided("stride-2^32+65", 0, G32 + 65, 200, 3))
    return tuple(out)


# ---------------------------------------------------------------------------
# records: whole records dealt to the three islands (the record calls do not
# require contiguous records; d_stream is the buffer, stream_len its length)

@dataclass
class Records:
    name: str
    ks: np.ndarray
    vs: np.ndarray
    layout: Case  # lens = record sizes

    @property
    def n(self) -> int:
        return int(self.ks.size)


def _records(name, ks, vs, mods, align=64) -> Records:
    ks, vs = np.asarray(ks, np.uint64), np.asarray(vs, np.uint64)
    return Records(name, ks, vs, _case(name, 30 + ks + vs, mods, 3, align))


@lru_cache(maxsize=None)
def record_cases() -> Tuple[Records, ...]:
    out = []
    for n in (64, 4160):
        rng = np.random.default_rng(0x66617232 + n)
        # records of one size start where a packed table would put them modulo
        # 64 (256) or 128 (4096: the values' segments start lines, LINES route)
        out.append(_records(f"rec256-n{n}", [16] * n, [256 - 46] * n, 0))
        out.append(_records(f"rec4096-n{n}", [16] * n, [4096 - 46] * n, 0, align=128))
        out.append(_records(f"ragged-n{n}", rng.integers(0, 41, n), rng.integers(0, 1501, n),
                            rng.integers(0, 64, n)))
    return tuple(out)


# ---------------------------------------------------------------------------
# a Data table longer than 4 GiB (nkv_merge_records_dev)

GIANT_VALUE = G32 + 5
GIANT_RUN0_AT = 0  # run 0: contiguous, a little over 4 GiB
GIANT_RUN1_AT = G32 + (1 << 20)
GIANT_OUT_AT = G32 + (2 << 20)
GIANT_SMALL = 1 << 16  # upper bound of everything in either run but the giant value
GIANT_OUT_CAP = GIANT_VALUE + 2 * GIANT_SMALL


def giant_ranges():
    """[(start, end)] of run 0, run 1 and d_out with its guard band."""
    return [(GIANT_RUN0_AT, GIANT_RUN0_AT + GIANT_VALUE + GIANT_SMALL),
            (GIANT_RUN1_AT, GIANT_RUN1_AT + GIANT_SMALL),
            (GIANT_OUT_AT, GIANT_OUT_AT + GIANT_OUT_CAP + 4096)]
