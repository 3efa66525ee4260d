"""GPU: malformed Data tables through every device entry that reads records.

Eight malformations of a table of 3 to 8 records (8-byte keys, 4-byte values)
are fed to the merge, the flush, Index/Summary, lookup + lookup_values, and
the record forms of the bloom and CRC entries.  What each entry answers is
pinned per (entry, case): its status codes, whether its outputs were left
untouched, and a checksum of everything it wrote.  Some entries accept some
cases -- Index never looks at ValueSize, CRC does not ask that a record ends
where the next starts -- and that is pinned as it is, not judged.

EXPECT was recorded on the commit before csrc/record_dev.hpp unified the
bounds checks of these entries; the entries must keep refusing exactly what
they refused then.

Every table lies in the middle of a larger allocation (tests/guarded.py) and
every case makes the library answer with a status, never follow the bad field:
each check compares against the room left in the stream before anything is
read through an offset or a size.
"""
import ctypes
import struct
import zlib

import numpy as np
import pytest

from nakevaleng_amd import record
from tests.guarded import guarded

pytestmark = pytest.mark.gpu

FILL = 0xA5
HDR = 30
U64 = 2**64

CASES = {
    1: "first offset not 0",
    2: "an offset of L - 29",
    3: "an offset of 2^64 - 16",
    4: "KeySize = room + 1",
    5: "ValueSize = room - ks + 1",
    6: "KeySize + ValueSize wraps",
    7: "one-byte gap between two records",
    8: "two records overlap by one byte",
}
COUNT = {1: 3, 2: 4, 3: 5, 4: 6, 5: 7, 6: 8, 7: 5, 8: 6}
ENTRIES = ["merge", "sort", "index", "lookup", "bloom", "crc"]


def _rec(i, odd=0):
    return record.New(b"key%05d" % (10 * i + odd), b"v%03d" % i, timestamp=i + 1)


def table(case):
    """(stream bytes, offsets) of the malformed table of `case`."""
    n = COUNT[case]
    parts = [_rec(i).ToBytes() for i in range(n)]
    assert all(len(p) == HDR + 12 for p in parts)
    j = n // 2  # the record that carries the bad field
    if case == 1:
        parts.insert(0, b"\x00")
    elif case == 7:
        parts.insert(j, b"\x00")
    elif case == 8:
        parts[j - 1] = parts[j - 1][:-1]
    off, at = [], 0
    for p in parts:
        if len(p) > 1:
            off.append(at)
        at += len(p)
    buf = bytearray(b"".join(parts))
    L = len(buf)
    room = L - off[j] - HDR
    if case == 2:
        off[n - 1] = L - 29
    elif case == 3:
        off[j] = U64 - 16
    elif case == 4:
        struct.pack_into("<Q", buf, off[j] + 14, room + 1)
    elif case == 5:
        struct.pack_into("<Q", buf, off[j] + 22, room - 8 + 1)
    elif case == 6:
        struct.pack_into("<Q", buf, off[j] + 22, U64 - 4)
    assert len(off) == n
    return bytes(buf), np.asarray(off, dtype=np.uint64)


def _digest(*outs):
    return zlib.crc32(b"".join(np.ascontiguousarray(o).tobytes() for o in outs)) & 0xFFFFFFFF


def observe(nkv, entry, case):
    """Run `entry` over the table of `case`: (status codes, outputs untouched,
    checksum of the outputs).  Inputs and guard bytes are checked here."""
    import torch
    _lib, ctx = nkv
    lib = _lib.lib()
    data, off = table(case)
    n, L = len(off), len(data)
    p_s, s_check = guarded(L, 1, fill=0x5A, init=data)
    p_o, o_check = guarded(8 * n, 8, fill=0x5A, init=off)
    outs = []

    def out(nbytes, at):
        p, check = guarded(nbytes, at, fill=FILL)
        outs.append(check)
        return p

    rcs, words = [], []
    if entry in ("merge", "sort"):
        good, goff = record.data_table([_rec(i, odd=5) for i in range(3)])
        goff = np.concatenate([[0], np.cumsum(goff)[:-1]]).astype(np.uint64)
        p_g, g_check = guarded(len(good), 3, fill=0x5A, init=good)
        p_go, go_check = guarded(8 * 3, 8, fill=0x5A, init=goff)
        total = L + (len(good) if entry == "merge" else 0)
        rows = n + (3 if entry == "merge" else 0)
        p_out, p_off, p_src = out(total, 1), out(8 * rows, 8), out(8 * rows, 8)
        n_out, out_len = ctypes.c_uint64(7), ctypes.c_uint64(7)
        if entry == "merge":
            runs = (_lib.NkvRun * 2)(_lib.NkvRun(p_s, L, p_o, n), _lib.NkvRun(p_g, len(good), p_go, 3))
            rcs.append(lib.nkv_merge_records_dev(ctx.h, runs, 2, p_out, total, p_off, p_src, ctypes.byref(n_out),
                                                 ctypes.byref(out_len)))
        else:
            rcs.append(lib.nkv_sort_records_dev(ctx.h, p_s, L, p_o, n, p_out, total, p_off, p_src,
                                                ctypes.byref(n_out), ctypes.byref(out_len)))
        words = [n_out.value, out_len.value]
        torch.cuda.synchronize()
        assert g_check().tobytes() == good and go_check().tobytes() == goff.tobytes()
    elif entry == "index":
        p_i, p_m = out(1024, 1), out(1024, 3)
        ilen, slen = ctypes.c_uint64(7), ctypes.c_uint64(7)
        rcs.append(lib.nkv_index_summary_dev(ctx.h, p_s, L, p_o, n, 2, p_i, 1024, p_m, 1024, ctypes.byref(ilen),
                                             ctypes.byref(slen)))
        words = [ilen.value, slen.value]
    elif entry == "lookup":
        keys = [_rec(i).Key for i in range(n)] + [b"key00001", b"a", b"z"]
        q = len(keys)
        koff = np.arange(q, dtype=np.uint64) * 8
        klen = np.asarray([len(k) for k in keys], dtype=np.uint64)
        p_k, k_check = guarded(8 * q, 5, fill=0x5A, init=b"".join(k.ljust(8, b"\x00") for k in keys))
        p_ko, _ko = guarded(8 * q, 8, fill=0x5A, init=koff)
        p_kl, _kl = guarded(8 * q, 8, fill=0x5A, init=klen)
        p_hit, p_st, p_sg = out(8 * q, 8), out(q, 1), out(q, 1)
        tab = (_lib.NkvLookupTable * 1)(_lib.NkvLookupTable(p_s, L, p_o, n, None, 0, 0, 0))
        rcs.append(lib.nkv_lookup_dev(ctx.h, tab, 1, p_k, p_ko, p_kl, q, p_hit, p_st, p_sg, None))
        torch.cuda.synchronize()
        p_v, p_vo = out(64 * q, 1), out(8 * (q + 1), 8)
        vlen = ctypes.c_uint64(7)
        rcs.append(lib.nkv_lookup_values_dev(ctx.h, tab, 1, p_hit, p_st, q, p_v, 64 * q, p_vo, ctypes.byref(vlen)))
        words = [vlen.value]
        torch.cuda.synchronize()
        k_check()
    elif entry == "bloom":
        p_b = out(32, 4)
        rcs.append(lib.nkv_bloom_insert_records_dev(ctx.h, p_s, L, p_o, n, 256, 3, 0, p_b))
    elif entry == "crc":
        p_c, p_t = out(4 * n, 4), out(24, 8)
        rcs.append(lib.nkv_record_crc_dev(ctx.h, p_s, L, p_o, n, p_c, p_t))
    torch.cuda.synchronize()
    assert s_check().tobytes() == data and o_check().tobytes() == off.tobytes()
    got = [check() for check in outs]  # every guard byte intact
    untouched = all((g == FILL).all() for g in got)
    return tuple(rcs), untouched, _digest(np.asarray(words, dtype=np.uint64), *got)


# (entry, case) -> (status codes, outputs untouched, checksum of the outputs)
EXPECT = {
    ('merge', 1): ((2,), True, 431595822),
    ('merge', 2): ((2,), True, 960957306),
    ('merge', 3): ((2,), True, 3572007699),
    ('merge', 4): ((2,), True, 3575115571),
    ('merge', 5): ((2,), True, 576652346),
    ('merge', 6): ((2,), True, 1384664621),
    ('merge', 7): ((2,), True, 4040430007),
    ('merge', 8): ((2,), True, 2026153889),
    ('sort', 1): ((2,), True, 2391529387),
    ('sort', 2): ((2,), True, 3181602087),
    ('sort', 3): ((2,), True, 1858942511),
    ('sort', 4): ((2,), True, 3674025749),
    ('sort', 5): ((2,), True, 960957306),
    ('sort', 6): ((2,), True, 3572007699),
    ('sort', 7): ((2,), True, 3741403269),
    ('sort', 8): ((2,), True, 2466100712),
    ('index', 1): ((0,), False, 3391674487),
    ('index', 2): ((2,), True, 3416489919),
    ('index', 3): ((2,), True, 3416489919),
    ('index', 4): ((2,), True, 3416489919),
    ('index', 5): ((0,), False, 500003555),
    ('index', 6): ((0,), False, 1099676560),
    ('index', 7): ((0,), False, 4010513859),
    ('index', 8): ((0,), False, 3369005863),
    ('lookup', 1): ((0, 0), False, 4262706648),
    ('lookup', 2): ((2, 0), False, 3017191137),
    ('lookup', 3): ((2, 0), False, 2017265595),
    ('lookup', 4): ((2, 0), False, 631108011),
    ('lookup', 5): ((0, 2), False, 1227560667),
    ('lookup', 6): ((0, 2), False, 2788718037),
    ('lookup', 7): ((0, 0), False, 1067809652),
    ('lookup', 8): ((0, 0), False, 181087754),
    ('bloom', 1): ((0,), False, 3444673485),
    ('bloom', 2): ((2,), False, 3444673485),
    ('bloom', 3): ((2,), False, 3043738671),
    ('bloom', 4): ((2,), False, 1628045728),
    ('bloom', 5): ((0,), False, 1617702918),
    ('bloom', 6): ((0,), False, 1167997296),
    ('bloom', 7): ((0,), False, 3182976998),
    ('bloom', 8): ((0,), False, 4288501915),
    ('crc', 1): ((0,), False, 3917212967),
    ('crc', 2): ((0,), False, 271363317),
    ('crc', 3): ((0,), False, 4157532208),
    ('crc', 4): ((0,), False, 4277375615),
    ('crc', 5): ((0,), False, 1857542242),
    ('crc', 6): ((0,), False, 1153680517),
    ('crc', 7): ((0,), False, 3218768216),
    ('crc', 8): ((0,), False, 3645642937),
}


@pytest.mark.parametrize("case", sorted(CASES), ids=[f"{c}-{CASES[c].replace(' ', '_')}" for c in sorted(CASES)])
@pytest.mark.parametrize("entry", ENTRIES)
def test_malformed(nkv, entry, case):
    got = observe(nkv, entry, case)
    print(f"({entry!r}, {case}): {got!r},")
    assert got == EXPECT[(entry, case)]

