"""The Index / Summary entry points from plain C: include/nkv_merkle.h with them
in it still compiles as C99 -pedantic -Werror, the three symbols link, a null
context is refused, adding them did not bump the ABI version, and
nkv_summary_entries (pure host arithmetic) equals the closed form of
tests/sstable_ref.py.  No device is needed."""
import os
import subprocess

from tests import sstable_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "index_abi_c99.c")

PAIRS = [(n, page) for n in (0, 1, 2, 3, 4, 5, 7, 64, 65, 100, 4097) for page in (1, 2, 3, 4, 64, 65, 1000)]


def test_index_entry_points_from_c99(tmp_path):
    from nakevaleng_amd import _lib, build as b
    so = b.build(quiet=True)
    libdir = os.path.dirname(so)
    exe = os.path.join(str(tmp_path), "index_abi_c99")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Werror", "-Wall", "-Wextra", "-O1",
                           "-I", os.path.join(ROOT, "include"), SRC, "-L", libdir, "-lnkvmerkle",
                           f"-Wl,-rpath,{libdir}", "-o", exe])
    args = [str(x) for pair in PAIRS for x in pair]
    out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    kv = dict(line.split(" ", 1) for line in out.stdout.strip().splitlines())
    assert kv["abi"] == "1"
    assert kv["symbols"] == "1"
    assert kv["null_ctx"] == "2 2"  # NKV_ERR_INVALID from both
    assert [int(x) for x in kv["entries"].split()] == [ref.summary_entries(n, page) for n, page in PAIRS]
    assert _lib.lib().nkv_abi_version() == 1 == _lib.NKV_ABI_VERSION


def test_binding_declares_the_index_entries():
    from nakevaleng_amd import _lib
    assert {"nkv_summary_entries", "nkv_index_summary_dev", "nkv_index_summary_from_records"} <= set(_lib.SIGNATURES)
    assert len(_lib.SIGNATURES["nkv_index_summary_dev"][1]) == 12
    assert len(_lib.SIGNATURES["nkv_index_summary_from_records"][1]) == 12
    assert _lib.INDEX_WRITE_TILE == 16384


def test_summary_entries_matches_the_closed_form():
    from nakevaleng_amd import _lib, build as b
    b.build(quiet=True)
    L = _lib.lib()
    for n in list(range(0, 70)) + [100, 255, 256, 257, 4097, 65537, 2**31 - 1]:
        for page in (1, 2, 3, 4, 5, 63, 64, 65, 1000, 4096, n + 5, 2**40):
            assert L.nkv_summary_entries(n, page) == ref.summary_entries(n, page), (n, page)
    # page 0: never divided by for n <= 1, refused (0 entries) from two records on
    assert [L.nkv_summary_entries(n, 0) for n in (0, 1, 2, 100)] == [0, 1, 0, 0]
