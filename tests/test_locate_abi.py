"""The index-lookup entry points from plain C: include/nkv_merkle.h with them in
it still compiles as C99 -pedantic -Werror, the two symbols link, a null
context is refused by both, adding them did not bump the ABI version, and the
ctypes binding declares them with the header's argument counts, constants and
struct layout.  No device is needed."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "locate_abi_c99.c")


def test_locate_entry_points_from_c99(tmp_path):
    from nakevaleng_amd import _lib, build as b
    so = b.build(quiet=True)
    libdir = os.path.dirname(so)
    exe = os.path.join(str(tmp_path), "locate_abi_c99")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Werror", "-Wall", "-Wextra", "-O1",
                           "-I", os.path.join(ROOT, "include"), SRC, "-L", libdir, "-lnkvmerkle",
                           f"-Wl,-rpath,{libdir}", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    kv = dict(line.split(" ", 1) for line in out.stdout.strip().splitlines())
    assert kv["abi"] == "1"
    assert kv["symbols"] == "1"
    assert kv["null_ctx"] == "2 2"  # NKV_ERR_INVALID from both
    assert [int(x) for x in kv["constants"].split()] == [
        _lib.NKV_INDEX_BAD_HEADER, _lib.NKV_INDEX_BAD_SUMMARY_CHAIN, _lib.NKV_INDEX_BAD_INDEX_CHAIN,
        _lib.NKV_INDEX_BAD_LINK, _lib.NKV_INDEX_BAD_ORDER, _lib.NKV_INDEX_BAD_RANGE, _lib.NKV_GET_LOCATED,
        _lib.NKV_OPT_INDEX_OPEN_PATH, _lib.NKV_OPT_INDEX_OPEN_CHUNK]
    assert [int(x) for x in kv["constants"].split()] == [1, 2, 4, 8, 16, 32, 3, 24, 25]
    T = _lib.NkvIndexTable
    assert [int(x) for x in kv["struct"].split()] == [ctypes.sizeof(T), T.index_len.offset, T.ent_off.offset,
                                                      T.bits.offset, T.seed0.offset]
    assert _lib.lib().nkv_abi_version() == 1 == _lib.NKV_ABI_VERSION


def test_binding_declares_the_locate_entries():
    from nakevaleng_amd import _lib
    assert {"nkv_index_open_dev", "nkv_locate_dev"} <= set(_lib.SIGNATURES)
    assert len(_lib.SIGNATURES["nkv_index_open_dev"][1]) == 10
    assert len(_lib.SIGNATURES["nkv_locate_dev"][1]) == 14
    assert sorted(_lib.INDEX_VERDICTS) == [1, 2, 4, 8, 16, 32]


def test_python_entry_points_exist():
    from nakevaleng_amd import lsmtree, sstable
    for mod, names in ((sstable, ("open_index", "open_index_files", "IndexedTable")),
                       (lsmtree, ("locate_many", "get_many_on_disk", "read_located"))):
        for name in names:
            assert callable(getattr(mod, name))
