"""The point-lookup entry points from plain C: include/nkv_merkle.h with them in
it still compiles as C99 -pedantic -Werror, the two symbols link, a null
context is refused by both, adding them did not bump the ABI version, and the
ctypes binding declares them with the header's argument counts, constants and
struct layout.  No device is needed."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "lookup_abi_c99.c")


def test_lookup_entry_points_from_c99(tmp_path):
    from nakevaleng_amd import _lib, build as b
    so = b.build(quiet=True)
    libdir = os.path.dirname(so)
    exe = os.path.join(str(tmp_path), "lookup_abi_c99")
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
        _lib.NKV_LOOKUP_MAX_TABLES, _lib.NKV_STAGE_NOT_SEARCHED, _lib.NKV_STAGE_FILTER, _lib.NKV_STAGE_SUMMARY,
        _lib.NKV_STAGE_INDEX, _lib.NKV_STAGE_FOUND, _lib.NKV_GET_ABSENT, _lib.NKV_GET_LIVE, _lib.NKV_GET_TOMBSTONE]
    assert [int(x) for x in kv["constants"].split()] == [32, 0, 1, 2, 3, 4, 0, 1, 2]
    T = _lib.NkvLookupTable
    assert [int(x) for x in kv["struct"].split()] == [ctypes.sizeof(T), T.bits.offset, T.seed0.offset]
    assert _lib.lib().nkv_abi_version() == 1 == _lib.NKV_ABI_VERSION


def test_binding_declares_the_lookup_entries():
    from nakevaleng_amd import _lib
    assert {"nkv_lookup_dev", "nkv_lookup_values_dev"} <= set(_lib.SIGNATURES)
    assert len(_lib.SIGNATURES["nkv_lookup_dev"][1]) == 11
    assert len(_lib.SIGNATURES["nkv_lookup_values_dev"][1]) == 10
    assert _lib.NKV_HIT_NONE == 2**64 - 1
