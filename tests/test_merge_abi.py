"""The compaction merge's two entry points from plain C: include/nkv_merkle.h
with them in it still compiles as C99 -pedantic -Werror, both symbols link, and
adding them did not bump the ABI version (the header's rule: new entry points
do not)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "merge_abi_c99.c")


def test_merge_entry_points_from_c99(tmp_path):
    from nakevaleng_amd import _lib, build as b
    so = b.build(quiet=True)
    libdir = os.path.dirname(so)
    exe = os.path.join(str(tmp_path), "merge_abi_c99")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Werror", "-Wall", "-Wextra", "-O1",
                           "-I", os.path.join(ROOT, "include"), SRC, "-L", libdir, "-lnkvmerkle",
                           f"-Wl,-rpath,{libdir}", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    kv = dict(line.split(" ", 1) for line in out.stdout.strip().splitlines())
    assert kv["abi"] == "1"
    assert kv["max_runs"] == "16" == str(_lib.NKV_MERGE_MAX_RUNS)
    assert kv["symbols"] == "1"
    assert kv["null_ctx"] == "2 2"  # NKV_ERR_INVALID from both
    assert _lib.lib().nkv_abi_version() == 1 == _lib.NKV_ABI_VERSION


def test_binding_declares_the_merge_entries():
    from nakevaleng_amd import _lib
    assert {"nkv_merge_records_dev", "nkv_merge_records"} <= set(_lib.SIGNATURES)
    assert [f[0] for f in _lib.NkvRun._fields_] == ["stream", "stream_len", "rec_off", "n"]
