"""The framing entry points from plain C: include/nkv_merkle.h with them in it
still compiles as C99 -pedantic -Werror, the two symbols link, a null context
is refused by both, adding them did not bump the ABI version, the ctypes
binding declares them with the header's argument counts, and the Python side
exposes what is built on them.  No device is needed."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "frame_abi_c99.c")


def test_frame_entry_points_from_c99(tmp_path):
    from nakevaleng_amd import _lib, build as b
    so = b.build(quiet=True)
    libdir = os.path.dirname(so)
    exe = os.path.join(str(tmp_path), "frame_abi_c99")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Werror", "-Wall", "-Wextra", "-O1",
                           "-I", os.path.join(ROOT, "include"), SRC, "-L", libdir, "-lnkvmerkle",
                           f"-Wl,-rpath,{libdir}", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    kv = dict(line.split(" ", 1) for line in out.stdout.strip().splitlines())
    assert kv["abi"] == "1"
    assert kv["symbols"] == "1"
    assert kv["constants"] == (f"{_lib.NKV_FRAME_STRICT} {_lib.NKV_OPT_FRAME_PATH} {_lib.NKV_OPT_FRAME_BUDGET} "
                               f"{_lib.NKV_PATH_FRAME_WALK} {_lib.NKV_PATH_FRAME_SPECULATIVE}")
    assert kv["null_ctx"] == "2 2"  # NKV_ERR_INVALID from both
    assert kv["untouched"] == "1"
    assert _lib.lib().nkv_abi_version() == 1 == _lib.NKV_ABI_VERSION


def test_binding_declares_the_frame_entries():
    from nakevaleng_amd import _lib
    assert {"nkv_frame_records_dev", "nkv_frame_records"} <= set(_lib.SIGNATURES)
    assert len(_lib.SIGNATURES["nkv_frame_records_dev"][1]) == 12
    assert len(_lib.SIGNATURES["nkv_frame_records"][1]) == 12
    assert (_lib.NKV_FRAME_STRICT, _lib.NKV_OPT_FRAME_PATH, _lib.NKV_OPT_FRAME_BUDGET) == (1, 22, 23)


def test_python_side_exposes_the_framing():
    from nakevaleng_amd import lsmtree, record, sstable, wal
    assert callable(record.frame) and callable(sstable.open_data_table)
    assert callable(wal.read_segments) and callable(lsmtree.recover)
