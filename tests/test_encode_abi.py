"""The record-encode entry points from plain C: include/nkv_merkle.h with them
in it still compiles as C99 -pedantic -Werror, the two symbols link, a null
context is refused by both, adding them did not bump the ABI version, the
ctypes binding declares them with the header's argument counts, and its
NkvPuts structure is laid out as the C compiler lays out nkv_puts.  No device
is needed."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "encode_abi_c99.c")
FIELDS = ["keys", "keys_len", "koff", "klen", "vals", "vals_len", "voff", "vlen", "ts", "ts_all", "status", "type",
          "n"]


def test_encode_entry_points_from_c99(tmp_path):
    from nakevaleng_amd import _lib, build as b
    so = b.build(quiet=True)
    libdir = os.path.dirname(so)
    exe = os.path.join(str(tmp_path), "encode_abi_c99")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Werror", "-Wall", "-Wextra", "-O1",
                           "-I", os.path.join(ROOT, "include"), SRC, "-L", libdir, "-lnkvmerkle",
                           f"-Wl,-rpath,{libdir}", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    kv = dict(line.split(" ", 1) for line in out.stdout.strip().splitlines())
    assert kv["abi"] == "1"
    assert kv["symbols"] == "1"
    assert kv["null_ctx"] == "2 2"  # NKV_ERR_INVALID from both
    assert kv["untouched"] == "1"
    assert _lib.lib().nkv_abi_version() == 1 == _lib.NKV_ABI_VERSION
    # the ctypes structure against the C compiler's layout
    assert int(kv["sizeof"]) == ctypes.sizeof(_lib.NkvPuts)
    assert [name for name, _ in _lib.NkvPuts._fields_] == FIELDS
    assert [int(x) for x in kv["offsets"].split()] == [getattr(_lib.NkvPuts, f).offset for f in FIELDS]


def test_binding_declares_the_encode_entries():
    from nakevaleng_amd import _lib
    assert {"nkv_encode_records_dev", "nkv_encode_records"} <= set(_lib.SIGNATURES)
    assert len(_lib.SIGNATURES["nkv_encode_records_dev"][1]) == 7
    assert len(_lib.SIGNATURES["nkv_encode_records"][1]) == 7


def test_python_exposes_the_encoder():
    from nakevaleng_amd import lsmtree, record
    assert callable(record.encode_many) and callable(lsmtree.flush_puts)
