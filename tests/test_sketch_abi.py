"""The sketch entry points from plain C: include/nkv_merkle.h with them in it
still compiles as C99 -pedantic -Werror, the twelve symbols link, a null
context is refused by the ten entries that take one, adding them did not bump
the ABI version, and the ctypes binding declares them with the header's
argument counts.  No device is needed."""
import math
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "sketch_abi_c99.c")
ARGS = {"nkv_hll_add_dev": 7, "nkv_hll_add_records_dev": 7, "nkv_cms_insert_dev": 9,
        "nkv_cms_insert_records_dev": 9, "nkv_cms_query_dev": 10, "nkv_hll_add": 7, "nkv_hll_add_records": 7,
        "nkv_cms_insert": 9, "nkv_cms_insert_records": 9, "nkv_cms_query": 10, "nkv_cms_params": 4,
        "nkv_hll_estimate": 4}


def test_sketch_entry_points_from_c99(tmp_path):
    from nakevaleng_amd import _lib, build as b
    so = b.build(quiet=True)
    libdir = os.path.dirname(so)
    exe = os.path.join(str(tmp_path), "sketch_abi_c99")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Werror", "-Wall", "-Wextra", "-O1",
                           "-I", os.path.join(ROOT, "include"), SRC, "-L", libdir, "-lnkvmerkle",
                           f"-Wl,-rpath,{libdir}", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    kv = dict(line.split(" ", 1) for line in out.stdout.strip().splitlines())
    assert kv["abi"] == "1"
    assert kv["symbols"] == "1"
    assert kv["null_ctx"] == " ".join(["2"] * 10)  # NKV_ERR_INVALID from all ten
    assert kv["untouched"] == "1"
    assert kv["params"] == "0 28 3"
    assert kv["params_refused"] == "2 2 2"
    rc, est = kv["estimate"].split()
    assert rc == "0" and float(est) == 16.0 * math.log(16.0 / 15.0)
    assert kv["constants"] == f"4 16 1 {_lib.NKV_OPT_SKETCH_PATH}"
    assert _lib.lib().nkv_abi_version() == 1 == _lib.NKV_ABI_VERSION


def test_binding_declares_the_sketch_entries():
    from nakevaleng_amd import _lib
    assert set(ARGS) <= set(_lib.SIGNATURES)
    for name, count in ARGS.items():
        assert len(_lib.SIGNATURES[name][1]) == count, name
    assert _lib.NKV_OPT_SKETCH_PATH == 21


def test_header_declares_the_sketch_entries_with_these_argument_counts():
    import re
    src = open(os.path.join(ROOT, "include", "nkv_merkle.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, count in ARGS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
        assert m, name
        assert len(m.group(1).split(",")) == count, name


def test_python_exposes_the_sketches():
    from nakevaleng_amd import lsmtree, sketch, sstable
    assert callable(sketch.New) and callable(sketch.NewCMS)
    assert callable(sstable.key_sketches_from_records) and callable(lsmtree.key_sketches)
