"""The live memtable's entry points from plain C: include/nkv_merkle.h with them
in it still compiles as C99 -pedantic -Werror, the four symbols link, a null
context is refused by each entry that takes one, nkv_memtable_index_bytes
refuses what is no power of two in 2..2^32, adding them did not bump the ABI
version, and the ctypes binding and the Python module declare them.  No device
is needed."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "memtable_abi_c99.c")


def test_memtable_entry_points_from_c99(tmp_path):
    from nakevaleng_amd import _lib, build as b
    so = b.build(quiet=True)
    libdir = os.path.dirname(so)
    exe = os.path.join(str(tmp_path), "memtable_abi_c99")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Werror", "-Wall", "-Wextra", "-O1",
                           "-I", os.path.join(ROOT, "include"), SRC, "-L", libdir, "-lnkvmerkle",
                           f"-Wl,-rpath,{libdir}", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    kv = dict(line.split(" ", 1) for line in out.stdout.strip().splitlines())
    assert kv["abi"] == "1"
    assert kv["symbols"] == "1"
    assert kv["null_ctx"] == "2 2 2"  # NKV_ERR_INVALID from each
    assert [int(x) for x in kv["constants"].split()] == [
        _lib.NKV_FLUSH_BY_CAPACITY, _lib.NKV_FLUSH_BY_THRESHOLD, _lib.NKV_MEMTABLE_STATE_WORDS] == [1, 2, 4]
    assert [int(x) for x in kv["index_bytes"].split()] == [0, 0, 0, 0, 16, 8 << 32]
    assert _lib.lib().nkv_abi_version() == 1 == _lib.NKV_ABI_VERSION


def test_binding_declares_the_memtable_entries():
    from nakevaleng_amd import _lib
    want = {"nkv_memtable_index_bytes": 1, "nkv_memtable_clear_dev": 4, "nkv_memtable_add_dev": 14,
            "nkv_memtable_find_dev": 16}
    for name, argc in want.items():
        assert len(_lib.SIGNATURES[name][1]) == argc, name
    L = _lib.lib()
    assert [L.nkv_memtable_index_bytes(s) for s in (0, 3, 1 << 33, 8192)] == [0, 0, 0, 65536]


def test_python_names_exist():
    import inspect
    from nakevaleng_amd import lsmtree, memtable
    for name in ("put_many", "add_log", "find_many", "count", "should_flush", "flush", "clear"):
        assert callable(getattr(memtable.Memtable, name)), name
    sig = inspect.signature(memtable.Memtable.__init__)
    assert [sig.parameters[p].default for p in ("strategy", "capacity", "threshold")] == [3, 10, 2048]
    assert inspect.signature(lsmtree.get_many).parameters["memtable"].default is None
