"""The admission entry point from plain C: include/nkv_merkle.h with it in it
still compiles as C99 -pedantic -Werror, the symbol links, a null context is
refused, adding it did not bump the ABI version, and the ctypes binding and the
Python modules declare it.  No device is needed."""
import ctypes
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "admit_abi_c99.c")


def test_admit_entry_point_from_c99(tmp_path):
    from nakevaleng_amd import _lib, build as b
    so = b.build(quiet=True)
    libdir = os.path.dirname(so)
    exe = os.path.join(str(tmp_path), "admit_abi_c99")
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Werror", "-Wall", "-Wextra", "-O1",
                           "-I", os.path.join(ROOT, "include"), SRC, "-L", libdir, "-lnkvmerkle",
                           f"-Wl,-rpath,{libdir}", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    kv = dict(line.split(" ", 1) for line in out.stdout.strip().splitlines())
    assert kv["abi"] == "1"
    assert kv["symbols"] == "1"
    assert kv["null_ctx"] == "2 2"  # NKV_ERR_INVALID from each
    assert [int(x) for x in kv["constants"].split()] == [
        _lib.NKV_ADMIT_ILLEGAL, _lib.NKV_ADMIT_ALLOWED, _lib.NKV_ADMIT_THROTTLED, _lib.NKV_ADMIT_BAD_SPAN,
        _lib.NKV_ADMIT_BAD_KEY, _lib.NKV_ADMIT_BAD_TIME, _lib.NKV_ADMIT_BAD_BUCKET] == [0, 1, 2, 1, 2, 4, 8]
    assert int(kv["sizeof"]) == ctypes.sizeof(_lib.NkvRequests) == 14 * 8
    assert _lib.lib().nkv_abi_version() == 1 == _lib.NKV_ABI_VERSION


def test_binding_declares_the_admit_entry():
    from nakevaleng_amd import _lib
    assert len(_lib.SIGNATURES["nkv_admit_dev"][1]) == 12
    names = [f[0] for f in _lib.NkvRequests._fields_]
    assert names == ["users", "users_len", "uoff", "ulen", "keys", "keys_len", "koff", "klen", "ts", "ts_all",
                     "buckets", "boff", "bstatus", "n"]
    # a null context is refused through the binding too, before any pointer is read
    req = _lib.NkvRequests()
    assert _lib.lib().nkv_admit_dev(None, ctypes.byref(req), b"$", 1, 100, 1, None, None, None, None, None,
                                    None) == _lib.NKV_ERR_INVALID


def test_python_names_exist():
    import inspect
    from nakevaleng_amd import engine, tokenbucket
    for name in ("new", "has_enough_tokens", "to_bytes", "from_bytes"):
        assert callable(getattr(tokenbucket.TokenBucket, name)), name
    assert callable(tokenbucket.validate_params)
    sig = inspect.signature(tokenbucket.admit_many)
    assert [sig.parameters[p].default for p in ("start", "max_tokens", "reset_interval", "stored")] == \
        [b"$", 100, 1, None]  # coreconf.go:40-45
    for f in (engine.put_many, engine.get_many):
        assert list(inspect.signature(f).parameters)[:5] == ["mt", "tables", "users", "keys",
                                                             "values" if f is engine.put_many else "now"]
