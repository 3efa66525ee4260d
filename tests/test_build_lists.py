"""The library's source hash (nakevaleng_amd/build.py) covers exactly what is
under csrc/: a source or header missing from SOURCES / HEADERS would go
unhashed, and a stale library would pass for a fresh one.
"""
import os

from nakevaleng_amd import build as nb


def test_every_csrc_file_is_listed_exactly_once():
    on_disk = sorted(f for f in os.listdir(nb.CSRC) if f.endswith((".hip", ".cpp", ".hpp")))
    listed = nb.SOURCES + nb.HEADERS
    assert sorted(listed) == on_disk, (sorted(set(on_disk) - set(listed)), sorted(set(listed) - set(on_disk)))
    assert len(set(listed)) == len(listed), "a name is listed twice"
    assert all(f.endswith((".hip", ".cpp")) for f in nb.SOURCES)
    assert all(f.endswith(".hpp") for f in nb.HEADERS)


def test_every_listed_file_exists():
    missing = [f for f in nb.SOURCES + nb.HEADERS if not os.path.isfile(os.path.join(nb.CSRC, f))]
    assert not missing, missing
