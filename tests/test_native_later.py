"""The libraries of _native.LATER_LIBRARIES: each one's header, its row of the table and the built library name the same
symbols (what tests/test_native_libraries.py and tests/test_native_tsne.py check for the two earlier tables).  Nothing here
pins the table's names or a symbol count: the header of a row says how many symbols there are, so the next library breaks
nothing.  No GPU."""
import os
import re

import pytest

from conftest import ROOT

from prosstt_amd import _native

TABLES = (_native.LIBRARIES, _native.ADDED_LIBRARIES, _native.LATER_LIBRARIES)


def test_the_tables_do_not_overlap():
    names = [name for table in TABLES for name in table]
    assert len(set(names)) == len(names)
    paths = [spec.path for table in TABLES for spec in table.values()]
    assert len(set(paths)) == len(paths)
    headers = [spec.header for table in TABLES for spec in table.values()]
    assert len(set(headers)) == len(headers)
    assert _native.LATER_LIBRARIES
    for name, spec in _native.LATER_LIBRARIES.items():
        assert _native._library(name) is spec


@pytest.mark.parametrize("name", list(_native.LATER_LIBRARIES))
def test_library_exports_every_declared_symbol(name):
    spec = _native.LATER_LIBRARIES[name]
    header = open(os.path.join(ROOT, "include", spec.header)).read()
    declared = re.findall(r"\b(prosstt_amd_\w+)\s*\(", header)
    assert declared and len(set(declared)) == len(declared)           # every symbol declared once
    assert set(declared) == set(spec.symbols)
    assert len(spec.symbols) == len(declared)
    assert all(symbol.startswith("prosstt_amd_%s_" % name) for symbol in declared)
    assert spec.last_error in spec.symbols
    makefile = open(os.path.join(ROOT, "prosstt_amd", "csrc", "Makefile")).read()
    row = re.search(r"^row_%s\s*:=\s*(\S+)\s+(\S+)\s+(\S+)" % name, makefile, re.M)
    assert row and row.group(2) == os.path.basename(spec.path) and row.group(3) == spec.header
    assert os.path.exists(os.path.join(ROOT, "prosstt_amd", "csrc", row.group(1)))
    listed = re.search(r"^%s_LIBS\s*:=(.*)$" % ("HIP" if spec.hip else "HOST"), makefile, re.M)
    assert listed and name in listed.group(1).split()
    if os.path.exists(spec.path):
        pytest.importorskip("torch")                  # the library links the HIP runtime: torch's comes first
        lib = _native.load(name)
        for symbol in declared:
            assert hasattr(lib, symbol), symbol
        exported = os.popen("nm -D --defined-only %s" % spec.path).read()
        assert set(re.findall(r"\b(prosstt_amd_\w+)", exported)) == set(declared)
