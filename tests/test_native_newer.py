"""The libraries of _native.NEWER_LIBRARIES: each one's header, its row of the table and the built library name the same
symbols (what tests/test_native_later.py checks for the table before it), the four tables do not overlap, and every library
here brings the guard-band test file of its own that the table's comment asks for.  Nothing here pins the table's names or a
symbol count: the header of a row says how many symbols there are, so the next library breaks nothing.  No GPU."""
import os
import re

import pytest

from conftest import ROOT

from prosstt_amd import _native

TABLES = (_native.LIBRARIES, _native.ADDED_LIBRARIES, _native.LATER_LIBRARIES, _native.NEWER_LIBRARIES)


def test_the_four_tables_do_not_overlap():
    names = [name for table in TABLES for name in table]
    assert len(set(names)) == len(names)
    paths = [spec.path for table in TABLES for spec in table.values()]
    assert len(set(paths)) == len(paths)
    headers = [spec.header for table in TABLES for spec in table.values()]
    assert len(set(headers)) == len(headers)
    assert _native.NEWER_LIBRARIES
    for table in TABLES:
        for name, spec in table.items():
            assert _native._library(name) is spec
    with pytest.raises(KeyError):
        _native._library("no such library")


def test_the_makefile_counts_its_libraries():
    makefile = open(os.path.join(ROOT, "prosstt_amd", "csrc", "Makefile")).read()
    hip = re.search(r"^HIP_LIBS\s*:=(.*)$", makefile, re.M).group(1).split()
    words = ["zero", "one", "two", "three", "four", "five", "six", "seven", "eight", "nine", "ten", "eleven", "twelve", "thirteen",
             "fourteen", "fifteen", "sixteen", "seventeen", "eighteen", "nineteen", "twenty"]
    said = re.search(r"^# Builds every shared library of the package into \.\./lib: (\w+) HIP libraries", makefile, re.M)
    assert said and said.group(1) in (words[len(hip)] if len(hip) < len(words) else "", str(len(hip)))
    on_device = {name for table in TABLES for name, spec in table.items() if spec.hip}
    assert set(hip) == on_device


@pytest.mark.parametrize("name", list(_native.NEWER_LIBRARIES))
def test_library_exports_every_declared_symbol(name):
    spec = _native.NEWER_LIBRARIES[name]
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


@pytest.mark.parametrize("name", [n for n, spec in _native.NEWER_LIBRARIES.items() if spec.hip])
def test_library_brings_its_own_guard_band_test(name):
    path = os.path.join(ROOT, "tests", "test_gpu_%s_guard_bands.py" % name)
    assert os.path.exists(path), path
    text = open(path).read()
    assert "pytestmark = pytest.mark.gpu" in text and "_guarded_runs(" in text and "def small_%s(" % name in text
