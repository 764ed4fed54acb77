"""Every shared library of the package: its header, the loader's table (_native.LIBRARIES) and the built library name the
same symbols.  COUNT is the census of the libraries: a new one adds its entry here.  No GPU."""
import os
import re

import pytest

from conftest import ROOT

from prosstt_amd import _native

COUNT = {"sampler": 29, "host": 7, "stats": 3, "embed": 5, "knn": 3, "graph": 7, "layout": 3}


@pytest.mark.parametrize("name", list(_native.LIBRARIES))
def test_library_exports_every_declared_symbol(name):
    spec = _native.LIBRARIES[name]
    header = open(os.path.join(ROOT, "include", spec.header)).read()
    declared = set(re.findall(r"\b(prosstt_amd_\w+)\s*\(", header))
    assert declared == set(spec.symbols)
    assert len(declared) == COUNT[name]
    if os.path.exists(spec.path):
        if spec.hip:
            pytest.importorskip("torch")              # the library links the HIP runtime: torch's comes first
        lib = _native.load(name)
        for symbol in declared:
            assert hasattr(lib, symbol), symbol
    if name == "sampler":
        assert _native.load().prosstt_amd_version() == 600       # PRNB-7 (the version moves with the sampler's definition)
    if name == "host":
        assert _native.load("host").prosstt_amd_host_has_avx2() in (0, 1)
