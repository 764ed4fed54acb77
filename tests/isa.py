"""The gfx950 device assembly of the package's HIP libraries, as prosstt_amd/csrc/Makefile compiles them (`make isa-<name>`:
the library's own compile line with -save-temps; cross-compiles without a GPU), and what the test_*_isa.py files read
from it."""
import functools
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def assembly(name):
    """The device assembly of library ``name`` (a row of the makefile's table), compiled once per process; skips the
    test when there is no hipcc."""
    if not shutil.which(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")):
        pytest.skip("no hipcc")
    tmp = tempfile.mkdtemp(prefix="prosstt_%s_isa_" % name)
    try:
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "prosstt_amd", "csrc"), "isa-" + name, "ISA_DIR=" + tmp],
                              stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        return open(os.path.join(tmp, name + ".s")).read()
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def body(text, mangled_part):
    m = re.search(r"^(_Z\w*%s\w*):[^\n]*\n(.*?)\n\s+s_endpgm" % mangled_part, text, re.S | re.M)
    assert m, mangled_part
    return m.group(2)


def meta(text, mangled_part, key):
    for blk in re.split(r"\n  - \.agpr_count", text)[1:]:
        if re.search(r"\.name:\s+\S*%s" % mangled_part, blk):
            return int(re.search(r"\." + key + r":\s+(\d+)", blk).group(1))
    raise AssertionError(mangled_part)


# any floating-point atomic: global / flat / buffer / LDS add, min, max, pk_add on f16, bf16, f32 or f64
FLOAT_ATOMIC = re.compile(r"\b(global|flat|buffer|ds)_(atomic_)?(add|sub|pk_add|min|max|fmin|fmax|cmpswap)\w*_(f16|bf16|f32|f64)\b"
                          r"|\bds_(add|min|max)_rtn_f\d+\b|\b\w+_atomic_\w*f(32|64)\b")


def global_atomics(text):
    """Every atomic on global memory that ``text`` names."""
    return re.findall(r"\b(?:global|flat|buffer)_atomic_\w+", text)


def lds_atomics(text):
    """Every atomic on LDS that ``text`` names."""
    return re.findall(r"\bds_(?:add|sub|inc|dec|min|max|and|or|xor|cmpst|wrxchg)\w*", text)
