"""What regress and factors share on the host (prosstt_amd/csrc/quasi_device.h, prosstt_amd/_cellpass.py):
the order and the words of their entry points' refusals, the one slab layout behind both ``*_workspace_bytes``, factors'
status messages as derived from regress's, and the helpers both wrappers take from ``_cellpass``.  It needs the built
libraries, not a device: every call here is refused, or only counts bytes, before the first use of a pointer or the runtime.
The messages are those of the build before the header existed, restated as literals."""
import ctypes

import pytest

from prosstt_amd import _cellpass, _native, device, factors, regress

ONE = ctypes.c_void_p(256)              # never read: a refusal comes first


def refused(name, call, **arguments):
    """The message with which ``call`` refuses ``arguments``."""
    assert call(**arguments) == _native.EINVAL, arguments
    return getattr(_native.load(name), "prosstt_amd_%s_last_error" % name)().decode()


def regress_call(N, G, ld, K, ldd, p, split, data, ws_bytes):
    return _native.load("regress").prosstt_amd_regress_normal_equations(
        None, data, N, G, ld, data, data, K, data, ldd, p, data, data, data, 0, split, data, ws_bytes, data, data, data, data, data)


def factors_call(N, G, ld, ldl, p, split, genes_per_block, data, ws_bytes):
    return _native.load("factors").prosstt_amd_factors_cell_equations(
        None, data, N, G, ld, data, None, data, ldl, p, data, data, data, split, genes_per_block, data, ws_bytes, data, data, data,
        data, data)


def test_regress_refuses_in_its_order_with_its_words():
    """Everything is wrong at first; each step mends what the step before it named."""
    bad = dict(N=0, G=5, ld=4, K=0, ldd=2, p=17, split=5, data=None, ws_bytes=100)
    steps = [
        ({}, "need 1 <= N < 2^31 and G >= 1 (got N = 0, G = 5)"),
        (dict(N=5), "need 1 <= p <= 16 coefficients (got 17)"),
        (dict(p=3), "need 1 <= K < 2^31 rows of the design (got 0)"),
        (dict(K=2), "row stride 4 is below the row length 5"),
        (dict(ld=5), "row stride 2 is below the row length 3"),
        (dict(ldd=3), "split must be 0, 8, 16 or 32 (got 5)"),
        (dict(split=0), "NULL argument"),
        (dict(data=ONE), "workspace of 100 bytes, 768 needed"),
    ]
    for mend, message in steps:
        bad.update(mend)
        assert refused("regress", regress_call, **bad) == message
    assert refused("regress", regress_call, **dict(bad, G=2 ** 40)) == "too many genes for one launch (G = 1099511627776)"


def test_factors_refuses_in_its_order_with_its_words():
    bad = dict(N=0, G=5, ld=4, ldl=2, p=17, split=5, genes_per_block=40, data=None, ws_bytes=100)
    steps = [
        ({}, "need 1 <= N < 2^31 and 1 <= G < 2^31 (got N = 0, G = 5)"),
        (dict(N=5), "need 1 <= p <= 16 coefficients (got 17)"),
        (dict(p=3), "genes_per_block must be 0 or a multiple of 32 (got 40)"),
        (dict(genes_per_block=32), "row stride 4 is below the row length 5"),
        (dict(ld=5), "row stride 2 is below the row length 3"),
        (dict(ldl=3), "split must be 0, 8, 16 or 32 (got 5)"),
        (dict(split=0), "NULL argument"),
        (dict(data=ONE), "workspace of 100 bytes, 768 needed"),
    ]
    for mend, message in steps:
        bad.update(mend)
        assert refused("factors", factors_call, **bad) == message
    assert (refused("factors", factors_call, **dict(bad, G=2 ** 31 - 1, ld=2 ** 31 - 1))
            == "genes_per_block = 32 cuts 2147483647 genes into more than 65535 blocks")


def pad(n):
    return (n + 255) // 256 * 256


def slab_bytes(blocks, sums, length):
    """[blocks][sums + 1][length] binary64 (U, I, then Q) and [blocks][length] uint32 (used), each padded to 256 bytes."""
    return pad(blocks * (sums + 1) * length * 8) + pad(blocks * length * 4)


@pytest.mark.parametrize("N, G", [(1, 1), (300, 257), (257, 513), (50000, 20000)])
@pytest.mark.parametrize("p", [1, 16])
def test_both_workspaces_are_the_one_slab_layout(N, G, p):
    sums = p + p * (p + 1) // 2
    need = ctypes.c_uint64(0)
    _native.check(_native.load("regress").prosstt_amd_regress_workspace_bytes(N, G, p, ctypes.byref(need)), "regress")
    assert need.value == slab_bytes(regress.row_blocks(N, G)[1], sums, G)
    _native.check(_native.load("factors").prosstt_amd_factors_workspace_bytes(N, G, p, 0, ctypes.byref(need)), "factors")
    assert need.value == slab_bytes(factors.gene_blocks(N, G)[1], sums, N)


def test_factors_status_messages_are_what_they_were():
    assert factors.STATUS_MESSAGES == (
        (1, "NEGATIVE", device.NEGATIVE_ENTRY),
        (4, "PARAMETER", "alpha and beta must be finite with alpha >= 0 and beta >= 1"),
        (8, "SIZE", "a size factor is not positive and finite (at most 1e150)"),
        (16, "COEFFICIENT", "a coefficient or a loading is not finite"),
        (32, "ETA", "a linear predictor is not finite or beyond 700 in size, or a mean overflowed"),
    )
    assert (factors.NEGATIVE, factors.PARAMETER, factors.SIZE, factors.COEFFICIENT, factors.ETA) == (1, 4, 8, 16, 32)
    assert regress.STATUS_MESSAGES[1] == (2, "LABEL", "a label is not below the number of rows of the design")
    assert regress.STATUS_MESSAGES[4] == (16, "COEFFICIENT", "a coefficient is not finite")


def test_the_shared_helpers_are_one_object_each():
    assert regress._per_gene is factors._per_gene is _cellpass._per_gene
    assert regress._check_split is factors._check_split is _cellpass._check_split
    assert regress.SPLITS is _cellpass.SPLITS and regress.SPLITS == (8, 16, 32)
    assert issubclass(factors._CellPass, _cellpass.SizedPass) and not issubclass(factors._CellPass, _cellpass.LabelledPass)
    assert issubclass(regress._Pass, _cellpass.LabelledPass) and issubclass(_cellpass.LabelledPass, _cellpass.SizedPass)
