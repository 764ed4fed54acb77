"""
What ``fit``, ``regress`` and ``factors`` share on the host: each runs a pass over a device count matrix whose cells carry a
size factor and, for the first two, a label (the row of a table: of means, of a design), in libraries built on one kernel plan
(csrc/column_device.h) or one definition of the sums (csrc/quasi_device.h), and each reports what the pass refused through a
status word.  Internal; every check here comes before any device use.
"""
import numpy as np

from . import markers
from . import device as _device
from .device import _torch


def _host(a):
    torch = _torch()
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a


def _codes(labels, n_cells):
    """int64 row of the table per cell in plan order (-1: left out), by ``markers.encode_labels``'s rule without its limit
    on the number of groups: integers are their own codes, names are numbered in sorted order; None: every cell in row 0."""
    if labels is None:
        return np.zeros(n_cells, dtype=np.int64)
    arr = np.asarray(_host(labels))
    if arr.shape != (n_cells,):
        raise ValueError("need one label per cell: shape (%d,), not %s" % (n_cells, arr.shape))
    if arr.dtype.kind in "iu":
        if arr.size and int(arr.max()) >= 1 << 31:
            raise ValueError("labels must be below 2^31")
        return np.where(arr < 0, -1, arr).astype(np.int64)
    if arr.dtype.kind in "bf":
        raise ValueError("labels must be integers or names, not %s" % arr.dtype)
    return np.unique(arr, return_inverse=True)[1].astype(np.int64).reshape(-1)


def size_factors(sc, n_cells):
    """``sc`` as a float64 host array, one per cell, or raise."""
    s = np.asarray(_host(sc), dtype=np.float64)
    if s.shape != (n_cells,):
        raise ValueError("need one size factor per cell: shape (%d,), not %s" % (n_cells, s.shape))
    return s


def check_status(bits, messages):
    """ValueError naming every bit of a pass's status word that is set; ``messages``: (bit, name, text) per known bit."""
    said = ["status bit %s (%d): %s" % (name, bit, text) for bit, name, text in messages if bits & bit]
    if said:
        raise ValueError("; ".join(said))
    if bits:
        raise RuntimeError("the pass set an unknown status bit (status %d)" % bits)


SPLITS = (8, 16, 32)            # how many sums of (U, I) a block of a quasi-likelihood pass may keep; 0 is the library's choice


def _check_split(split):
    if isinstance(split, (bool, np.bool_)) or split not in (0,) + SPLITS:
        raise ValueError("split must be 0 (the library's choice), 8, 16 or 32 (got %r)" % (split,))
    return int(split)


def _per_gene(value, n_genes, name):
    v = np.asarray(_host(value), dtype=np.float64)
    if v.ndim == 0:
        v = np.full(n_genes, float(v))
    if v.shape != (n_genes,):
        raise ValueError("%s must be a number or one per gene: shape (%d,), not %s" % (name, n_genes, v.shape))
    return np.ascontiguousarray(v)


class SizedPass:
    """The device side of repeated calls of a pass over one matrix whose cells carry a size factor.  ``__init__`` checks the
    matrix and the size factors on the host; ``place_size`` is the first use of the device."""

    def __init__(self, X, sc, who):
        m = X if isinstance(X, _device.CountMatrix) else _device.CountMatrix(X, who)
        if m.N < 1 or m.G < 1:
            raise ValueError("%s needs at least one cell and one gene (got %d x %d)" % (who, m.N, m.G))
        self._check_bounds(m, who)
        self.m, self._sc = m, size_factors(sc, m.N)

    def _check_bounds(self, m, who):
        if m.N >= 1 << 31:
            raise ValueError("%s takes fewer than 2^31 cells" % who)

    def place_size(self, name):
        """The checked matrix view, library ``name``, and the size factors in row order on the matrix's device.  Returns
        the view."""
        m = self.m.on_device()
        self.lib = _device.need_device(name)
        torch = _torch()
        with torch.cuda.device(m.device):
            self.size = torch.as_tensor(np.ascontiguousarray(markers.codes_in_row_order(self._sc, m.cell_of_row))).to(m.device)
        return m


class LabelledPass(SizedPass):
    """A ``SizedPass`` whose cells carry a label besides.  The subclass checks what it adds after ``__init__`` and then calls
    ``place``, the first use of the device."""

    def place(self, codes, name, query_symbol, *sizes):
        """``place_size``, the labels in row order on the matrix's device, and the workspace that ``query_symbol`` asks for
        the matrix and ``sizes``.  Returns the device."""
        m = self.place_size(name)
        torch = _torch()
        with torch.cuda.device(m.device):
            rows = markers.codes_in_row_order(codes, m.cell_of_row)
            self.labels = torch.as_tensor(np.ascontiguousarray(rows, dtype=np.int32)).to(m.device)
            self.ws = m.workspace(name, query_symbol, *sizes)
        return m.device
