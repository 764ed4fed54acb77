"""
-m gpu: the sampler's domain check (``check_domain`` / ``strict``) against the reference's rule, one offending sample at a
time, through every path the verdict takes on the device.

The rule is ``oracle.ref_numpy.domain_error``: ``draw_counts``' argument check (scipy's, simulation.py:647-648) evaluated
in binary64 from the arrays the device is given.  The verdict is split over three kernels -- ``row_flags_kernel`` (a used
row of the mean tensor has an entry that is not a positive finite number), ``prep_kernel`` (a cell's scaling, a gene with
alpha < 0 or beta < 1 that asks for the full pass, a row index outside the tensor) and the per-sample pass at the tail of
``sample_counts_heavy_kernel`` (theta = alpha*m + beta - 1 < 0) -- plus the request word of alternating parity, the
sticky verdict words and the cached row flags on the host side.  Every case below

  1. runs an all-valid input through the checked call: no raise;
  2. plants ONE value and asks for the verdict: it must be the rule's;
  3. takes the value out again: no raise, on the same context;

through ``check_domain=True``, through ``"deferred"`` + ``domain_status()``, and (a subset) through the C ABI with host
pointers.  The cases are built without a GPU (``CASES``): tests/test_domain_rule.py imports them and asserts on the CPU
that none of their samples lies in the band where binary32 rounding could decide the sign of theta, so every verdict
here is required exactly.

Shapes are the smallest at which each loop takes another step (constants read from the sources by ``kernel_constants``):
``row_flags_kernel`` -- 256 threads stride the genes of a row, at most 65 536 blocks stride the rows; ``prep_kernel`` --
one thread per index below max(N + 4, G), 256 to a block; the per-sample pass -- blocks (at least 256) stride the cells,
``kHeavyBlock`` threads stride the genes.
"""
import ctypes
import functools
import os
import re
from dataclasses import dataclass

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- the value table (pinned on the CPU by tests/test_domain_rule.py) -------------------------------------------------
MEAN_VALUES = (0.0, -0.0, -1.0, float("nan"), float("inf"), float("-inf"), 1e-45, 1.17549435e-38, 1.0, 5000.0)
SCALING_VALUES = (0.0, -1.0, float("nan"), float("inf"), 1e-50, 1e-10, 1.0)
PARAM_VALUES = ((0.2, 2.0), (0.0, 1.0), (0.0, 1.0 + 1e-8), (-0.1, 2.0), (0.2, 0.5), (0.0, 0.5), (-0.1, 1.0), (-1e-4, 1.5),
                (5.0, 40.0))
ALPHA0, BETA0 = 0.2, 2.0                     # every gene of a valid input, unless a case says otherwise


def kernel_constants():
    """The launch constants the shapes below are chosen against, read from the sources."""
    def src(name):
        with open(os.path.join(ROOT, "prosstt_amd", "csrc", name)) as f:
            return f.read()
    hip, heavy = src("prosstt_amd.hip"), src("k3_heavy.h")
    flags = re.search(r"row_flags_kernel<<<dim3\(\(unsigned\)\(rows < (\d+) \? rows : (\d+)\)\), dim3\((\d+)\)", hip)
    prep = re.search(r"prep_kernel<<<dim3\(\(unsigned\)\(\(span \+ (\d+)\) / (\d+)\)\), dim3\((\d+)\)", hip)
    grid = re.search(r"heavy_blocks = \(unsigned\)\(region_blocks < (\d+)u \? (\d+)u", hip)
    block = re.search(r"constexpr int kHeavyBlock = (\d+);", heavy)
    assert flags and prep and grid and block, "the launch lines this test reads its constants from have changed"
    assert flags.group(1) == flags.group(2) and int(prep.group(1)) + 1 == int(prep.group(2)) == int(prep.group(3))
    assert grid.group(1) == grid.group(2)
    return dict(flag_rows=int(flags.group(1)), flag_threads=int(flags.group(3)), prep_threads=int(prep.group(3)),
                heavy_min_grid=int(grid.group(1)), heavy_block=int(block.group(1)))


K = kernel_constants()


# ---- cases --------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=4)
def _base_means(rows, G):
    """Valid means in [0.5, 4): with scalings in [0.5, 2) every m lies in [0.25, 8)."""
    return np.random.default_rng(1000003 * rows + G).uniform(0.5, 4.0, (rows, G)).astype(np.float32)


@functools.lru_cache(maxsize=16)
def _base_scaling(N):
    return np.random.default_rng(N).uniform(0.5, 2.0, N)


@dataclass(frozen=True)
class Case:
    """One valid input and one value to plant in it.

    plant        ("means", (row, gene), value) | ("scaling", cell, value) | ("params", gene, (alpha, beta)) |
                 ("roc", cell, row index), or a tuple of several of these that are planted together
    roc          row of every cell (default: cell n uses row n % rows)
    genes        ((gene, alpha, beta), ...): genes of the VALID input that differ from (ALPHA0, BETA0)
    columns      ((gene, mean), ...): columns of the valid mean tensor set to one value
    cells        ((cell, scaling), ...): scalings of the valid input set to a value
    params       "host": alpha and beta are given as host arrays (the host decides PARAMS_NONNEG); "device": as device
                 tensors (only prep_kernel looks at them)
    abi          also run through the C ABI with host pointers"""
    name: str
    rows: int
    G: int
    N: int
    plant: tuple
    roc: tuple = None
    genes: tuple = ()
    columns: tuple = ()
    cells: tuple = ()
    params: str = "host"
    abi: bool = False

    @property
    def plants(self):
        return self.plant if isinstance(self.plant[0], tuple) else (self.plant,)

    def inputs(self, planted):
        """dict(means float32 (rows, G), roc int32 (N,), scaling, alpha, beta float64) -- fresh arrays where a case
        writes, the shared valid arrays elsewhere (never modified)."""
        means = _base_means(self.rows, self.G)
        scaling = _base_scaling(self.N)
        roc = (np.arange(self.N) % self.rows if self.roc is None else np.array(self.roc)).astype(np.int32)
        alpha, beta = np.full(self.G, ALPHA0), np.full(self.G, BETA0)
        for g, a, b in self.genes:
            alpha[g], beta[g] = a, b
        fields = {p[0] for p in self.plants} if planted else ()
        if self.columns or "means" in fields:
            means = means.copy()
        for g, value in self.columns:
            means[:, g] = value
        if self.cells or "scaling" in fields:
            scaling = scaling.copy()
        for n, value in self.cells:
            scaling[n] = value
        for field, where, value in (self.plants if planted else ()):
            if field == "means":
                means[where] = value
            elif field == "scaling":
                scaling[where] = value
            elif field == "params":
                alpha[where], beta[where] = value
            else:
                roc[where] = value
        return dict(means=means, roc=roc, scaling=scaling, alpha=alpha, beta=beta)

    def expected(self):
        """"einval" | "domain" | None: what the planted input must give."""
        from oracle import ref_numpy
        x = self.inputs(True)
        if self.N and (x["roc"].min() < 0 or x["roc"].max() >= self.rows):
            return "einval"
        return "domain" if ref_numpy.domain_error(x["means"], x["roc"], x["scaling"], x["alpha"], x["beta"]) else None


def _tag(v):
    return repr(v).replace(" ", "").replace("(", "").replace(")", "").replace(",", "_")


def _where(size, *more):
    """0, size - 1 and the given further indices, where they exist (each once)."""
    return sorted({i for i in (0, size - 1) + more if 0 <= i < size})


def build_cases():
    cases = []
    T = K["flag_threads"]
    assert T == K["prep_threads"] == K["heavy_block"] == 256 and K["flag_rows"] == 65536 and K["heavy_min_grid"] == 256, \
        "the shapes below were chosen for these launch constants: choose them again"

    # -- values: every entry of the three lists at one place (a cell whose scaling is exactly 1, so m = M), alpha and
    #    beta once as host arrays and once as device tensors
    for params in ("host", "device"):
        for i, v in enumerate(MEAN_VALUES):
            cases.append(Case("value-mean-%s-%s" % (_tag(v), params), 3, 8, 3, ("means", (1, 5), v), cells=((1, 1.0),),
                              params=params, abi=params == "host"))
        for v in SCALING_VALUES:
            cases.append(Case("value-scaling-%s-%s" % (_tag(v), params), 3, 8, 3, ("scaling", 2, v), params=params,
                              abi=params == "host"))
        for v in PARAM_VALUES:
            cases.append(Case("value-params-%s-%s" % (_tag(v), params), 3, 8, 3, ("params", 6, v), params=params,
                              abi=params == "host"))
    # ... and the product that underflows binary32 (1e-30 * 1e-10 is a binary32 denormal, 1e-30 * 1e-20 is 0) while both
    # factors are positive: valid in binary64, with and without another gene that asks for the per-sample pass
    for s in (1e-10, 1e-20):
        for genes, label in (((), "rowflags"), (((2, -0.1, 2.0),), "persample")):
            for params in ("host", "device"):
                cases.append(Case("value-product-1e-30x%s-%s-%s" % (_tag(s), label, params), 3, 8, 3, ("scaling", 1, s),
                                  columns=((5, 1e-30),), genes=genes, params=params, abi=params == "host"))
    # the same two ways for a scaling below binary32's range
    cases.append(Case("value-scaling-1e-50-persample-host", 3, 8, 3, ("scaling", 2, 1e-50), genes=((2, -0.1, 2.0),), abi=True))
    cases.append(Case("value-scaling-1e-50-persample-device", 3, 8, 3, ("scaling", 2, 1e-50), genes=((2, -0.1, 2.0),),
                      params="device"))
    # an infinite mean that only the per-sample pass could have caught through theta (alpha < 0: theta = -inf) and one it
    # cannot (alpha = 0: theta = NaN)
    for a in (-0.1, 0.0):
        cases.append(Case("value-mean-inf-persample-alpha%s" % _tag(a), 3, 8, 3, ("means", (1, 5), float("inf")),
                          genes=((5, a, 2.0), (2, -0.1, 2.0)), cells=((1, 1.0),), params="device"))

    # -- row_flags_kernel: a thread's loop over the genes runs 1, 2 and 5 times
    for G in (1, 3, 4, T - 1, T, T + 1, 4 * T + 1):
        for g in _where(G, T):
            for v in (0.0, float("inf")):
                cases.append(Case("rowflags-G%d-gene%d-%s" % (G, g, _tag(v)), 3, G, 3, ("means", (2, g), v),
                                  abi=(G in (T + 1, 4 * T + 1))))
    # ... and the grid-stride over the rows takes a second step; the offending row used by a cell, and by none
    for rows in (1, 3, K["flag_rows"] + 4):
        for r in _where(rows, K["flag_rows"]):
            others = [q for q in _where(rows, K["flag_rows"], 1) if q != r]
            for v in (0.0, float("inf")):
                cases.append(Case("rowflags-rows%d-row%d-%s-used" % (rows, r, _tag(v)), rows, 4, 3, ("means", (r, 3), v),
                                  roc=tuple((others[:1] or [r]) + [r] + (others[:1] or [r])), abi=(rows > 3 and v != 0.0)))
                if others:
                    cases.append(Case("rowflags-rows%d-row%d-%s-unused" % (rows, r, _tag(v)), rows, 4, 3,
                                      ("means", (r, 3), v), roc=tuple((others * 3)[:3])))

    # -- prep_kernel: one thread per index below max(N + 4, G), N + 4 > G and G > N + 4, more than one block of each
    for N in (1, T - 1, T, T + 1, 1000):
        for G in (3, T + 1, 4 * T + 1):
            for n in _where(N, T):
                for v in (0.0, float("nan")):
                    cases.append(Case("prep-N%d-G%d-cell%d-scaling-%s" % (N, G, n, _tag(v)), 5, G, N, ("scaling", n, v),
                                      params="device" if (N + G + n) % 2 else "host", abi=(N == T + 1 and G == T + 1)))
            for g in _where(G, T):
                for v in ((0.0, 0.5), (-0.1, 1.0)):
                    cases.append(Case("prep-N%d-G%d-gene%d-params-%s" % (N, G, g, _tag(v)), 5, G, N, ("params", g, v),
                                      params="device" if (N + G + g) % 2 else "host", abi=(N == T + 1 and G == T + 1)))
    # a row index outside the tensor is EINVAL, and wins over a domain error of the same call (cell 0's scaling, a gene
    # with beta < 1 whose per-sample pass must then not read through the index)
    for N, n, r in ((1, 0, -1), (T + 1, T, 5), (T + 1, 0, -1), (1000, 999, 5), (1000, T, 2 ** 31 - 1)):
        cases.append(Case("prep-N%d-cell%d-row%d-alone" % (N, n, r), 5, 3, N, ("roc", n, r), abi=(N == T + 1)))
        cases.append(Case("prep-N%d-cell%d-row%d-with-domain-error" % (N, n, r), 5, 3, N,
                          (("roc", n, r), ("scaling", (n + 1) % N, 0.0), ("params", 1, (0.0, 0.5))), params="device"))

    # -- the per-sample pass: a block takes four cells (N = 1000 over 256 blocks), a thread three or four genes; exactly
    #    one sample with theta < 0.  The valid input is the mirror case: a gene with alpha < 0 (or beta < 1) whose theta
    #    is positive in every cell.  Every cell has its own row, so that one entry of the tensor is one sample.
    B, grid, N = K["heavy_block"], K["heavy_min_grid"], 1000
    for G in (3 * B, 3 * B + 9):
        spots = [(0, 0), (N - 1, G - 1), (grid + 5, 3), (2 * grid + 7, 3), (2, B + 3), (2, 2 * B + 9),
                 (2 * grid + 7, 2 * B + 9), (3 * grid + 1, G - 1)]
        for i, (n, g) in enumerate(spots):
            # alpha < 0: theta = 1 - 0.1 m, the column holds m = 1 * s in [0.5, 2), the planted mean 50 / s gives m = 50
            cases.append(Case("persample-G%d-cell%d-gene%d-negalpha" % (G, n, g), N, G, N, ("means", (n, g), 50.0),
                              genes=((g, -0.1, 2.0),), columns=((g, 1.0),), params="device" if i % 2 else "host",
                              abi=(i in (1, 6))))
            # beta < 1: theta = 0.2 m - 0.5, the column holds m = 10 * s in [5, 20), the planted mean 0.5 gives m < 1
            cases.append(Case("persample-G%d-cell%d-gene%d-betabelow1" % (G, n, g), N, G, N, ("means", (n, g), 0.5),
                              genes=((g, 0.2, 0.5),), columns=((g, 10.0),), params="host" if i % 2 else "device"))
    assert len({c.name for c in cases}) == len(cases)
    assert all(c.roc is None or len(c.roc) == c.N for c in cases)
    return cases


CASES = build_cases()
ABI_CASES = [c for c in CASES if c.abi]


# ---- running a case -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx():
    """A context of its own: the sequences below count its calls."""
    from prosstt_amd import device
    c = device.Context()
    yield c
    c.close()


def _params(ctx, case, x):
    import torch
    if case.params == "device":
        return ctx.tensor(x["alpha"], torch.float64), ctx.tensor(x["beta"], torch.float64)
    return x["alpha"], x["beta"]


def verdict(ctx, case, x, mode, **kw):
    """"domain" | "einval" | None of one checked call on ``ctx``: mode True (synchronous) or "deferred"."""
    from prosstt_amd import _native
    alpha, beta = _params(ctx, case, x)
    try:
        ctx.sample_counts(x["means"], x["roc"], x["scaling"], alpha, beta, seed=11, check_domain=mode, **kw)
        if mode == "deferred":
            ctx.domain_status()
    except ValueError as exc:
        assert "Domain error" in str(exc), exc            # (the library's verdict, not a refused argument)
        return "domain"
    except _native.NativeError as exc:
        assert exc.code == _native.EINVAL, exc
        return "einval"
    return None


def _run(ctx, case, mode):
    good, bad = case.inputs(False), case.inputs(True)
    assert verdict(ctx, case, good, mode) is None, "the valid input was refused"
    want = case.expected()
    got = verdict(ctx, case, bad, mode)
    assert got == want, "planted %r: the device says %r, the reference's rule %r" % (case.plant, got, want)
    assert verdict(ctx, case, good, mode) is None, "the verdict outlived the offending value"
    ctx.domain_status()                       # nothing is left behind


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_synchronous_verdict(ctx, case):
    _run(ctx, case, True)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_deferred_verdict(ctx, case):
    _run(ctx, case, "deferred")


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.fixture(scope="module")
def abi():
    from prosstt_amd import _native
    L = _native.load()
    handle = ctypes.c_void_p()
    assert L.prosstt_amd_ctx_create(0, None, ctypes.byref(handle)) == 0
    yield L, handle
    L.prosstt_amd_ctx_destroy(handle)


@pytest.mark.parametrize("case", ABI_CASES, ids=lambda c: c.name)
def test_host_pointer_verdict(abi, case):
    """The same through ``prosstt_amd_sample_counts`` with HOST_INPUTS | HOST_OUTPUT | CHECK_DOMAIN (the row index is then
    checked on the host), and the deferred form read through ``prosstt_amd_domain_status``."""
    from prosstt_amd import _native
    L, handle = abi
    codes = {None: 0, "domain": _native.EDOMAIN, "einval": _native.EINVAL}

    def call(x, flag):
        out = np.empty((case.N, case.G), np.int32)
        return L.prosstt_amd_sample_counts(
            handle, _ptr(x["means"]), case.rows, case.G, _ptr(x["roc"]), _ptr(x["scaling"]), _ptr(x["alpha"]),
            _ptr(x["beta"]), case.N, ctypes.c_uint64(3), ctypes.c_uint64(0), None, _ptr(out), case.G,
            _native.HOST_INPUTS | _native.HOST_OUTPUT | flag)

    def status():
        word = ctypes.c_int32(-1)
        assert L.prosstt_amd_domain_status(handle, ctypes.byref(word)) == 0
        return word.value

    good, bad, want = case.inputs(False), case.inputs(True), codes[case.expected()]
    assert call(good, _native.CHECK_DOMAIN) == 0
    assert call(bad, _native.CHECK_DOMAIN) == want, L.prosstt_amd_last_error()
    assert call(good, _native.CHECK_DOMAIN) == 0 and status() == 0
    if want != _native.EINVAL:                                   # (refused on the host before anything is enqueued)
        assert call(bad, _native.CHECK_DEFERRED) == 0 and status() == want
        assert status() == 0 and call(good, _native.CHECK_DEFERRED) == 0 and status() == 0


# ---- sequences on one context ---------------------------------------------------------------------------------------------

def _case(name):
    return next(c for c in CASES if c.name == name)


def test_alternating_good_and_bad_calls_both_parities(ctx):
    """The request for the per-sample pass lives in one of two words, by the parity of the call: a requesting and a
    non-requesting call on either parity, in both orders, synchronous and deferred."""
    case = _case("persample-G768-cell261-gene3-negalpha")
    plain = _case("prep-N257-G257-cell256-scaling-0.0")
    good, bad = case.inputs(False), case.inputs(True)
    for mode in (True, "deferred"):
        for first in (0, 1):                                  # (an extra call shifts the parity of everything behind it)
            for _ in range(first):
                assert verdict(ctx, plain, plain.inputs(False), mode) is None
            seen = [verdict(ctx, case, bad if i % 2 else good, mode) for i in range(6)]
            assert seen == [None, "domain"] * 3, (mode, first, seen)
            # a call that asks for no per-sample pass behind one that did: the request has not outlived its call
            assert verdict(ctx, plain, plain.inputs(False), mode) is None
            assert verdict(ctx, case, bad, mode) == "domain"
            assert verdict(ctx, plain, plain.inputs(False), mode) is None
    ctx.domain_status()


def test_unchecked_and_empty_calls_between_checked_ones(ctx):
    case = _case("persample-G768-cell261-gene3-negalpha")
    good, bad = case.inputs(False), case.inputs(True)
    # an unchecked call between two deferred ones neither sets nor clears anything
    for middle in (good, bad):
        ctx.sample_counts(good["means"], good["roc"], good["scaling"], good["alpha"], good["beta"], seed=1, check_domain="deferred")
        ctx.sample_counts(middle["means"], middle["roc"], middle["scaling"], middle["alpha"], middle["beta"], seed=1,
                          check_domain=False)
        ctx.sample_counts(good["means"], good["roc"], good["scaling"], good["alpha"], good["beta"], seed=1, check_domain="deferred")
        ctx.domain_status()
    ctx.sample_counts(bad["means"], bad["roc"], bad["scaling"], bad["alpha"], bad["beta"], seed=1, check_domain="deferred")
    ctx.sample_counts(good["means"], good["roc"], good["scaling"], good["alpha"], good["beta"], seed=1, check_domain=False)
    with pytest.raises(ValueError):
        ctx.domain_status()
    ctx.domain_status()
    # an empty call with beta < 1 has no sample to refuse and leaves no request for the call behind it
    for mode in (True, "deferred"):
        none = ctx.sample_counts(good["means"], good["roc"][:0], good["scaling"][:0], np.zeros(case.G), np.full(case.G, 0.5),
                                 seed=1, check_domain=mode)
        assert tuple(none.shape) == (0, case.G)
        assert verdict(ctx, case, good, mode) is None
    # three deferred calls, only the middle one bad: one raise, then a clean status
    for x in (good, bad, good):
        ctx.sample_counts(x["means"], x["roc"], x["scaling"], x["alpha"], x["beta"], seed=1, check_domain="deferred")
    with pytest.raises(ValueError):
        ctx.domain_status()
    ctx.domain_status()


def test_cached_row_flags_follow_tensor_and_token(ctx):
    """``means_token``: the documented contract of the cached per-row flags of the mean tensor."""
    import torch
    from prosstt_amd import _native
    G = 4
    al, be = np.full(G, ALPHA0), np.full(G, BETA0)
    means = torch.ones((3, G), dtype=torch.float32, device=ctx.torch_device)
    roc, sc = np.arange(3, dtype=np.int32), np.ones(3)

    def call(m, token, r=roc, s=sc, mode=True):
        ctx.sample_counts(m, r, s, al, be, seed=2, check_domain=mode, means_token=token)

    call(means, "a")
    means[2, 1] = 0.0
    call(means, "a")                          # not announced: the old flags are reused (the documented contract)
    with pytest.raises(ValueError):
        call(means, "b")                      # a new token rescans
    assert ctx._checked_means is None         # a refused call leaves no cached key behind ...
    with pytest.raises(ValueError):
        call(means, "b")                      # ... so the same token scans again and finds it again
    means[2, 1] = 1.0
    call(means, "b")
    # another tensor of the same shape under the same token is not the tensor the flags belong to
    other = torch.ones((3, G), dtype=torch.float32, device=ctx.torch_device)
    other[0, 3] = 0.0
    assert other.data_ptr() != means.data_ptr()
    with pytest.raises(ValueError):
        call(other, "b")
    call(means, "b")
    # more rows than the flag buffer holds (it grows in steps of 4096): the last row's flag is where it belongs
    rows = 4096 * 3 + 5
    big = torch.ones((rows, G), dtype=torch.float32, device=ctx.torch_device)
    far = np.array([0, rows - 1, 4096], np.int32)
    call(big, "c", r=far)
    call(big, "c", r=far)
    big[rows - 1, 0] = float("nan")
    with pytest.raises(ValueError):
        call(big, "d", r=far)
    call(big, "e", r=far[[0, 2, 2]])          # the row is bad, but no cell uses it
    call(big, "e", r=far, mode="deferred")    # same token: the flags of the scan above, and now a cell does
    with pytest.raises(ValueError):
        ctx.domain_status()
    ctx.domain_status()
    # a row index outside the tensor under a token: EINVAL, no cached key
    with pytest.raises(_native.NativeError):
        call(means, "b", r=np.array([0, 3, 1], np.int32))
    assert ctx._checked_means is None
    call(means, "b")


# ---- the same through the host API ----------------------------------------------------------------------------------------

G_TREE = 40
HOST_RETURNS = [("numpy", "presented"), ("numpy32", "presented"), ("numpy16", "presented"), ("csr", "presented"),
                ("torch", "presented"), ("torch", "plan")]


def _tiny_tree():
    from prosstt_amd.tree import Tree
    t = Tree(topology=[["A", "B"], ["A", "C"]], time={"A": 6, "B": 5, "C": 7}, num_branches=3, branch_points=1,
             modules=5, G=G_TREE)
    rng = np.random.default_rng(5)
    t.add_genes({b: rng.uniform(0.5, 30.0, (int(t.time[b]), G_TREE)) for b in t.branches})
    return t


def _stacked(t):
    """The mean tensor the device holds, from the host dict."""
    return np.concatenate([np.asarray(t.means[b]) for b in t.branches]).astype(np.float32)


def _dense(result):
    from prosstt_amd import device
    if isinstance(result, device.PresentedCounts):
        return result.in_plan_order().cpu().numpy()
    if hasattr(result, "toarray"):
        return result.toarray()
    return result.cpu().numpy() if hasattr(result, "cpu") else np.asarray(result)


def _strict_and_not(ctx, call):
    """``call(strict)`` raises with strict=True and returns with strict=False; neither leaves a verdict in the context."""
    with pytest.raises(ValueError):
        call(True)
    ctx.domain_status()
    out = call(False)
    ctx.domain_status()
    return out


@pytest.mark.parametrize("how", ["in-place", "fresh-array"])
def test_draw_counts_sees_an_edited_mean_in_every_return_form(how):
    from oracle import nb_model, ref_numpy
    from prosstt_amd import device
    from prosstt_amd import simulation as sim
    ctx = device.get_context()
    ctx.domain_status()
    al, be = np.full(G_TREE, ALPHA0), np.full(G_TREE, BETA0)
    t = _tiny_tree()
    pt, br = (np.asarray(v) for v in sim.cover_whole_tree(t))
    sc = np.random.default_rng(9).uniform(0.5, 2.0, len(pt))
    rows = sim.cell_rows(t, pt, br)
    clean = sim.draw_counts(t, pt, br, sc, al, be, seed=21, out="numpy32")
    assert not ref_numpy.domain_error(_stacked(t), rows, sc, al, be)
    assert np.array_equal(clean, nb_model.sample_counts(_stacked(t), rows, sc, al, be, 21))
    kept = t.means["B"][2, 7]
    if how == "in-place":
        t.means["B"][2, 7] = 0.0
    else:
        fresh = np.array(t.means["B"])
        fresh[2, 7] = 0.0
        t.means["B"] = fresh
    assert ref_numpy.domain_error(_stacked(t), rows, sc, al, be)
    hit = np.zeros(clean.shape, bool)
    hit[rows == t.row_offsets()[0]["B"] + 2, 7] = True
    assert hit.any()
    for out, order in HOST_RETURNS:
        got = _dense(_strict_and_not(ctx, lambda strict: sim.draw_counts(t, pt, br, sc, al, be, seed=21, out=out, order=order,
                                                                         strict=strict)))
        # unchecked: 0 for the samples the reference refuses, every other count as before
        assert (got[hit] == 0).all() and np.array_equal(got[~hit], clean[~hit]), (out, order)
    # repaired: the counts of a context that never saw the error
    t.means["B"][2, 7] = kept
    for out, order in HOST_RETURNS:
        assert np.array_equal(_dense(sim.draw_counts(t, pt, br, sc, al, be, seed=21, out=out, order=order)), clean)
    ctx.domain_status()


def test_plan_drawing_entry_points_raise_and_leave_nothing_behind():
    from oracle import ref_numpy
    from prosstt_amd import device
    from prosstt_amd import parallel
    from prosstt_amd import simulation as sim
    from prosstt_amd import summary
    ctx = device.get_context()
    ctx.domain_status()
    al, be = np.full(G_TREE, ALPHA0), np.full(G_TREE, BETA0)
    t = _tiny_tree()
    state = np.random.get_state()

    def seeded(fn):
        def call(strict):
            np.random.seed(33)
            return fn(strict)
        return call

    cells, chunk = 20, 7
    density = seeded(lambda strict: sim.sample_density(t, cells, alpha=al, beta=be, seed=3, out="numpy32", strict=strict))
    chunks = seeded(lambda strict: list(sim.sample_density_chunks(t, cells, chunk, alpha=al, beta=be, seed=3, strict=strict)))
    # (no process group: the one rank owns every cell)
    sharded = seeded(lambda strict: parallel.sample_density_sharded(t, cells, alpha=al, beta=be, seed=3, strict=strict))
    gathered = seeded(lambda strict: parallel.sample_and_gather(t, cells, alpha=al, beta=be, seed=3, chunk_cells=chunk,
                                                                strict=strict))
    clean, pt, br, sc = density(True)
    rows = sim.cell_rows(t, pt, br)
    stacked = _stacked(t)
    # a cell of the first, the middle and the last chunk that is the only user of its row of the mean tensor
    alone = [n for n in range(cells) if (rows == rows[n]).sum() == 1]
    targets = [next(n for n in alone if n // chunk == k) for k in range(3)]
    assert -(-cells // chunk) == 3
    offsets = t.row_offsets()[0]
    for k, n in enumerate(targets):
        label = str(br[n])
        at = (int(rows[n]) - offsets[label], 11)
        kept = t.means[label][at]
        t.means[label][at] = 0.0
        stacked_bad = _stacked(t)
        assert ref_numpy.domain_error(stacked_bad, rows, sc, al, be)
        assert not ref_numpy.domain_error(stacked_bad, np.delete(rows, n), np.delete(sc, n), al, be)
        got = _strict_and_not(ctx, density)
        assert got[0][n, 11] == 0 and np.array_equal(np.delete(got[0], n, axis=0), np.delete(clean, n, axis=0))
        parts = _strict_and_not(ctx, chunks)
        assert np.array_equal(np.concatenate([p[0] for p in parts]), got[0])
        # the same plan (same numpy seed, same draws) through the sharded pair and the pipeline, brought to plan order
        counts, mine = _strict_and_not(ctx, sharded)[:2]
        assert np.array_equal(parallel.gather_rows(counts, mine, cells).cpu().numpy(), got[0])
        full, cell_of_row = _strict_and_not(ctx, gathered)[:2]
        assert np.array_equal(device.to_plan_order(cell_of_row, full.cpu().numpy())[0], got[0])
        # the chunks that were served before the raise held no refused sample: chunk i + 1 is enqueued before the
        # verdict behind chunk i is read, so the raise comes with the offending chunk or the one before it
        np.random.seed(33)
        served = 0
        with pytest.raises(ValueError):
            for part in sim.sample_density_chunks(t, cells, chunk, alpha=al, beta=be, seed=3):
                served += 1
        assert max(0, k - 1) <= served <= k
        ctx.domain_status()
        _strict_and_not(ctx, seeded(lambda strict: summary.sample_density_summary(t, cells, alpha=al, beta=be, chunk_cells=chunk,
                                                                                 seed=3, strict=strict)))
        if k == 2:
            # the generator dropped after its first chunk, while the launch behind it is still unread
            np.random.seed(33)
            gen = sim.sample_density_chunks(t, cells, chunk, alpha=al, beta=be, seed=3)
            assert np.array_equal(next(gen)[0], clean[:chunk])
            gen.close()
            ctx.domain_status()
        t.means[label][at] = kept
        again = density(True)
        assert np.array_equal(again[0], clean)
        assert np.array_equal(np.concatenate([p[0] for p in chunks(True)]), clean)
    # every position of the tree is used
    t.means["C"][6, G_TREE - 1] = 0.0
    whole = _strict_and_not(ctx, seeded(lambda strict: sim.sample_whole_tree(t, 2, alpha=al, beta=be, seed=3, strict=strict)))
    assert whole[0].shape == (2 * 18, G_TREE)
    np.random.set_state(state)


def test_add_non_diff_genes_raises_and_leaves_nothing_behind():
    from oracle import nb_model
    from prosstt_amd import device
    from prosstt_amd import simulation as sim
    ctx = device.get_context()
    ctx.domain_status()
    params = dict(alpha=np.full(6, ALPHA0), beta=np.full(6, BETA0), base_expr=np.array([1.0, 2.0, 0.0, 4.0, 5.0, 6.0]))
    inform = np.ones((9, 4))
    wide = _strict_and_not(ctx, lambda strict: sim.add_non_diff_genes(inform, 6, params, np.ones(9), seed=8, strict=strict))
    assert wide.shape == (9, 10) and (wide[:, 6] == 0).all()
    params["base_expr"][2] = 3.0
    repaired = sim.add_non_diff_genes(inform, 6, params, np.ones(9), seed=8)
    assert np.array_equal(np.delete(repaired, 6, axis=1), np.delete(wide, 6, axis=1))
    want = nb_model.sample_counts(params["base_expr"][None].astype(np.float32), np.zeros(9, np.int32), np.ones(9),
                                  params["alpha"], params["beta"], 8)
    assert np.array_equal(repaired[:, 4:], want)
    ctx.domain_status()
