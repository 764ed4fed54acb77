"""
Thin object layer over the C ABI: one ``Context`` per (device, stream).

torch supplies device memory and the stream handle; every numeric step is a
call into libprosstt_amd.so.  Nothing here computes on the CPU.
"""
import ctypes
import os
import threading
import warnings
import weakref

import numpy as np

from . import _native


def _torch():
    import torch
    return torch


def require_gpu():
    """Raise unless the HIP library loads and a gfx950 device is visible."""
    _native.load()
    torch = _torch()
    if not torch.cuda.is_available() or _native.device_count() == 0:
        raise RuntimeError("prosstt_amd needs an AMD MI355X (gfx950) device: there is no CPU fallback")


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def need_device(name):
    """Library ``name`` of _native.LIBRARIES, loaded; RuntimeError unless a device is visible."""
    L = _native.load(name)
    if not _torch().cuda.is_available():
        raise RuntimeError("prosstt_amd needs an AMD MI355X (gfx950) device: there is no CPU fallback")
    return L


def current_stream(dev):
    """torch's current stream on ``dev``, as the C ABI takes it."""
    return ctypes.c_void_p(_torch().cuda.current_stream(dev).cuda_stream)


def workspace(name, query_symbol, dev, *sizes):
    """A uint8 tensor on ``dev`` of the bytes that library ``name``'s ``*_workspace_bytes`` (``query_symbol``) asks for
    ``sizes``."""
    need = ctypes.c_uint64(0)
    _native.check(getattr(_native.load(name), query_symbol)(*sizes, ctypes.byref(need)), name)
    return _torch().empty(max(int(need.value), 1), dtype=_torch().uint8, device=dev)


class Context:
    """Owns a prosstt_amd_ctx bound to ``device`` and to torch's current stream there."""

    def __init__(self, device=None):
        require_gpu()
        torch = _torch()
        self.device = torch.cuda.current_device() if device is None else int(device)
        self.torch_device = torch.device("cuda", self.device)
        self.stream = torch.cuda.current_stream(self.device)
        self._lib = _native.load()
        handle = ctypes.c_void_p()
        _native.check(self._lib.prosstt_amd_ctx_create(
            self.device, ctypes.c_void_p(self.stream.cuda_stream), ctypes.byref(handle)))
        self._h = handle
        self._checked_means = None      # (pointer, rows, G, token) of the mean tensor whose row flags the ctx holds

    def close(self):
        if getattr(self, "_h", None):
            self._lib.prosstt_amd_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- helpers ------------------------------------------------------------
    def tensor(self, array, dtype):
        """Host array (or tensor) -> contiguous device tensor of ``dtype``."""
        torch = _torch()
        if isinstance(array, torch.Tensor):
            return array.to(device=self.torch_device, dtype=dtype).contiguous()
        host = np.ascontiguousarray(array)
        if not host.flags.writeable:               # e.g. a broadcast view: torch wants an owned buffer
            host = host.copy()
        return torch.as_tensor(host, dtype=dtype).to(self.torch_device)

    def synchronize(self):
        _native.check(self._lib.prosstt_amd_ctx_synchronize(self._h))

    def last_kernel_ms(self):
        ms = ctypes.c_float(0)
        _native.check(self._lib.prosstt_amd_last_kernel_ms(self._h, ctypes.byref(ms)))
        return ms.value

    # ---- K3: fused count sampler -------------------------------------------
    def sample_counts(self, means, row_of_cell, scaling, alpha, beta, seed, cell_offset=0,
                      out=None, check_domain=True, time_kernel=False, cell_index=None, means_token=None):
        """int32 device tensor (N, G) of counts; see prosstt_amd_sample_counts.

        check_domain  True: the reference's argument check, raised here (ValueError; synchronises);
                      "deferred": the same check, enqueued with the call and not waited for -- the verdict is
                      raised by the next ``domain_status()`` (the host-returning entry points call it behind the
                      copy that synchronises anyway); False: no check.
        means_token   any hashable that changes whenever the content of ``means`` does (the host layer passes the
                      tree's fingerprint): with the same tensor and token as the previous checked call the per-row
                      flags of the mean tensor are reused instead of rescanned."""
        torch = _torch()
        means = self.tensor(means, torch.float32)
        rows, G = means.shape
        row_of_cell = self.tensor(row_of_cell, torch.int32)
        N = row_of_cell.numel()
        scaling = self.tensor(scaling, torch.float64)
        nonneg = bool(check_domain) and self._params_nonneg(alpha, beta)
        alpha = self.tensor(alpha, torch.float64)
        beta = self.tensor(beta, torch.float64)
        if scaling.numel() != N or alpha.numel() != G or beta.numel() != G:
            raise ValueError("scaling must have one entry per cell, alpha/beta one per gene")
        if out is None:
            out = torch.empty((N, G), dtype=torch.int32, device=self.torch_device)
        elif out.dtype != torch.int32 or out.shape != (N, G) or out.stride(1) != 1:
            raise ValueError("out must be an int32 (N, G) tensor with unit column stride")
        if cell_index is not None:
            cell_index = self.tensor(cell_index, torch.int64)
            if cell_index.numel() != N:
                raise ValueError("cell_index must have one entry per cell")
        # (row_of_cell indexes the mean tensor unchecked in the kernels -- device pointers are the caller's
        # contract in the C ABI; with check_domain the library's domain pass also reports an index outside
        # the tensor, as PROSSTT_AMD_EINVAL)
        if check_domain not in (True, False, "deferred"):
            raise ValueError("check_domain must be True, False or 'deferred'")
        flags = _native.TIME_KERNEL if time_kernel else 0
        if check_domain:
            flags |= _native.CHECK_DEFERRED if check_domain == "deferred" else _native.CHECK_DOMAIN
            if nonneg:
                flags |= _native.PARAMS_NONNEG
            key = (means.data_ptr(), rows, G, means_token)
            if means_token is not None and key == self._checked_means:
                flags |= _native.MEANS_CACHED
            self._checked_means = None              # the ctx holds this tensor's row flags only once the call has gone through
        _native.check(self._lib.prosstt_amd_sample_counts(
            self._h, _ptr(means), rows, G, _ptr(row_of_cell), _ptr(scaling), _ptr(alpha), _ptr(beta),
            N, ctypes.c_uint64(seed & (2 ** 64 - 1)), ctypes.c_uint64(cell_offset), _ptr(cell_index),
            _ptr(out), out.stride(0) if N else G, flags))
        if check_domain and N and G and means_token is not None:
            self._checked_means = key
        return out

    def _params_nonneg(self, alpha, beta):
        """alpha >= 0 and beta >= 1 for every gene, as far as the HOST can tell for free (then alpha*m + beta < 1 cannot
        happen and the checked call tells the library so: PROSSTT_AMD_PARAMS_NONNEG).  Host arrays are looked at here
        (O(G)).  Device tensors are not looked at at all: the preparation kernel tests them anyway and the per-sample
        pass at the end of the call's second kernel runs only if it found a gene with alpha < 0 or beta < 1 -- no torch
        kernel (whose first use in a process costs tens of milliseconds of code loading: tools/cold_probe.py), no cache
        of verdicts that could outlive its tensor."""
        torch = _torch()
        for arr, floor in ((alpha, 0.0), (beta, 1.0)):
            if isinstance(arr, torch.Tensor) or not bool(np.all(np.asarray(arr) >= floor)):
                return False
        return True

    def domain_status(self):
        """Raise what the ``check_domain="deferred"`` calls since the last time found (ValueError where the
        reference's scipy call raises, NativeError for a row index outside the tensor); synchronises."""
        status = ctypes.c_int32(0)
        _native.check(self._lib.prosstt_amd_domain_status(self._h, ctypes.byref(status)))
        _native.check(status.value)

    def last_list(self, cap=1 << 22):
        """(cells, genes, total, overflowed): the samples the streaming kernel of the last
        sample_counts call left to its second kernel (see prosstt_amd_last_list)."""
        cells = np.empty(cap, np.int64)
        genes = np.empty(cap, np.int32)
        total = ctypes.c_int64(0)
        over = ctypes.c_int32(0)
        _native.check(self._lib.prosstt_amd_last_list(
            self._h, cells.ctypes.data_as(ctypes.c_void_p), genes.ctypes.data_as(ctypes.c_void_p), cap,
            ctypes.byref(total), ctypes.byref(over)))
        n = min(cap, total.value)
        return cells[:n], genes[:n], total.value, bool(over.value)

    def last_run_plan(self):
        """(words, strip_cells): the run words of the cell records of the last sample_counts call (N + 4 of them) and
        the strip length of its launch (see prosstt_amd_last_run_plan and ``run_plan``)."""
        total = ctypes.c_int64(0)
        strip = ctypes.c_int32(0)
        _native.check(self._lib.prosstt_amd_last_run_plan(self._h, None, 0, ctypes.byref(total), ctypes.byref(strip)))
        words = np.empty(total.value, np.uint32)
        _native.check(self._lib.prosstt_amd_last_run_plan(
            self._h, words.ctypes.data_as(ctypes.c_void_p), words.size, ctypes.byref(total), ctypes.byref(strip)))
        return words, strip.value

    def last_strip_plan(self):
        """(classes, tiles_g, blocks): the strip plan of the last sample_counts call, as ``strip_plan`` gives it."""
        classes = np.zeros((4, 3), np.int32)
        n, tiles, blocks = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
        _native.check(self._lib.prosstt_amd_last_strip_plan(
            self._h, classes.ctypes.data_as(ctypes.c_void_p), ctypes.byref(n), ctypes.byref(tiles), ctypes.byref(blocks)))
        return classes[:n.value].copy(), tiles.value, blocks.value

    HW_OPS = dict(rcp=0, log2=1, exp2neg=2)

    def hw_math(self, op, first_bits, count):
        """float32 host array y[i] = f(as_float(first_bits + i)), i < count, of one of the three hardware
        functions of the sampler's definition ('rcp', 'log2', 'exp2neg'), computed by the device
        (prosstt_amd_hw_math): the tables the checking model is given."""
        out = np.empty(int(count), np.float32)
        _native.check(self._lib.prosstt_amd_hw_math(
            self._h, self.HW_OPS[op], ctypes.c_uint32(first_bits), ctypes.c_uint64(int(count)),
            out.ctypes.data_as(ctypes.c_void_p), _native.HOST_OUTPUT))
        return out

    HW_OPS_AT = dict(rcp=0, log2=1, exp2neg=2, sqrt=3, rsq=4, cos=5)

    def hw_math_at(self, op, x):
        """float32 host array y[i] = f(x[i]) of one of the hardware functions of the sampler's definition (a name of
        HW_OPS_AT or its code; 'cos' takes revolutions), computed by the device (prosstt_amd_hw_math_at): what the
        checking model asks while it evaluates the gamma-Poisson class."""
        x = np.ascontiguousarray(x, np.float32)
        out = np.empty(x.size, np.float32)
        code = self.HW_OPS_AT[op] if isinstance(op, str) else int(op)
        _native.check(self._lib.prosstt_amd_hw_math_at(
            self._h, code, x.ctypes.data_as(ctypes.c_void_p), ctypes.c_uint64(x.size),
            out.ctypes.data_as(ctypes.c_void_p), _native.HOST_OUTPUT | _native.HOST_INPUTS))
        return out

    def nb_params(self, means, row_of_cell, scaling, alpha, beta):
        """(mu, p, r, path) device tensors (N, G) -- the sampler's deterministic intermediates."""
        torch = _torch()
        means = self.tensor(means, torch.float32)
        rows, G = means.shape
        row_of_cell = self.tensor(row_of_cell, torch.int32)
        N = row_of_cell.numel()
        scaling = self.tensor(scaling, torch.float64)
        alpha = self.tensor(alpha, torch.float64)
        beta = self.tensor(beta, torch.float64)
        mu = torch.empty((N, G), dtype=torch.float32, device=self.torch_device)
        p = torch.empty_like(mu)
        r = torch.empty_like(mu)
        path = torch.empty((N, G), dtype=torch.int32, device=self.torch_device)
        _native.check(self._lib.prosstt_amd_nb_params(
            self._h, _ptr(means), rows, G, _ptr(row_of_cell), _ptr(scaling), _ptr(alpha), _ptr(beta),
            N, _ptr(mu), _ptr(p), _ptr(r), _ptr(path), 0))
        return mu, p, r, path

    # ---- K2: lineage ---------------------------------------------------------
    def lineage_attempt_batch(self, programs, H, sib_programs=()):
        """B attempts of one branch in one launch: ``programs`` is (B, T, K); returns
        (max(programs[b]@H) as (B,) float64, #genes with r<0 per sibling as (B, n_sib) int64)
        -- simulation.py:269-272 per attempt."""
        programs = np.ascontiguousarray(programs, np.float64)
        if programs.ndim != 3:
            raise ValueError("programs must be (B, T, K)")
        B, T, K = programs.shape
        H = self._coefficients(H, K)
        sibs = [np.ascontiguousarray(s, np.float64) for s in sib_programs]
        n = len(sibs)
        for s in sibs:
            if s.ndim != 2 or s.shape[1] != K:
                raise ValueError("sibling programs must have %d columns" % K)
        ptrs = (ctypes.c_void_p * max(n, 1))(*[s.ctypes.data for s in sibs])
        lens = (ctypes.c_int32 * max(n, 1))(*[s.shape[0] for s in sibs])
        top = np.empty(B, np.float64)
        counts = np.zeros((B, max(n, 1)), np.int64)
        _native.check(self._lib.prosstt_amd_lineage_attempt_batch(
            self._h, programs.ctypes.data_as(ctypes.c_void_p), B, T, K, _ptr(H), H.shape[1], n,
            ctypes.cast(ptrs, ctypes.c_void_p), ctypes.cast(lens, ctypes.c_void_p),
            top.ctypes.data_as(ctypes.c_void_p), counts.ctypes.data_as(ctypes.c_void_p)))
        return top, counts[:, :n]

    def lineage_attempt(self, programs, H, sib_programs=()):
        """(max(programs@H), [#genes with r<0 per sibling]) -- simulation.py:269-272."""
        top, counts = self.lineage_attempt_batch(np.asarray(programs, np.float64)[None], H, sib_programs)
        return float(top[0]), [int(c) for c in counts[0]]

    def lineage_walk(self, seed, stream_id, T, K):
        """(T, K) float64 expression programs drawn on the device (K1, PRLW-1)."""
        out = np.empty((T, K), np.float64)
        _native.check(self._lib.prosstt_amd_lineage_walk(
            self._h, ctypes.c_uint64(seed & (2 ** 64 - 1)), ctypes.c_uint64(stream_id), T, K,
            out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def lineage_walks(self, seed, stream_ids, T, K):
        """(B, T, K) programs of the walk streams ``stream_ids`` (consecutive ids: one launch, one copy back)."""
        ids = [int(i) for i in stream_ids]
        if not ids:
            return np.empty((0, T, K), np.float64)
        if ids != list(range(ids[0], ids[0] + len(ids))):
            return np.stack([self.lineage_walk(seed, i, T, K) for i in ids])
        out = np.empty((len(ids), T, K), np.float64)
        _native.check(self._lib.prosstt_amd_lineage_walk_batch(
            self._h, ctypes.c_uint64(seed & (2 ** 64 - 1)), ctypes.c_uint64(ids[0]), len(ids), T, K,
            out.ctypes.data_as(ctypes.c_void_p)))
        return out

    def lineage_commit(self, programs, H, rel_out=None, gene_max=None):
        """rel_out = programs @ H and gene_max = max(gene_max, max over rows of rel) on the device (either may be None);
        ``rel_out`` (T, G) and ``gene_max`` (G,) must be contiguous binary64 tensors on this context's device."""
        torch = _torch()
        programs = np.ascontiguousarray(programs, np.float64)
        if programs.ndim != 2:
            raise ValueError("programs must be (T, K)")
        T, K = programs.shape
        H = self._coefficients(H, K)
        G = H.shape[1]
        self._output(rel_out, "rel_out", torch.float64, (T, G))
        self._output(gene_max, "gene_max", torch.float64, (G,))
        _native.check(self._lib.prosstt_amd_lineage_commit(
            self._h, programs.ctypes.data_as(ctypes.c_void_p), T, K, _ptr(H), H.shape[1],
            _ptr(rel_out), _ptr(gene_max)))

    def gene_max(self, rel, gene_max):
        """gene_max[g] = max(gene_max[g], max over rows of rel[:, g]) -- sim_utils.py:423-425 in log space."""
        torch = _torch()
        rel = self.tensor(rel, torch.float64)
        if rel.dim() != 2:
            raise ValueError("rel must be (rows, G)")
        self._output(gene_max, "gene_max", torch.float64, (rel.shape[1],))
        if rel.numel():                           # (an empty tensor has no data pointer to pass)
            _native.check(self._lib.prosstt_amd_gene_max(self._h, _ptr(rel), rel.shape[0], rel.shape[1], _ptr(gene_max)))
        return gene_max

    def means_from_rel(self, rel, base, out=None):
        """float32 (rows, G) device tensor exp(rel) * base (one rounding of the binary64 value; a positive mean below
        binary32's smallest normal is stored as that); ``out`` must be a contiguous float32 tensor on this device."""
        torch = _torch()
        rel = self.tensor(rel, torch.float64)
        if rel.dim() != 2:
            raise ValueError("rel must be (rows, G)")
        rows, G = rel.shape
        base = self.tensor(base, torch.float64)
        if base.shape != (G,):
            raise ValueError("base must have one entry per gene")
        if out is None:
            out = torch.empty((rows, G), dtype=torch.float32, device=self.torch_device)
        self._output(out, "out", torch.float32, (rows, G))
        if out.numel():
            _native.check(self._lib.prosstt_amd_means_from_rel(self._h, _ptr(rel), _ptr(base), rows, G, _ptr(out)))
        return out

    def _coefficients(self, H, K):
        """H as a contiguous (K, G) binary64 device tensor (the kernels index it as H + k*G + g)."""
        H = self.tensor(H, _torch().float64)
        if H.dim() != 2 or H.shape[0] != K or H.shape[1] == 0:
            raise ValueError("H must be (%d, G >= 1), not %s" % (K, tuple(H.shape)))
        return H

    def _output(self, t, name, dtype, shape):
        """Refuse (on the host, before any launch) an output the kernels could not write as they index it."""
        if t is None:
            return
        torch = _torch()
        if not isinstance(t, torch.Tensor):
            raise TypeError("%s must be a torch tensor on %s" % (name, self.torch_device))
        if t.device != self.torch_device:
            raise ValueError("%s is on %s, not on %s" % (name, t.device, self.torch_device))
        if t.dtype != dtype:
            raise TypeError("%s must be %s, not %s" % (name, dtype, t.dtype))
        if tuple(t.shape) != tuple(shape):
            raise ValueError("%s must have shape %s, not %s" % (name, tuple(shape), tuple(t.shape)))
        if not t.is_contiguous():
            raise ValueError("%s must be contiguous" % name)


def plan_order(row_of_cell, rows=None):
    """int32 array ``order``: the cells grouped by their row of the mean tensor (stable): the order of presentation that
    keeps a gene tile's rows of the mean tensor in cache (prosstt_amd_plan_order; host arrays, no device work).  Present
    cell ``order[i]`` at position i with ``cell_index[i]`` = its global id; row i of the result is that cell's."""
    roc = np.ascontiguousarray(row_of_cell, dtype=np.int32)
    order = np.empty(roc.size, dtype=np.int32)
    if roc.size:
        n_rows = int(roc.max()) + 1 if rows is None else int(rows)
        _native.check(_native.load().prosstt_amd_plan_order(
            roc.ctypes.data_as(ctypes.c_void_p), roc.size, n_rows, order.ctypes.data_as(ctypes.c_void_p)))
    return order


def run_plan(row_of_cell, rows, strip_cells):
    """uint32 array of N + 4 words: where cells presented in this order share rows of the mean tensor, as the sampler's
    preparation kernel records it for waves that take ``strip_cells`` cells each (prosstt_amd_run_plan; host arrays, no
    device work).  Low 16 bits: the length of the run that starts at the cell (0: none starts there); high 16 bits, at a
    strip's first cell: the runs of the strip."""
    roc = np.ascontiguousarray(row_of_cell, dtype=np.int32)
    words = np.empty(roc.size + 4, dtype=np.uint32)
    _native.check(_native.load().prosstt_amd_run_plan(
        roc.ctypes.data_as(ctypes.c_void_p), roc.size, int(rows), int(strip_cells), words.ctypes.data_as(ctypes.c_void_p)))
    return words


def strip_plan(n_cells, G, resident_blocks, strip_cells=0, taper=0):
    """(classes, tiles_g, blocks): which cells the waves of the sampler's stream kernel take in a call of ``n_cells`` x
    ``G`` on a device that holds ``resident_blocks`` of its blocks at once (prosstt_amd_strip_plan; no device work).
    ``classes`` is an int32 array of up to 4 rows {first cell, strip length, first block}."""
    classes = np.zeros((4, 3), np.int32)
    n, tiles, blocks = ctypes.c_int32(0), ctypes.c_int32(0), ctypes.c_int32(0)
    _native.check(_native.load().prosstt_amd_strip_plan(
        int(n_cells), int(G), int(resident_blocks), int(strip_cells), int(taper), classes.ctypes.data_as(ctypes.c_void_p),
        ctypes.byref(n), ctypes.byref(tiles), ctypes.byref(blocks)))
    return classes[:n.value].copy(), tiles.value, blocks.value


def inverse_permutation(perm):
    """int64 array ``inv`` with ``inv[perm[i]] = i``: the row of every cell, from the cell of every row."""
    perm = np.asarray(perm, dtype=np.int64)
    inv = np.empty(perm.size, dtype=np.int64)
    inv[perm] = np.arange(perm.size, dtype=np.int64)
    return inv


def host_fingerprint(arrays):
    """Identity and content fingerprint of host arrays that a device tensor mirrors: the caches of
    ``Tree.device_means`` and of ``simulate_lineage`` compare it before they trust their device copy,
    so that the caller's arrays stay writable (as the reference's are) and an in-place edit is seen.
    One pass at memory speed (64 MB in ~6 ms)."""
    try:
        from xxhash import xxh3_64_intdigest as digest
    except ImportError:                              # slower (64 MB in ~60 ms), as position-sensitive
        import zlib

        def digest(buf):
            view = memoryview(buf).cast("B")
            return (zlib.crc32(view) << 32) | zlib.adler32(view)
    out = []
    for a in arrays:
        if isinstance(a, np.ndarray):
            c = a if a.flags.c_contiguous else np.ascontiguousarray(a)
            out.append((id(a), a.shape, a.dtype.str, digest(c.data if c.size else b"")))
        else:
            out.append((id(a), None, None, None))
    return tuple(out)


PINNED_RETURN_MAX = int(os.environ.get("PROSSTT_AMD_PINNED_MAX_BYTES", str(32 << 30)))


HOST_DTYPES = {"numpy": np.int64, "numpy32": np.int32, "numpy16": np.uint16}


# How an int64 / int32 host return of 2^24 counts or more travels.  WIDEN_ON = "host" (default): the matrix crosses PCIe in
# a wire format narrower than its type -- first "u8", the low 8 bits of every count, and beside them the entries that
# have higher bits set (two thirds of a count matrix are zeros; one count in a thousand of C3 is above 255, the largest is
# 84 036); "u16", then "i32", for a matrix with too many of those -- and the host library's threads (libprosstt_amd_host.so)
# widen chunk i - 1 into the result while chunk i is on the bus; "device": as rounds 2 to 5 did -- int64 formed on the
# device, 8 bytes per count over PCIe, int32 copied as it lies (the choice for a host with very few cores).
# (tools/host_widen_probe.py, tools/e2e_threads.py on an MI355X box's host: the pool writes 250 - 340 GB/s from eight threads
# on; PCIe carries 52 GB/s.  C3 end to end: int64 147 -> 39 - 51 ms, int32 76 -> 32 - 39 ms, out="csr" 58 -> 38 ms.)
WIDEN_ON = os.environ.get("PROSSTT_AMD_WIDEN", "host")
HOST_THREADS = int(os.environ.get("PROSSTT_AMD_HOST_THREADS", str(max(1, min(16, os.cpu_count() or 1)))))


def to_host(counts, dtype=np.int64, chunk_bytes=256 << 20, row_order=None):
    """int32 device counts -> host ndarray of ``dtype``: int64 (the reference's return type,
    simulation.py:651), int32 (what the device holds) or uint16 (raises OverflowError if a count does not fit: C3's
    largest is 84 036).

    int64 and int32 of 2^24 counts or more cross PCIe a chunk of rows at a time in a wire format narrower than the result
    (``WIDEN_ON``) and are widened by the host library's threads into pageable memory on huge pages that is recycled once
    the caller has dropped the result (``_result_array``).  Everything else -- uint16, smaller matrices, ``WIDEN_ON`` =
    "device", no host library, bounce buffers that cannot be page-locked -- lands by DMA in the result's own type, in
    page-locked memory from torch's caching host allocator (at most PROSSTT_AMD_PINNED_MAX_BYTES, default 32 GiB; beyond
    that, or when page-locking fails, in ordinary memory); int64 is formed and uint16 narrowed on the device.

    row_order: the device matrix holds its cells in an order of PRESENTATION (``plan_order``): row i is cell
    ``row_order[i]``.  The host array comes back in plan order -- row ``row_order[i]`` = device row i -- the rows of every
    chunk gathered on the device under the transfer of the previous chunk: nothing is added to the PCIe-bound copy."""
    torch = _torch()
    dtype = np.dtype(dtype)
    n, g = (int(v) for v in counts.shape)
    if dtype not in (np.dtype(np.int64), np.dtype(np.int32), np.dtype(np.uint16)):
        raise ValueError("host counts are int64, int32 or uint16")
    if n == 0 or g == 0:
        return np.zeros((n, g), dtype=dtype)
    if dtype.itemsize == 2 and int(counts.max()) > 65535:
        raise OverflowError("a count of %d does not fit uint16: ask for 'numpy32'" % int(counts.max()))
    inv = _device_rows(row_order, n, counts.device)
    own = {8: "i64", 4: "i32", 2: "u16"}[dtype.itemsize]
    if dtype.itemsize >= 4 and WIDEN_ON == "host" and n * g >= (1 << 24):
        host = torch.from_numpy(_result_array((n, g), dtype))
        for wire in (w for w in ("u8", "u16", "i32") if w != own):
            try:
                _dense_attempt(counts, host, inv, chunk_bytes, wire)
                return host.numpy()
            except _WireTooNarrow:
                continue
            except _NoHostWidening:
                break
    # (torch has no arithmetic on uint16: the device narrows to int16 bit patterns, viewed as uint16 on the host)
    host = _dma_result((n, g), {8: torch.int64, 4: torch.int32, 2: torch.int16}[dtype.itemsize])
    _dense_attempt(counts, host, inv, chunk_bytes, own)
    return host.numpy().view(dtype)


def _dense_attempt(counts, host, inv, chunk_bytes, wire):
    """One try of ``to_host``: the device matrix over ``wire`` into the (n, g) host tensor ``host``, rows in host order
    through ``inv``.  A wire narrower than ``host`` lands in page-locked bounce buffers, chunks of ``chunk_bytes`` of int32,
    and the host library's threads widen it; the entries that "u8" / "u16" cannot carry travel beside it, at most one in
    256 of a chunk (else _WireTooNarrow).  A wire as wide as ``host`` lands in it by DMA, chunks of ``chunk_bytes`` of it."""
    torch = _torch()
    n, g = (int(v) for v in counts.shape)
    dev = counts.device
    t_wire = getattr(torch, {"u8": "uint8", "u16": "int16", "i32": "int32", "i64": "int64"}[wire])
    on_host = t_wire.itemsize < host.element_size()
    rows = max(1, min(n, int(chunk_bytes) // (g * (4 if on_host else t_wire.itemsize))))
    chunks = [(lo, min(lo + rows, n)) for lo in range(0, n, rows)]
    slots = min(2, len(chunks))
    if on_host:
        widen = getattr(_host_lib(), "prosstt_amd_host_widen_%s_i%d" % (wire, 8 * host.element_size()))
        bounce = [_bounce((rows, g), t_wire) for _ in range(slots)]
    over = _Overflow(dev, slots, rows * g, 256, -256 if wire == "u8" else -65536) if on_host and wire != "i32" else None
    # device staging: the chunk's rows gathered (int32; for the int32 wire straight into the slot) and converted to the wire
    convert = wire != "i32"
    staged = [torch.empty((rows, g), dtype=t_wire, device=dev) for _ in range(slots)] if (inv is not None or convert) else None
    gathered = torch.empty((rows, g), dtype=torch.int32, device=dev) if (inv is not None and convert) else None

    def stage(chunk, slot):
        lo, hi = chunk
        block = counts[lo:hi] if inv is None else torch.index_select(
            counts, 0, inv[lo:hi], out=(gathered if convert else staged[slot])[:hi - lo])
        if convert:
            staged[slot][:hi - lo].copy_(block)              # int32 -> int64, or the low 16 / 8 bits
        copies = [(bounce[slot][:hi - lo] if on_host else host[lo:hi], staged[slot][:hi - lo] if convert else block)]
        return copies if over is None else copies + over.note(block.reshape(-1), lo * g, slot)

    def land(chunk, slot):
        lo, hi = chunk
        if over is not None:
            over.take(slot, (hi - lo) * g)
        _widen(widen, bounce[slot], host, lo * g, (hi - lo) * g)

    _copy_chunks(dev, chunks, slots, stage, land if on_host else None)
    if over is not None:
        over.scatter(host)


def to_host_csr(counts, chunk_bytes=256 << 20, row_order=None):
    """int32 device counts -> ``scipy.sparse.csr_matrix`` (int32 data, int32 column indices sorted within a row, int64
    row pointers) in plan order: what the single-cell toolchains downstream of the reference's count files hold a count
    matrix in.  Two thirds of such a matrix are zeros, and only the NON-ZEROS cross PCIe -- 3 bytes each (the value's low 8
    bits, a 16-bit column index; more for a matrix of large counts or of more than 65 536 columns), widened by the host
    library's threads -- and the dense matrix never exists on the host.

    Two passes over the device matrix, a chunk of rows at a time: the non-zeros per row first (the row pointers, and with
    them the exact size of the result), then every chunk's non-zeros are compacted on the device (row-major) and copied
    toward their final place while the next chunk is compacted (``_csr_attempt``).  ``row_order``: as in ``to_host``
    (device row i is cell ``row_order[i]``; the gather of whole rows rides in the first step of each chunk)."""
    torch = _torch()
    import scipy.sparse as sparse
    n, g = (int(v) for v in counts.shape)
    if n == 0 or g == 0:
        return sparse.csr_matrix((n, g), dtype=np.int32)
    if g >= 2 ** 31:
        raise ValueError("column indices are int32")
    dev = counts.device
    rows = max(1, min(n, int(chunk_bytes) // (g * 4)))
    bounds = [(lo, min(lo + rows, n)) for lo in range(0, n, rows)]
    inv = _device_rows(row_order, n, dev)
    # pass 1: non-zeros of every row, in the order of the rows on the host
    per_row = torch.empty(n, dtype=torch.int64, device=dev)
    for lo, hi in bounds:
        per_row[lo:hi] = torch.count_nonzero(counts[lo:hi], dim=1)
    if inv is not None:
        per_row = per_row.index_select(0, inv)
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(per_row.cpu().numpy(), out=indptr[1:])
    total = int(indptr[-1])
    # pass 2, over the chunks that hold non-zeros: (rows lo:hi, their non-zeros first:last)
    chunks = [(lo, hi, int(indptr[lo]), int(indptr[hi])) for lo, hi in bounds if indptr[hi] > indptr[lo]]
    made = {}

    def attempt(vals, cols):
        for name, wire in (("data", vals), ("indices", cols)):      # each result array once per call and kind of memory
            if (name, wire) not in made:
                made[name, wire] = (_dma_result((total,), torch.int32) if wire == "i32"
                                    else torch.from_numpy(_result_array((total,), np.int32)))
        data, indices = made["data", vals], made["indices", cols]
        _csr_attempt(counts, inv, rows, chunks, data, indices, vals, cols)
        out = sparse.csr_matrix((data.numpy(), indices.numpy(), indptr), shape=(n, g), copy=False)
        out.has_sorted_indices = True
        return out

    if WIDEN_ON == "host" and total >= (1 << 22):
        cols = "u16" if g <= 65536 else "i32"
        for vals in ("u8", "i32"):
            try:
                return attempt(vals, cols)
            except _WireTooNarrow:
                continue
            except _NoHostWidening:
                break
    return attempt("i32", "i32")


def _csr_attempt(counts, inv, rows, chunks, data, indices, vals_wire, cols_wire):
    """Pass 2 of ``to_host_csr`` over one wire configuration: the non-zeros of every chunk (lo, hi, first, last) compacted
    on the device, values over ``vals_wire`` into ``data[first:last]``, column indices over ``cols_wire`` into
    ``indices[first:last]``.  "u8" values (those above 255 beside them, at most one in 16 of a chunk's, else
    _WireTooNarrow) and "u16" columns land in page-locked bounce buffers for the host library's threads; "i32" by DMA."""
    torch = _torch()
    g = int(counts.shape[1])
    dev = counts.device
    cap = max((last - first for _, _, first, last in chunks), default=0)
    slots = min(2, len(chunks))
    lib = _host_lib() if (vals_wire, cols_wire) != ("i32", "i32") else None
    bounce_v = [_bounce(cap, torch.uint8) for _ in range(slots)] if vals_wire == "u8" else None
    bounce_c = [_bounce(cap, torch.int16) for _ in range(slots)] if cols_wire == "u16" else None
    over = _Overflow(dev, slots, cap, 16, -256) if vals_wire == "u8" else None
    vals = [torch.empty(cap, dtype=torch.uint8 if vals_wire == "u8" else torch.int32, device=dev) for _ in range(slots)]
    cols = [torch.empty(cap, dtype=torch.int16 if cols_wire == "u16" else torch.int32, device=dev) for _ in range(slots)]
    vals32 = torch.empty(cap, dtype=torch.int32, device=dev) if over is not None else None
    gathered = torch.empty((rows, g), dtype=torch.int32, device=dev) if inv is not None else None

    def stage(chunk, slot):
        lo, hi, first, last = chunk
        k = last - first
        block = counts[lo:hi] if inv is None else torch.index_select(counts, 0, inv[lo:hi], out=gathered[:hi - lo])
        flat = block.reshape(-1)
        where = torch.nonzero_static(flat, size=k, fill_value=0).squeeze(1)     # ascending flat positions = CSR order
        if over is None:
            torch.index_select(flat, 0, where, out=vals[slot][:k])
        else:
            torch.index_select(flat, 0, where, out=vals32[:k])
            vals[slot][:k].copy_(vals32[:k])                    # the low 8 bits
        cols[slot][:k].copy_(torch.remainder(where, g))
        copies = [(data[first:last] if bounce_v is None else bounce_v[slot][:k], vals[slot][:k]),
                  (indices[first:last] if bounce_c is None else bounce_c[slot][:k], cols[slot][:k])]
        return copies if over is None else copies + over.note(vals32[:k], first, slot)

    def land(chunk, slot):
        first, last = chunk[2:]
        if bounce_v is not None:
            over.take(slot, last - first)
            _widen(lib.prosstt_amd_host_widen_u8_i32, bounce_v[slot], data, first, last - first)
        if bounce_c is not None:
            _widen(lib.prosstt_amd_host_widen_u16_i32, bounce_c[slot], indices, first, last - first)

    _copy_chunks(dev, chunks, slots, stage, land if lib is not None else None)
    if over is not None:
        over.scatter(data)


def _copy_chunks(dev, chunks, slots, stage, land=None):
    """The double-buffered copy of a device matrix to the host, a chunk at a time, on a second stream; chunk i uses the
    buffers of slot i % ``slots``.  ``stage(chunk, slot)`` enqueues on the current stream what the chunk sends and returns
    its copies, (host destination, device source) pairs; ``land(chunk, slot)`` finishes the chunk on the host once they
    have arrived.  The current stream stages into a slot only once the slot's previous chunk has left; the copier starts
    on a chunk once it is staged; chunk i - 1 lands while chunk i is on the bus, so a slot's previous chunk has landed
    before its bounce buffers are written again.  Nothing is in flight when this returns or raises."""
    torch = _torch()
    compute = torch.cuda.current_stream(dev)
    copier = torch.cuda.Stream(dev)
    arrived = [None] * slots
    try:
        for i, chunk in enumerate(chunks):
            slot = i % slots
            if arrived[slot] is not None:
                compute.wait_event(arrived[slot])           # the slot's previous chunk has left
            copies = stage(chunk, slot)
            copier.wait_stream(compute)
            with torch.cuda.stream(copier):
                for dst, src in copies:
                    dst.copy_(src, non_blocking=True)
                arrived[slot] = copier.record_event()
            if land is not None and i >= 1:
                arrived[(i - 1) % slots].synchronize()
                land(chunks[i - 1], (i - 1) % slots)
        copier.synchronize()
        if land is not None and chunks:
            land(chunks[-1], (len(chunks) - 1) % slots)
    except BaseException:
        copier.synchronize()                                # (nothing of this attempt is in flight when its buffers go back)
        compute.synchronize()
        raise


class _Overflow:
    """The side channel of a narrow wire: the entries of a chunk with a bit of ``mask`` set (higher bits than the wire
    carries, or a negative count) travel beside it as (position in the result, value) pairs, in fixed-size buffers of
    each slot with room for one entry in ``per`` of ``capacity``, so that nothing on the way waits for the device; more
    than one in ``per`` of a chunk, counted when it has landed, is _WireTooNarrow.  The pairs are written at the end."""

    def __init__(self, dev, slots, capacity, per, mask):
        torch = _torch()
        self.room, self.per, self.mask = max(1, capacity // per), per, mask
        # per slot: (positions, values, their number) on the device, and page-locked on the host
        self.dev = [tuple(torch.empty(shape, dtype=t, device=dev) for shape, t in
                          ((self.room, torch.int64), (self.room, torch.int32), ((), torch.int64))) for _ in range(slots)]
        self.host = [tuple(_bounce(t.shape, t.dtype) for t in bufs) for bufs in self.dev]
        self.pairs = []

    def note(self, values, offset, slot):
        """Stage the entries of the flat int32 device tensor ``values`` beyond the wire, at ``offset`` + their index."""
        torch = _torch()
        where, value, count = self.dev[slot]
        high = torch.bitwise_and(values, self.mask)
        count.copy_(torch.count_nonzero(high))
        at = torch.nonzero_static(high, size=self.room, fill_value=0).squeeze(1)     # (padded with index 0: never read)
        torch.index_select(values, 0, at, out=value)
        torch.add(at, offset, out=where)
        return list(zip(self.host[slot], self.dev[slot]))

    def take(self, slot, size):
        """Keep the pairs of the chunk of ``size`` entries that has landed in ``slot``."""
        where, value, count = self.host[slot]
        k = int(count)
        if k > self.room or k * self.per > size:
            raise _WireTooNarrow()
        if k:
            self.pairs.append((where[:k].clone(), value[:k].clone()))

    def scatter(self, result):
        """Write the pairs over the widened int32 / int64 host tensor ``result``."""
        if self.pairs:
            torch = _torch()
            where, values = (torch.cat([pair[i] for pair in self.pairs]) for i in (0, 1))
            if _native.load("host").prosstt_amd_host_scatter_i32(result.data_ptr(), result.element_size(), where.data_ptr(),
                                                                 values.data_ptr(), where.numel(), HOST_THREADS) != 0:
                raise RuntimeError("the host library refused its arguments")


class _WireTooNarrow(Exception):
    """Too many entries of a chunk do not fit the wire: the copy starts again with the next wider one."""


class _NoHostWidening(Exception):
    """No host library or no page-locked bounce buffers: the copy falls through to the one in the result's own type."""


_warned_no_host_lib = False


def _host_lib():
    """libprosstt_amd_host.so, or _NoHostWidening (and, the first time in the process, a RuntimeWarning)."""
    global _warned_no_host_lib
    try:
        return _native.load("host")
    except RuntimeError as exc:
        if not _warned_no_host_lib:
            _warned_no_host_lib = True
            warnings.warn("%s: host returns are not widened on the host" % exc, RuntimeWarning)
        raise _NoHostWidening() from exc


def _bounce(shape, t_dtype):
    """A page-locked host buffer that a narrow wire lands in, or _NoHostWidening."""
    try:
        return _torch().empty(shape, dtype=t_dtype, pin_memory=True)
    except RuntimeError as exc:
        raise _NoHostWidening() from exc


def _widen(fn, src, dst, first, count):
    """The host library's widening ``fn`` of ``count`` entries of ``src`` into the host tensor ``dst`` from entry ``first``."""
    if fn(src.data_ptr(), dst.data_ptr() + first * dst.element_size(), count, HOST_THREADS) != 0:
        raise RuntimeError("the host library refused its arguments")


def _dma_result(shape, t_dtype):
    """A host tensor that DMA lands a result in: page-locked up to PINNED_RETURN_MAX bytes, else ordinary memory."""
    torch = _torch()
    if 0 < int(np.prod(shape)) * t_dtype.itemsize <= PINNED_RETURN_MAX:
        try:
            return torch.empty(shape, dtype=t_dtype, pin_memory=True)
        except RuntimeError:
            pass
    return torch.empty(shape, dtype=t_dtype)


def _device_rows(row_order, n, dev):
    """The device row of every host row (the inverse of ``row_order``) as an int64 device tensor; None without an order."""
    if row_order is None:
        return None
    order = np.asarray(row_order, dtype=np.int64)
    if order.shape != (n,):
        raise ValueError("row_order must have one entry per row")
    return _torch().as_tensor(inverse_permutation(order)).to(dev)


_free_blocks = []              # pageable result memory that no result holds, oldest first; see _result_array
_result_lock = threading.Lock()
RESULT_CACHE_BYTES = int(os.environ.get("PROSSTT_AMD_RESULT_CACHE_BYTES", str(40 << 30)))


class _Lease:
    """A result's hold on its block: the result is ``np.asarray(lease)``, so every numpy view and torch tensor of it keeps
    the lease alive, and the block goes back to the free blocks when the last of them goes."""
    __slots__ = ("__array_interface__", "__weakref__")

    def __init__(self, block, shape, dtype):
        self.__array_interface__ = dict(shape=tuple(shape), typestr=np.dtype(dtype).str, data=(block.ctypes.data, False),
                                        version=3)


def _result_array(shape, dtype):
    """A pageable result that the host library's threads write, on a numpy allocation (numpy asks for transparent huge
    pages: the first touch of 8 GB costs 45 ms instead of the 500 ms of 4 KB pages) lent to it: once the result and every
    view of it -- numpy or torch -- are gone, the next result of that size or a little less is laid over the same, already
    touched pages, without the 0.6 - 0.9 s of page-locking that torch's caching host allocator puts before 8 GB."""
    nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
    with _result_lock:
        fits = [i for i, free in enumerate(_free_blocks) if nbytes <= free.size <= 2 * nbytes + (1 << 20)]
        block = _free_blocks.pop(fits[0]) if fits else np.empty(nbytes, dtype=np.uint8)
        held = sum(free.size for free in _free_blocks)
        while _free_blocks and held > RESULT_CACHE_BYTES:
            held -= _free_blocks.pop(0).size             # the oldest first
    lease = _Lease(block, shape, dtype)
    # (a plain append, no lock: the finalizer may run in any thread, in a collection while _result_lock is held)
    weakref.finalize(lease, _free_blocks.append, block)
    return np.asarray(lease)


def release_result_memory():
    """Free the recycled result blocks that no result holds (PROSSTT_AMD_RESULT_CACHE_BYTES bounds them: 40 GiB); a block
    that a result still holds joins them when its last user drops it."""
    with _result_lock:
        del _free_blocks[:]


HOST_OUTS = tuple(HOST_DTYPES) + ("csr",)
OUT_CHOICES = "out must be 'numpy', 'numpy32', 'numpy16', 'csr' or 'torch'"


def host_return(counts, out, row_order=None):
    """The host form ``out`` names (``HOST_OUTS``) of a device count matrix, rows in plan order."""
    if out == "csr":
        return to_host_csr(counts, row_order=row_order)
    return to_host(counts, HOST_DTYPES[out], row_order=row_order)


class Comm:
    """The one exchange of the path on RCCL directly, through the C ABI (prosstt_amd_comm_* / prosstt_amd_gather_counts:
    what a host binding without torch.distributed uses; prosstt_amd.parallel is the torch.distributed form).

        uid = Comm.unique_id()                 # on rank 0; carry the 128 bytes to the other ranks yourself
        comm = Comm(ctx, uid, rank, world)     # collective
        full = comm.gather_counts(counts, rows_of_rank, root=0)      # (sum(rows_of_rank), G) on the root, None elsewhere:
                                                                     # rank 0's rows, then rank 1's, ... (shard order)
    """

    @staticmethod
    def unique_id():
        buf = ctypes.create_string_buffer(128)
        _native.check(_native.load().prosstt_amd_comm_unique_id(buf))
        return buf.raw

    def __init__(self, ctx, unique_id, rank, world):
        if len(unique_id) != 128:
            raise ValueError("the unique id is 128 bytes")
        self.ctx, self.rank, self.world = ctx, int(rank), int(world)
        self._lib = _native.load()
        self._h = ctypes.c_void_p()
        _native.check(self._lib.prosstt_amd_comm_init(ctx._h, ctypes.c_char_p(unique_id), self.rank, self.world,
                                                      ctypes.byref(self._h)))

    def gather_counts(self, counts, rows_of_rank, root=0):
        torch = _torch()
        rows_of_rank = np.ascontiguousarray(rows_of_rank, dtype=np.int64)
        if rows_of_rank.shape != (self.world,) or int(rows_of_rank[self.rank]) != counts.shape[0]:
            raise ValueError("rows_of_rank must hold every rank's row count, this rank's equal to its rows")
        counts = counts.contiguous()
        G = int(counts.shape[1])
        dst = torch.empty((int(rows_of_rank.sum()), G), dtype=torch.int32, device=counts.device) if self.rank == root else None
        _native.check(self._lib.prosstt_amd_gather_counts(
            self.ctx._h, self._h, ctypes.c_void_p(counts.data_ptr()), rows_of_rank.ctypes.data_as(ctypes.c_void_p), G, int(root),
            ctypes.c_void_p(dst.data_ptr()) if dst is not None else None))
        return dst

    def selftest(self, nbytes=1 << 20):
        _native.check(self._lib.prosstt_amd_comm_selftest(self.ctx._h, self._h, ctypes.c_uint64(int(nbytes))))

    def close(self):
        if self._h:
            self._lib.prosstt_amd_comm_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PresentedCounts:
    """The count matrix as it lies on the device after a call that PRESENTED its cells grouped by their row of the mean
    tensor (what keeps a gene tile's rows of the tensor in cache: 2 to 5 % of the kernel, and 1.75 x less HBM traffic on a
    32-branch tree): ``counts`` is the (N, G) int32 device tensor, row i of it belongs to cell ``cell_of_row[i]`` of the
    plan (the order of the pseudotime / branch / scaling arrays the call returns).  Every count is keyed by the cell's
    position in the plan, so ``counts`` holds exactly the rows of the plan-ordered matrix, permuted.

        counts, cell_of_row = presented                  # unpacks like a pair
        presented.in_plan_order()                        # a new device tensor, rows in plan order (one gather pass)
        presented.to_host("numpy32")                     # host ndarray in plan order (the gather rides in the copy)
        presented.row_of_cell                            # the inverse permutation
    """

    def __init__(self, counts, cell_of_row):
        self.counts = counts
        self.cell_of_row = np.asarray(cell_of_row, dtype=np.int64)
        self._row_of_cell = None

    def __iter__(self):
        return iter((self.counts, self.cell_of_row))

    def __len__(self):
        return 2

    @property
    def shape(self):
        return tuple(self.counts.shape)

    @property
    def row_of_cell(self):
        if self._row_of_cell is None:
            self._row_of_cell = inverse_permutation(self.cell_of_row)
        return self._row_of_cell

    def in_plan_order(self):
        torch = _torch()
        return self.counts.index_select(0, torch.as_tensor(self.row_of_cell).to(self.counts.device))

    def to_host(self, out="numpy"):
        return host_return(self.counts, out, row_order=self.cell_of_row)


NEGATIVE_ENTRY = "the count matrix has a negative entry"      # the ValueError of every reader of a count matrix


def to_plan_order(cell_of_row, *per_row):
    """Host arrays with one entry per row of a presented matrix, scattered to plan order (row i is cell
    ``cell_of_row[i]``); the arrays themselves when ``cell_of_row`` is None."""
    if cell_of_row is None:
        return per_row
    out = tuple(np.empty_like(a) for a in per_row)
    for o, a in zip(out, per_row):
        o[cell_of_row] = a
    return out


class CountMatrix:
    """A count input as the libraries that read the int32 matrix where it lies take it, checked in two steps.

    ``CountMatrix(counts, who)`` accepts an int32 (cells, genes) torch tensor or a ``PresentedCounts`` and exposes ``X``,
    ``N``, ``G`` and ``cell_of_row`` (None for a plain tensor); TypeError for anything but an int32 tensor, ValueError
    for other than two dimensions.  ``who`` names the caller in the messages.  ``on_device()`` then requires a device
    tensor with unit column stride and rows that do not overlap, sets ``ld`` (the row stride in elements) and ``device``
    and returns the view.  Limits on N and G are the caller's, between the steps or after them."""

    def __init__(self, counts, who):
        torch = _torch()
        self.who, self.cell_of_row = who, None
        if isinstance(counts, PresentedCounts):
            counts, self.cell_of_row = counts.counts, counts.cell_of_row
        if not isinstance(counts, torch.Tensor):
            raise TypeError("%s takes an int32 device tensor or a device.PresentedCounts, not %s (host arrays are refused: "
                            "there is no CPU path)" % (who, type(counts).__name__))
        if counts.dtype != torch.int32:
            raise TypeError("%s needs int32 counts, not %s" % (who, counts.dtype))
        if counts.dim() != 2:
            raise ValueError("%s needs a (cells, genes) matrix, not %d dimensions" % (who, counts.dim()))
        self.X = counts
        self.N, self.G = counts.shape

    def on_device(self):
        X, N, G = self.X, self.N, self.G
        if X.device.type != "cuda":
            raise ValueError("%s needs a device tensor, not one on %s" % (self.who, X.device))
        if G > 1 and X.stride(1) != 1:
            raise ValueError("%s needs unit column stride (got %d)" % (self.who, X.stride(1)))
        self.ld = X.stride(0) if N > 1 else G
        if self.ld < G:
            raise ValueError("rows overlap (row stride %d < %d genes)" % (self.ld, G))
        self.device = X.device
        return self

    def stream(self):
        """torch's current stream on the matrix's device, as the C ABI takes it."""
        return current_stream(self.device)

    def workspace(self, name, query_symbol, *sizes):
        """A uint8 device tensor of the bytes that library ``name``'s ``*_workspace_bytes`` (``query_symbol``) asks for
        this matrix and ``sizes``."""
        return workspace(name, query_symbol, self.device, self.N, self.G, *sizes)


_contexts = {}


def get_context(device=None):
    """Process-wide Context of a device, bound to torch's current stream at first use."""
    torch = _torch()
    require_gpu()
    dev = torch.cuda.current_device() if device is None else int(device)
    key = (dev, torch.cuda.current_stream(dev).cuda_stream)
    if key not in _contexts:
        _contexts[key] = Context(dev)
    return _contexts[key]
