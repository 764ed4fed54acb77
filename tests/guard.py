"""Control over what lies AROUND an allocation, as tests/stale.py controls what lies inside one.  ``guarded(byte)`` replaces,
for the duration of a block, every allocator the wrappers under prosstt_amd/ use (``torch.empty``, ``empty_like``,
``empty_strided``, ``zeros``, ``zeros_like``, ``ones``, ``ones_like``, ``full``, ``full_like`` and ``Tensor.new_empty``,
``new_zeros``, ``new_ones``, ``new_full``).  A device tensor is then carved out of one uint8 buffer of the helper's own:

    | BAND bytes of ``byte`` | the tensor's bytes: 0x00, then the call's own fill | BAND bytes of ``byte`` |

with the shape, dtype and strides of the original call and the original's address modulo 256 (so ``aligned()`` picks the
same kernel), the back band starting at the tensor's last byte.  ``state.check()`` then tells whether every band still holds
``byte``: a store one element, one row or one tile past either end of an output, a slab or a workspace, which otherwise lands
in the allocator's rounding or in a neighbouring tensor and changes no result, is named with its allocation site.
``place(tensor, byte)`` does the same for an input made before the call, the padding columns between the rows of a view
included, and its ``check_untouched()`` tells whether any byte of the buffer changed at all.  Since the interior is 0x00
under every byte, a result that differs between bytes can only come from a READ outside a buffer.

BAND is a condition, not a measurement: a multiple of 256, and 8 rows (less 96 bytes) of the widest matrix in the suite (2051
int32 genes, 8204 bytes a row).

Out of reach: memory that native code allocates itself, tensors allocated before the block was entered, allocations inside
torch's own operators (``clone``, ``cat``, arithmetic, ``from_numpy(...).cuda()``), tensors without bytes (handed through),
reads outside a buffer that change no result, and overruns of more than BAND bytes.  Nothing here faults: the bands are
memory the helper owns.  A helper: nothing here is collected."""
import contextlib
import os
import sys

import numpy as np
import torch

BAND = 65536
_PACKAGE = os.sep + "prosstt_amd" + os.sep
_HERE = os.path.abspath(__file__)


def _span(t):
    """Bytes from the first to the last byte of ``t``'s elements (0 without elements; strides are not negative in torch)."""
    if t.numel() == 0:
        return 0
    return (1 + sum((n - 1) * s for n, s in zip(t.shape, t.stride()))) * t.element_size()


def _carve(like, byte, full, empty_strided):
    """(buffer, start, tensor): a uint8 buffer of ``byte`` with at least BAND bytes before ``start`` and BAND after
    ``start + span``, and a tensor of ``like``'s shape, dtype and strides at ``start``, whose address is ``like``'s modulo
    256.  ``full`` and ``empty_strided`` are torch's own."""
    span = _span(like)
    buffer = full((BAND + 256 + span + BAND,), byte, dtype=torch.uint8, device=like.device)
    start = BAND + (like.data_ptr() - buffer.data_ptr() - BAND) % 256
    assert start % like.element_size() == 0 and buffer.data_ptr() % like.element_size() == 0
    tensor = empty_strided((0,), (1,), dtype=like.dtype, device=like.device).set_(
        buffer.untyped_storage(), start // like.element_size(), like.shape, like.stride())
    assert tensor.data_ptr() == buffer.data_ptr() + start and tensor.data_ptr() % 256 == like.data_ptr() % 256
    return buffer, start, tensor


def _original(function):
    """torch's own allocator behind ``function``, also inside a ``guarded`` or ``stale.poisoned`` block."""
    while hasattr(function, "__wrapped__"):
        function = function.__wrapped__
    return function


def _site():
    """file:line of the nearest calling frame under prosstt_amd/, else of the nearest frame outside this file."""
    frame, nearest = sys._getframe(1), None
    while frame is not None:
        name = os.path.abspath(frame.f_code.co_filename)
        if name != _HERE:
            where = "%s:%d" % (name, frame.f_lineno)
            nearest = nearest or where
            if _PACKAGE in name:
                return "prosstt_amd/" + where.split(_PACKAGE)[-1]
        frame = frame.f_back
    return nearest


class Record:
    """One guarded tensor: its buffer (kept alive), where the tensor starts and ends in it, and what to call it."""

    def __init__(self, buffer, start, span, tensor, site, mod):
        self.buffer, self.start, self.end = buffer, start, start + span
        self.shape, self.dtype, self.site, self.mod = tuple(tensor.shape), tensor.dtype, site, mod

    def name(self):
        return "%s of %s allocated at %s" % (self.shape, self.dtype, self.site)


def _damage(record, which, band, byte):
    """None, or the message for a band (a host uint8 array) that no longer holds ``byte``."""
    bad = np.flatnonzero(band != byte)
    if not bad.size:
        return None
    first = int(bad[0]) if which == "back" else int(bad[0]) - band.size
    return "%s band of %s: %d bytes damaged, first at %+d from the tensor's %s" % (
        which, record.name(), bad.size, first, "end" if which == "back" else "start")


class Guard:
    """What ``guarded`` yields: ``byte``, ``records`` (one per guarded tensor, holding its buffer until ``release``) and
    ``allocations``, their count."""

    def __init__(self, byte, devices):
        self.byte, self.devices, self.records = int(byte), tuple(devices), []

    @property
    def allocations(self):
        return len(self.records)

    def check(self):
        """Every band against ``byte`` after a synchronize, with one transfer for all of them.  AssertionError names site,
        shape, dtype, the band, the number of damaged bytes and the offset of the first from the tensor's end or start."""
        if not self.records:
            return
        if torch.cuda.is_available() and any(r.buffer.is_cuda for r in self.records):
            torch.cuda.synchronize()
        found = []
        for device in {r.buffer.device for r in self.records}:
            mine = [r for r in self.records if r.buffer.device == device]
            bands = [b for r in mine for b in (r.buffer[:r.start], r.buffer[r.end:])]
            host = torch.cat(bands).cpu().numpy()
            at = 0
            for r in mine:
                for which, size in (("front", r.start), ("back", r.buffer.numel() - r.end)):
                    found.append(_damage(r, which, host[at:at + size], self.byte))
                    at += size
        found = [f for f in found if f]
        if found:
            raise AssertionError("a write outside a tensor: " + "; ".join(found[:8])
                                 + ("; and %d more" % (len(found) - 8) if len(found) > 8 else ""))

    def release(self):
        """Drops the buffers (results that are views of them keep theirs)."""
        self.records = []


_FILLERS = (("empty", False), ("empty_like", False), ("empty_strided", False), ("zeros", True), ("zeros_like", True),
            ("ones", True), ("ones_like", True), ("full", True), ("full_like", True))
_METHODS = (("new_empty", False), ("new_zeros", True), ("new_ones", True), ("new_full", True))


@contextlib.contextmanager
def guarded(byte, devices=("cuda",)):
    """For the block: every allocator named in the module docstring returns, for a tensor with bytes whose device type is in
    ``devices`` and that is not page-locked, a tensor between two bands of ``byte``; every other tensor as before.  Yields a
    ``Guard``.  The originals are back on exit, also after an exception; the buffers live as long as the ``Guard`` holds
    them, so that no band is handed out again during the call or before ``check``."""
    if not 0 <= int(byte) <= 255:
        raise ValueError("a byte is 0 .. 255")
    state = Guard(byte, devices)
    saved = [(torch, name, getattr(torch, name), fills) for name, fills in _FILLERS]
    saved += [(torch.Tensor, name, getattr(torch.Tensor, name), fills) for name, fills in _METHODS]
    full, empty_strided = torch.full, torch.empty_strided

    def wrap(original, fills):
        def allocate(*args, **kwargs):
            like = original(*args, **kwargs)
            if (kwargs.get("out") is not None or not isinstance(like, torch.Tensor) or like.device.type not in state.devices
                    or like.numel() == 0 or like.is_sparse or (like.device.type == "cpu" and like.is_pinned())):
                return like
            buffer, start, tensor = _carve(like, state.byte, full, empty_strided)
            span = _span(like)
            buffer[start:start + span].zero_()
            if fills:
                tensor.copy_(like)
            if like.requires_grad:
                tensor.requires_grad_(True)
            state.records.append(Record(buffer, start, span, tensor, _site(), like.data_ptr() % 256))
            return tensor
        allocate.__name__ = getattr(original, "__name__", "allocate")
        allocate.__wrapped__ = original
        return allocate

    try:
        for owner, name, original, fills in saved:
            setattr(owner, name, wrap(original, fills))
        yield state
    finally:
        for owner, name, original, _ in saved:
            setattr(owner, name, original)


class Placed:
    """What ``place`` returns: ``tensor``, the copy inside the guarded buffer, and ``check_untouched``."""

    def __init__(self, buffer, start, span, tensor, byte, what):
        self.buffer, self.start, self.end, self.tensor, self.byte, self.what = buffer, start, start + span, tensor, byte, what
        self.snapshot = buffer.clone()

    def _owned(self):
        """A host mask of the buffer: the bytes of the view's own elements."""
        integer = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[self.tensor.element_size()]
        mask = torch.zeros_like(self.buffer)
        torch.empty((0,), dtype=integer, device=mask.device).set_(
            mask.untyped_storage(), self.start // self.tensor.element_size(), self.tensor.shape, self.tensor.stride()).fill_(-1)
        return mask.cpu().numpy() != 0

    def check_untouched(self, elements=True):
        """Every byte of the buffer (bands, padding between the rows and the view's own elements) as ``place`` left it.
        ``elements=False`` is for an argument that its entry point documents as written: its own elements may change, the
        bands and the padding may not."""
        if self.buffer.is_cuda:
            torch.cuda.synchronize()
        if torch.equal(self.buffer, self.snapshot):
            return
        bad = np.flatnonzero((self.buffer != self.snapshot).cpu().numpy())
        owned = self._owned()
        if not elements:
            bad = bad[~owned[bad]]
            if not bad.size:
                return
        found = []
        for which, sel, origin in (("front band", bad[bad < self.start], self.start), ("back band", bad[bad >= self.end], self.end),
                                   ("padding", bad[(bad >= self.start) & (bad < self.end) & ~owned[bad]], self.start),
                                   ("elements", bad[owned[bad]], self.start)):
            if sel.size:
                found.append("%s: %d bytes changed, first at %+d from the view's %s" % (
                    which, sel.size, int(sel[0]) - origin, "end" if origin == self.end else "start"))
        raise AssertionError("an input was written: %s of %s, strides %s (%s): %s" % (
            tuple(self.tensor.shape), self.tensor.dtype, self.tensor.stride(), self.what, "; ".join(found)))


def place(tensor, byte, what="an input"):
    """A copy of ``tensor`` inside a guarded buffer: the same shape, dtype and strides and the same address modulo 256 (an
    "aligned", "wide" or "shifted" view stays what it is), the bands and every byte of the span that is not an element of
    the view (the padding columns between the rows) filled with ``byte``.  Returns a ``Placed``."""
    if not 0 <= int(byte) <= 255:
        raise ValueError("a byte is 0 .. 255")
    if tensor.numel() == 0 or tensor.element_size() not in (1, 2, 4, 8):
        raise ValueError("place() takes a tensor with elements of 1, 2, 4 or 8 bytes")
    buffer, start, copy = _carve(tensor, int(byte), _original(torch.full), _original(torch.empty_strided))
    copy.copy_(tensor)
    return Placed(buffer, start, _span(tensor), copy, int(byte), what)
