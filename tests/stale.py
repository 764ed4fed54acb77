"""Control over what "uninitialised" memory holds.  ``poisoned(byte)`` replaces torch's four allocators of uninitialised
tensors for the duration of a block; each allocates as before and then fills the tensor's whole storage with ``byte``.  A
kernel that reads a slot before it writes it, or leaves an output element unwritten, then gives results that differ between
bytes, where a fresh process, which gets zero pages from the allocator most of the time, shows nothing.

    0x00   zeros of every type
    0xFF   NaN in float32 and float64, -1 in the integer types
    0x7F   3.39e38 (float32), 1.38e306 (float64), 2139062143 (int32), 9187201950435737471 (int64)

Out of reach: memory that native code allocates itself, tensors allocated before the block was entered, and allocations
made inside torch's own operators (``x.clone()``, ``torch.zeros``: those are written in full by the operator).  What lies
AROUND an allocation, a store or a load past its end, is tests/guard.py's.  A helper: nothing here is collected."""
import contextlib

import torch

BYTES = (0x00, 0xFF, 0x7F)


class Poison:
    """What ``poisoned`` yields: ``byte``, and ``fills``, the tensors filled so far."""

    def __init__(self, byte):
        self.byte, self.fills = int(byte), 0


def _fill(t, state):
    """Every byte of the storage behind ``t`` set to the poison (on the current stream for device memory)."""
    if not isinstance(t, torch.Tensor) or t.device.type == "meta":
        return t
    storage = t.untyped_storage()
    if storage.nbytes() == 0:
        return t
    raw = torch.tensor([], dtype=torch.uint8, device=t.device).set_(storage)
    raw.fill_(state.byte)
    state.fills += 1
    return t


@contextlib.contextmanager
def poisoned(byte):
    """For the block: ``torch.empty``, ``torch.empty_like``, ``torch.empty_strided`` and ``torch.Tensor.new_empty`` fill
    what they return, device and page-locked or pageable host memory alike, nothing for a tensor without bytes.  Yields a
    ``Poison`` that counts the fills.  The originals are back on exit, also after an exception."""
    if not 0 <= int(byte) <= 255:
        raise ValueError("a byte is 0 .. 255")
    state = Poison(byte)
    saved = [(torch, "empty", torch.empty), (torch, "empty_like", torch.empty_like),
             (torch, "empty_strided", torch.empty_strided), (torch.Tensor, "new_empty", torch.Tensor.new_empty)]

    def wrap(original):
        def allocate(*args, **kwargs):
            return _fill(original(*args, **kwargs), state)
        allocate.__name__ = getattr(original, "__name__", "allocate")
        allocate.__wrapped__ = original
        return allocate

    try:
        for owner, name, original in saved:
            setattr(owner, name, wrap(original))
        yield state
    finally:
        for owner, name, original in saved:
            setattr(owner, name, original)
