"""tests/guard.py itself, on host memory (``devices=("cpu",)``): the check sees a store one element outside a tensor at
either end and into a padding column of a placed view, and sees none where there is none; every hooked allocator gives what
the original gives.  Every overrun here is made with ``torch.as_strided`` over the helper's own storage, so that it lands
in the helper's own band: nothing is written outside memory the test owns.  No GPU."""
import pytest
import torch

import guard

CPU = ("cpu",)


def _beyond(t, elements):
    """A view of ``elements`` elements of ``t``'s storage starting ``elements`` before ``t`` (negative) or at its end."""
    flat = t.reshape(-1)
    assert flat.is_contiguous() and flat.data_ptr() == t.data_ptr()
    offset = t.storage_offset() + (t.numel() if elements > 0 else elements)
    return torch.as_strided(t, (abs(elements),), (1,), offset)


def test_a_tensor_written_in_full_passes():
    with guard.guarded(0xFF, CPU) as state:
        out = torch.empty((5, 7), dtype=torch.int32)
        assert not out.any()                                      # the interior is 0x00 under every byte
        out.fill_(3)
        work = torch.zeros(11, dtype=torch.float64)
        work += 1.5
        state.check()
    assert state.allocations == 2
    state.check()                                                 # the buffers outlive the block


def test_a_store_one_element_past_the_end():
    with guard.guarded(0x7F, CPU) as state:
        out = torch.empty((5, 7), dtype=torch.int32)
        out.fill_(3)
        _beyond(out, 1).fill_(3)
        with pytest.raises(AssertionError) as err:
            state.check()
    message = str(err.value)
    assert "back band of (5, 7) of torch.int32 allocated at" in message and "test_guard.py:" in message
    assert "4 bytes damaged, first at +0 from the tensor's end" in message and "front band" not in message


def test_a_store_one_element_before_the_start():
    with guard.guarded(0xFF, CPU) as state:
        torch.empty(3, dtype=torch.float32).fill_(1.0)
        out = torch.zeros((4, 2), dtype=torch.float64)
        _beyond(out, -1).fill_(2.0)
        with pytest.raises(AssertionError) as err:
            state.check()
    message = str(err.value)
    assert "front band of (4, 2) of torch.float64 allocated at" in message and "back band" not in message
    assert "8 bytes damaged, first at -8 from the tensor's start" in message and "(3,)" not in message


def test_a_store_a_row_past_the_end_and_a_single_byte():
    with guard.guarded(0xFF, CPU) as state:
        out = torch.empty((3, 6), dtype=torch.int16)
        _beyond(out, 6)[5:].fill_(-2)                             # the last element of "row 3": one byte differs from 0xFF
        with pytest.raises(AssertionError, match=r"back band .* 1 bytes damaged, first at \+10 from the tensor's end"):
            state.check()


@pytest.mark.parametrize("layout", ["aligned", "wide", "shifted"])
def test_a_placed_view_keeps_its_geometry_and_sees_a_store_into_a_padding_column(layout):
    G = 5
    ld, shift = {"aligned": (8, 0), "wide": (G + 1, 0), "shifted": (G + 4, 1)}[layout]
    wide = torch.full((3, ld), 12345, dtype=torch.int32)
    wide[:, shift:shift + G] = torch.arange(3 * G, dtype=torch.int32).reshape(3, G)
    view = wide[:, shift:shift + G]
    placed = guard.place(view, 0x7F)
    copy = placed.tensor
    assert copy.shape == view.shape and copy.dtype == view.dtype and copy.stride() == view.stride()
    assert copy.data_ptr() % 256 == view.data_ptr() % 256 and torch.equal(copy, view)
    padding = torch.as_strided(copy, (3, ld), (ld, 1), copy.storage_offset())[:2, G:]
    assert padding.numel() and bool((padding == 0x7F7F7F7F).all())           # the padding columns hold the byte
    placed.check_untouched()
    (copy * 2).sum()                                              # reading is no write
    placed.check_untouched()
    padding[1, 0] = 6
    with pytest.raises(AssertionError) as err:
        placed.check_untouched()
    assert "padding: 4 bytes changed, first at %+d from the view's start" % (4 * (ld + G)) in str(err.value)
    assert "band" not in str(err.value) and "elements" not in str(err.value)


def test_a_placed_input_sees_a_write_to_its_elements_and_to_either_band():
    placed = guard.place(torch.arange(6, dtype=torch.int32).reshape(2, 3), 0x00, "the panel")
    placed.check_untouched()
    placed.tensor[1, 2] = -250                                    # 0x00000005 to 0xFFFFFF06
    with pytest.raises(AssertionError, match=r"the panel\): elements: 4 bytes changed, first at \+20 from the view's start"):
        placed.check_untouched()
    placed = guard.place(torch.zeros(6, dtype=torch.int64), 0xFF)
    _beyond(placed.tensor, 1).fill_(0)
    _beyond(placed.tensor, -1).fill_(0)
    with pytest.raises(AssertionError) as err:
        placed.check_untouched()
    assert "front band: 8 bytes changed, first at -8 from the view's start" in str(err.value)
    assert "back band: 8 bytes changed, first at +0 from the view's end" in str(err.value)


_LIKE = torch.arange(24, dtype=torch.int16).reshape(2, 3, 4).permute(2, 0, 1)          # empty_like keeps these strides

ALLOCATORS = {
    "empty": lambda: torch.empty((3, 5), dtype=torch.float64),
    "empty, sizes as arguments": lambda: torch.empty(3, 5, dtype=torch.int32, device="cpu"),
    "empty_like": lambda: torch.empty_like(_LIKE),
    "empty_strided": lambda: torch.empty_strided((3, 5), (7, 1), dtype=torch.float32),
    "zeros": lambda: torch.zeros((4, 3), dtype=torch.int64),
    "zeros_like": lambda: torch.zeros_like(_LIKE),
    "ones": lambda: torch.ones(9, dtype=torch.float32),
    "ones_like": lambda: torch.ones_like(_LIKE, dtype=torch.float64),
    "full": lambda: torch.full((2, 6), -7, dtype=torch.int32),
    "full, a float": lambda: torch.full((5,), 2.5),
    "full_like": lambda: torch.full_like(_LIKE, 11),
    "new_empty": lambda: _LIKE.new_empty((4, 4)),
    "new_zeros": lambda: _LIKE.new_zeros(6, dtype=torch.uint8),
    "new_ones": lambda: _LIKE.new_ones((2, 2)),
    "new_full": lambda: _LIKE.new_full((3,), 5),
}


def test_every_allocator_of_the_helper_is_tried():
    assert {name.split(",")[0] for name in ALLOCATORS} == {name for name, _ in guard._FILLERS + guard._METHODS}


@pytest.mark.parametrize("name", list(ALLOCATORS))
@pytest.mark.parametrize("byte", [0x00, 0xFF, 0x7F])
def test_every_hooked_allocator_returns_what_the_original_does(name, byte):
    want = ALLOCATORS[name]()
    with guard.guarded(byte, CPU) as state:
        got = ALLOCATORS[name]()
    assert state.allocations == 1 and got.data_ptr() != want.data_ptr()
    record = state.records[0]
    assert got.shape == want.shape and got.dtype == want.dtype and got.stride() == want.stride() and got.device == want.device
    assert record.buffer.data_ptr() + record.start == got.data_ptr() and got.data_ptr() % 256 == record.mod
    assert record.mod % 64 == 0                                   # the original's own remainder: torch aligns host memory to 64
    assert record.start >= guard.BAND and record.buffer.numel() - record.end >= guard.BAND
    assert record.end - record.start == guard._span(want)        # the back band starts at the tensor's last byte
    if "empty" in name:
        assert not got.any()
    else:
        assert torch.equal(got, want)
    assert bool((record.buffer[:record.start] == byte).all()) and bool((record.buffer[record.end:] == byte).all())
    state.check()


def test_host_tensors_pass_through_when_the_device_is_guarded_and_a_tensor_without_bytes_always():
    with guard.guarded(0xFF) as state:                            # devices = ("cuda",)
        assert torch.empty(5).numel() == 5 and torch.zeros((2, 2), dtype=torch.int32).sum() == 0
    assert state.allocations == 0
    with guard.guarded(0xFF, CPU) as state:
        assert torch.empty((0, 4)).shape == (0, 4) and torch.zeros(0).numel() == 0
        out = torch.empty(4)
        assert torch.empty(3, out=out[:3]).data_ptr() == out.data_ptr()
    assert state.allocations == 1


def test_the_originals_are_restored_after_an_exception():
    before = [getattr(torch, name) for name, _ in guard._FILLERS] + [getattr(torch.Tensor, name) for name, _ in guard._METHODS]
    with pytest.raises(RuntimeError, match="inside the block"):
        with guard.guarded(0x7F, CPU):
            assert torch.empty is not before[0] and torch.empty.__wrapped__ is before[0]
            raise RuntimeError("inside the block")
    after = [getattr(torch, name) for name, _ in guard._FILLERS] + [getattr(torch.Tensor, name) for name, _ in guard._METHODS]
    assert all(a is b for a, b in zip(after, before))
    with pytest.raises(ValueError):
        with guard.guarded(256, CPU):
            pass
    assert torch.empty is before[0]


def test_a_block_that_allocates_nothing_counts_nothing():
    with guard.guarded(0x00, CPU) as state:
        torch.arange(5) + 1
        state.check()
    assert state.allocations == 0


def test_the_site_is_the_first_frame_under_the_package():
    """An allocation is named by the wrapper's line under prosstt_amd/, not by the test's or the helper's."""
    import os
    path = os.path.join(os.sep + "somewhere", "prosstt_amd", "wrapper.py")
    scope = {"torch": torch}
    exec(compile("\n\ndef allocate():\n    return torch.zeros((2, 3))\n", path, "exec"), scope)
    with guard.guarded(0x00, CPU) as state:
        scope["allocate"]()
        torch.empty(3)
    assert state.records[0].site == "prosstt_amd/wrapper.py:4" and "test_guard.py:" in state.records[1].site
    scope["allocate"]()                                           # (outside the block: an ordinary tensor, nothing recorded)
    assert state.allocations == 2


def test_the_band_is_the_stated_condition():
    assert guard.BAND == 65536 and guard.BAND % 256 == 0 and guard.BAND // (2051 * 4) == 7 and guard.BAND > 7.98 * 2051 * 4


def test_a_written_argument_may_change_its_elements_but_not_its_padding():
    wide = torch.zeros((2, 6), dtype=torch.int32)
    placed = guard.place(wide[:, 1:4], 0xFF, "out")
    placed.tensor.fill_(9)
    placed.check_untouched(elements=False)
    with pytest.raises(AssertionError, match="elements: 6 bytes changed"):
        placed.check_untouched()
    torch.as_strided(placed.tensor, (1,), (1,), placed.tensor.storage_offset() + 3).fill_(9)
    with pytest.raises(AssertionError, match=r"out\): padding: 4 bytes changed, first at \+12 from the view's start$"):
        placed.check_untouched(elements=False)


def test_every_library_has_a_guard_band_test():
    """The census: a library added to prosstt_amd._native cannot be forgotten in tests/test_gpu_guard_bands.py."""
    import test_gpu_guard_bands as bands
    from prosstt_amd import _native
    names = set(_native.LIBRARIES) | set(_native.ADDED_LIBRARIES) | set(_native.LATER_LIBRARIES)
    assert bands.NOT_ON_THE_DEVICE == {"host"} and bands.NOT_ON_THE_DEVICE <= names
    assert set(bands.LIBRARIES) == names - bands.NOT_ON_THE_DEVICE
    assert all(callable(shared) and callable(smallest) for shared, smallest in bands.LIBRARIES.values())


def test_place_inside_a_guarded_block_uses_the_original_allocators():
    with guard.guarded(0x7F, CPU) as state:
        placed = guard.place(torch.arange(5), 0x7F)
    assert state.allocations == 0 and torch.equal(placed.tensor, torch.arange(5))
    placed.check_untouched()
