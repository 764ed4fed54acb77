"""tests/stale.py without a device: the value every byte gives per dtype, the whole storage of every allocator's tensor,
empty_like of a strided view, the counter, and the originals back after the block and after an exception."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import stale  # noqa: E402

ALLOCATORS = ("empty", "empty_like", "empty_strided")


def _originals():
    return [torch.empty, torch.empty_like, torch.empty_strided, torch.Tensor.new_empty]


def test_fill_values_per_dtype():
    assert stale.BYTES == (0x00, 0xFF, 0x7F)
    with stale.poisoned(0x00) as p:
        for dtype in (torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8, torch.int16):
            assert bool((torch.empty(7, dtype=dtype) == 0).all())
        assert p.fills == 6
    with stale.poisoned(0xFF) as p:
        assert bool(torch.isnan(torch.empty((3, 5), dtype=torch.float32)).all())
        assert bool(torch.isnan(torch.empty((3, 5), dtype=torch.float64)).all())
        for dtype in (torch.int32, torch.int64, torch.int16):
            assert bool((torch.empty(9, dtype=dtype) == -1).all())
        assert bool((torch.empty(9, dtype=torch.uint8) == 255).all())
    with stale.poisoned(0x7F) as p:
        f32 = torch.empty(4, dtype=torch.float32).numpy()
        f64 = torch.empty(4, dtype=torch.float64).numpy()
        assert np.all(f32 == np.frombuffer(b"\x7f" * 4, np.float32)[0]) and 3.39e38 < f32[0] < 3.4e38
        assert np.all(f64 == np.frombuffer(b"\x7f" * 8, np.float64)[0]) and 1.38e306 < f64[0] < 1.39e306
        assert bool((torch.empty(4, dtype=torch.int32) == 2139062143).all())
        assert bool((torch.empty(4, dtype=torch.int64) == 0x7F7F7F7F7F7F7F7F).all())
        assert bool((torch.empty(4, dtype=torch.uint8) == 127).all())


def test_every_allocator_fills_its_whole_storage():
    base = torch.zeros((6, 10), dtype=torch.int32)
    view = base[:, 2:7]                                          # strided: rows of 5 in a pitch of 10
    assert not view.is_contiguous()
    with stale.poisoned(0x7F) as p:
        made = [torch.empty((3, 4), dtype=torch.int32), torch.empty(3, 4, dtype=torch.int32), torch.empty_like(view),
                torch.empty_like(view, dtype=torch.float64), torch.empty_strided((4, 3), (8, 2), dtype=torch.int32),
                base.new_empty((2, 5)), view.new_empty(11, dtype=torch.int64)]
        assert p.fills == len(made)
        assert tuple(made[2].shape) == (6, 5) and made[2].dtype == torch.int32
        assert tuple(made[3].shape) == (6, 5) and made[3].dtype == torch.float64
        assert made[4].stride() == (8, 2)
        for t in made:
            raw = np.frombuffer(bytes(t.untyped_storage()), np.uint8)
            assert raw.size >= t.numel() * t.element_size() and np.all(raw == 0x7F)
        gaps = made[4].untyped_storage().nbytes()                # the bytes between the strided entries as well
        assert gaps > made[4].numel() * 4
        torch.empty(0, dtype=torch.float32)                      # no bytes: nothing to fill, not counted
        torch.empty((5, 0), dtype=torch.int64)
        assert p.fills == len(made)
    assert bool((base == 0).all())                               # the tensor a view was taken of is left alone


def test_the_counter_counts_calls_made_elsewhere():
    def library_code():
        import torch as t
        a = t.empty(5, dtype=t.float32)
        return a, t.empty_like(a), a.new_empty(3)

    with stale.poisoned(0xFF) as p:
        assert p.fills == 0 and p.byte == 0xFF
        out = library_code()
        assert p.fills == 3 and all(bool(torch.isnan(o).all()) for o in out)
    before = p.fills
    library_code()
    assert p.fills == before                                     # outside the block nothing is counted


def test_originals_are_back_after_exit_and_after_an_exception():
    originals = _originals()
    with stale.poisoned(0x00):
        assert all(now is not was for now, was in zip(_originals(), originals))
        with stale.poisoned(0xFF) as inner:                      # nested: the inner byte, then the outer one again
            assert bool((torch.empty(3, dtype=torch.int32) == -1).all())
        assert inner.fills == 1 and bool((torch.empty(3, dtype=torch.int32) == 0).all())
    assert all(now is was for now, was in zip(_originals(), originals))
    with pytest.raises(KeyError):
        with stale.poisoned(0x7F):
            raise KeyError("inside")
    assert all(now is was for now, was in zip(_originals(), originals))
    for bad in (-1, 256):
        with pytest.raises(ValueError):
            with stale.poisoned(bad):
                pass
    assert all(now is was for now, was in zip(_originals(), originals))
