"""The guard-band helper (tests/_guard.py) itself, on the CPU."""
import pytest
import torch

from _guard import BACK, FRONT, POISON, SENTINEL, SENTINEL_BYTE, arena, assert_intact, bit_equal, guarded


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32, torch.int64, torch.int32])
@pytest.mark.parametrize("fill", [POISON, SENTINEL])
def test_arena_keeps_contents_contiguity_alignment(dtype, fill):
    t = (torch.arange(5 * 24).reshape(5, 24) % 97).to(dtype)
    buf, view = arena(t, fill)
    assert view.shape == t.shape and view.dtype == t.dtype and view.is_contiguous()
    assert torch.equal(view, t)
    off = view.data_ptr() - buf.data_ptr()
    assert off == FRONT and off % 128 == 0 and off % 256 != 0
    es = t.element_size()
    assert buf.numel() * es == FRONT + t.numel() * es + BACK
    front, back = buf[: FRONT // es], buf[FRONT // es + t.numel():]
    if fill == SENTINEL:
        assert (front.view(torch.uint8) == SENTINEL_BYTE).all() and (back.view(torch.uint8) == SENTINEL_BYTE).all()
    elif t.is_floating_point():
        assert torch.isnan(front).all() and torch.isnan(back).all()
    else:
        assert (front == 0).all() and (back == 0).all()  # index margins hold a valid index
    view.add_(1)  # a view into buf, not a copy
    assert torch.equal(buf[FRONT // es: FRONT // es + t.numel()].view(t.shape), t + 1)
    assert_intact(buf, view)


@pytest.mark.parametrize("fill", [POISON, SENTINEL])
@pytest.mark.parametrize("where", ["front_first", "front_last", "back_first", "back_last"])
def test_assert_intact_sees_one_flipped_byte(fill, where):
    t = torch.randn(3, 8).to(torch.bfloat16)
    buf, view = arena(t, fill)
    assert_intact(buf, view)
    view.zero_()  # writes inside the operand are not the margins' business
    assert_intact(buf, view)
    nbytes = t.numel() * 2
    pos, rel = {"front_first": (0, -FRONT), "front_last": (FRONT - 1, -1),
                "back_first": (FRONT + nbytes, nbytes), "back_last": (FRONT + nbytes + BACK - 1, nbytes + BACK - 1)}[where]
    buf.view(torch.uint8)[pos] ^= 1
    with pytest.raises(AssertionError, match=rf"offset {rel} relative"):
        assert_intact(buf, view)
    buf.view(torch.uint8)[pos] ^= 1
    assert_intact(buf, view)


def test_bitwise_nan_comparison():
    nan = torch.full((4,), float("nan"))
    assert not torch.equal(nan, nan) and bit_equal(nan, nan)
    other = nan.clone()
    other.view(torch.int32)[2] ^= 1  # another NaN payload
    assert torch.isnan(other).all() and not bit_equal(nan, other)
    assert bit_equal(torch.tensor([0.0]), torch.tensor([0.0])) and not bit_equal(torch.tensor([0.0]), torch.tensor([-0.0]))
    # a NaN margin rewritten with the same NaN is unchanged, with any other value it is not
    buf, view = arena(torch.zeros(8), POISON)
    buf[0] = float("nan")
    assert_intact(buf, view)
    buf[0] = 0.0
    with pytest.raises(AssertionError, match="margin byte"):
        assert_intact(buf, view)


def test_guarded_flags_leaks_and_spills():
    x = torch.randn(4, 8)

    def good(x, y):
        y.copy_(x * 2)
        return x.sum(1)

    out, io = guarded(good, {"x": x}, {"y": torch.zeros(4, 8)}, name="good")
    assert torch.equal(out[0], x.sum(1)) and torch.equal(io["y"], x * 2)

    def reads_before(x, y):  # one element in front of the operand reaches the result
        flat = x.as_strided((x.numel() + 1,), (1,), x.storage_offset() - 1) if x.storage_offset() else x.reshape(-1)
        y.copy_(x)
        return flat.sum().reshape(1) * 0

    with pytest.raises(AssertionError, match="non-finite"):
        guarded(reads_before, {"x": x}, {"y": torch.zeros(4, 8)}, name="leak")

    def writes_after(x, y):
        n = y.numel() + (2 if y.storage_offset() else 0)
        y.as_strided((n,), (1,), y.storage_offset()).fill_(1.0)

    with pytest.raises(AssertionError, match=r"offset 128 relative"):
        guarded(writes_after, {"x": x}, {"y": torch.zeros(4, 8)}, name="spill")
