"""Guard bands for kernel tests: operands placed inside a larger allocation whose margins are
either poisoned (NaN: a read outside the operand that reaches the result shows up as NaN or as a
difference from the plain run) or hold a sentinel (a write outside an output changes a margin byte).

A helper module, not a conftest: tests import what they use.

    buf, view = arena(t, POISON)        # view == t, NaN on both sides
    ...run the kernel on view...
    assert_intact(buf, view)            # no margin byte changed

``guarded(fn, inputs, inouts)`` does both runs and every comparison for one kernel call.
"""
from __future__ import annotations

import torch

POISON = "poison"      # NaN for floating dtypes; 0 (a valid index / an empty keep word) for integers
SENTINEL = "sentinel"  # every byte 0xA5: bf16 0xA5A5 = -7.2e-17, fp32 0xA5A5A5A5 = -2.9e-16 (finite)
SENTINEL_BYTE = 0xA5
FRONT = 4096 + 128     # operand at 128-byte but not 256-byte alignment (the flat store's weakest)
BACK = 4096


def _bytes(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.uint8)


def arena(t: torch.Tensor, fill: str = POISON, front: int = FRONT, back: int = BACK):
    """(buf, view): ``view`` has ``t``'s shape, dtype and contents, is contiguous and lives inside the
    1-D ``buf`` with ``front`` bytes before and ``back`` bytes after it, both filled with ``fill``."""
    es, n = t.element_size(), t.numel()
    if front % 128 or back % es or front < 128:
        raise ValueError("arena: front must be a multiple of 128 bytes, back of the element size")
    buf = torch.empty(front // es + n + back // es, dtype=t.dtype, device=t.device)
    if fill == SENTINEL:
        _bytes(buf).fill_(SENTINEL_BYTE)
    elif fill == POISON:
        buf.fill_(float("nan") if t.is_floating_point() else 0)
    else:
        raise ValueError(f"arena: unknown fill {fill!r}")
    view = buf[front // es: front // es + n].view(t.shape)
    view.copy_(t)
    b = _bytes(buf)
    buf._guard = (front, n * es, b[:front].clone(), b[front + n * es:].clone())
    return buf, view


def assert_intact(buf: torch.Tensor, view: torch.Tensor, what: str = "operand") -> None:
    """Both margins of ``buf`` around ``view`` are bitwise what ``arena`` left there; on failure the
    first changed byte's offset relative to the operand's first byte is reported."""
    front, nbytes, before, after = buf._guard
    assert view.data_ptr() - buf.data_ptr() == front and view.numel() * view.element_size() == nbytes
    b = _bytes(buf)
    for got, want, origin in ((b[:front], before, -front), (b[front + nbytes:], after, nbytes)):
        if not torch.equal(got, want):
            i = int((got != want).nonzero()[0].item())
            raise AssertionError(
                f"{what}: margin byte at offset {origin + i} relative to the operand "
                f"({nbytes} bytes long) changed: {int(want[i]):#04x} -> {int(got[i]):#04x}, "
                f"{int((got != want).sum())} margin bytes differ on this side")


def bit_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Bitwise equality (NaN == NaN of the same payload), through an integer view."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return torch.equal(_bytes(a.contiguous().reshape(-1)), _bytes(b.contiguous().reshape(-1)))


def _flat(out):
    if out is None:
        return []
    if isinstance(out, torch.Tensor):
        return [out]
    return [o for o in out if isinstance(o, torch.Tensor)]


def guarded(fn, inputs: dict, inouts: dict | None = None, approx: dict | None = None, name: str = "",
            skip: tuple = ()):
    """Run ``fn(**inputs, **inouts)`` on plain tensors, then with every input in a POISON arena and
    every caller-provided output / in-place buffer in a SENTINEL arena.

    * every floating output (returned tensors and the in-place buffers) of both runs is finite;
    * the guarded run equals the plain run: ``torch.equal``, or ``assert_close(atol, rtol)`` for the
      names in ``approx`` (returned tensors are named ``"out0"``, ``"out1"``, ...): outputs summed
      with cross-workgroup atomics, whose order is not fixed;
    * no margin changed.

    ``skip`` names tensors whose VALUES are not looked at (a workspace, or an output with elements
    the kernel leaves unspecified); their margins still are.  ``None`` values and empty tensors pass
    through.  Returns (returned tensors, in-place buffers) of the PLAIN run, so
    the caller can go on to check values."""
    inouts = inouts or {}
    approx = approx or {}
    plain_io = {k: (v.clone() if v is not None else None) for k, v in inouts.items()}
    plain_out = _flat(fn(**inputs, **plain_io))
    bufs, gin, gio = {}, {}, {}
    for k, v in inputs.items():
        if isinstance(v, torch.Tensor) and v.numel():
            bufs[k], gin[k] = arena(v, POISON)
        else:
            gin[k] = v
    for k, v in inouts.items():
        if v is None:
            gio[k] = None
        else:
            bufs[k], gio[k] = arena(v, SENTINEL)
    g_out = _flat(fn(**gin, **gio))
    assert len(g_out) == len(plain_out), f"{name}: {len(g_out)} outputs, the plain run {len(plain_out)}"
    pairs = [(f"out{i}", g, p) for i, (g, p) in enumerate(zip(g_out, plain_out))]
    pairs += [(k, gio[k], plain_io[k]) for k in inouts if inouts[k] is not None]
    for k, g, p in pairs:
        if k in skip:
            continue
        if g.is_floating_point():
            assert torch.isfinite(p).all(), f"{name}: {k} of the plain run is not finite"
            bad = ~torch.isfinite(g)
            assert not bad.any(), (f"{name}: {k} has {int(bad.sum())} non-finite values with poisoned "
                                   f"margins, first at flat index {int(bad.reshape(-1).nonzero()[0])}")
        if k in approx:
            atol, rtol = approx[k]
            torch.testing.assert_close(g, p, atol=atol, rtol=rtol, msg=lambda m: f"{name}: {k}: {m}")
        else:
            assert torch.equal(g, p), (f"{name}: {k} differs from the plain run at "
                                       f"{int((g != p).sum())} of {g.numel()} elements")
    for k, buf in bufs.items():
        view = gin[k] if k in gin else gio[k]
        assert_intact(buf, view, f"{name}: {k}")
    return plain_out, plain_io
