"""Per-element fp64 parity helpers shared by test_vocoder_kernels_gpu.py and test_decode_kernels_gpu.py: the grid spacing of a
16-bit storage type at a reference value, the worst err / bound ratio of a tensor with the element it sits at, and the two
assertions built on it (`check`: every element within its bound; `must_fail`: a deliberately wrong reference is NOT)."""
import math

import numpy as np
import torch

PREC = {torch.float16: (11, -14), torch.bfloat16: (8, -126)}   # significand bits, smallest normal exponent


def ulp(v, dtype):
    """Spacing of the storage type's grid at |v| (subnormal spacing below the smallest normal), float64."""
    p, emin = PREC[dtype]
    _, e = torch.frexp(v)
    e = torch.where(v == 0, torch.full_like(e, emin), torch.clamp(e - 1, min=emin))
    return torch.ldexp(torch.ones_like(v), e - (p - 1))


def excess(y, ref, bound, valid=None):
    """(worst err / bound, message parts) over the elements selected by `valid` (bool, broadcastable) or all."""
    err = (y.double() - ref).abs()
    r = torch.where(torch.isfinite(err), err / bound, torch.full_like(err, math.inf))
    if valid is not None:
        r = torch.where(valid, r, torch.zeros_like(r))
    i = int(torch.argmax(r))
    idx = tuple(int(v) for v in np.unravel_index(i, tuple(r.shape)))
    return r.flatten()[i].item(), (idx, y.double().flatten()[i].item(), ref.flatten()[i].item(),
                                   err.flatten()[i].item(), bound.flatten()[i].item())


def check(what, y, ref, bound, valid=None):
    ratio, (idx, got, want, err, b) = excess(y, ref, bound, valid)
    assert ratio <= 1.0, (f"{what}: worst element {idx}: got {got!r} want {want!r} err {err:.3e} > bound {b:.3e} "
                          f"({ratio:.2f}x)")
    return ratio


def must_fail(what, control, y, ref, bound, valid=None):
    ratio, (idx, _, _, err, b) = excess(y, ref, bound, valid)
    assert ratio > 1.0, f"{what}: negative control '{control}' passed (worst {ratio:.2f}x of the bound at {idx}): the bound cannot discriminate"
    return ratio
