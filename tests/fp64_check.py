"""Per-element fp64 parity helpers shared by test_vocoder_kernels_gpu.py, test_decode_kernels_gpu.py and the front-end files: the grid spacing of a
16-bit storage type at a reference value, the worst err / bound ratio of a tensor with the element it sits at, and the two
assertions built on it (`check`: every element within its bound; `must_fail`: a deliberately wrong reference is NOT), the
reporting wrappers `ok` / `bad` that print one `fp64 | kind | case | ratio` line per check (the profiles/*_fp64.txt files), and
what the decode and the front-end references share: `rnd`, the `fold_rows` operand rows and one key tile of an online-softmax
walk with its error bookkeeping (`walk_start` / `walk_step`)."""
import math

import numpy as np
import torch

PREC = {torch.float16: (11, -14), torch.bfloat16: (8, -126), torch.float32: (24, -126)}   # significand bits, smallest normal exponent


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


def tname(dtype):
    return "f32" if dtype == torch.float32 else "f16" if dtype == torch.float16 else "bf16"


def note(kind, what, ratio):
    print(f"fp64 | {kind} | {what} | {ratio:.3f}")


def ok(what, y, ref, bound, valid=None):
    note("case", what, check(what, y, ref, bound, valid))


def bad(what, control, y, ref, bound, valid=None):
    note("control", f"{what}: {control}", must_fail(what, control, y, ref, bound, valid))


def rnd(*shape, seed=0, scale=1.0, device="cpu"):
    """Seeded float64 normal values, drawn on the CPU (the same on every device) and moved to `device`."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g, dtype=torch.float64) * scale).to(device)


def fold_rows(M, K, seed, device="cpu"):
    """Raw residual rows for a LayerNorm: sigma 1, and by row index mod 4 a common offset of 0, 8 and 64 sigma and a row with
    one outlier feature (GPT-2 residual streams have both)."""
    h = rnd(M, K, seed=seed, device=device)
    r = torch.arange(M, device=device)
    h[r % 4 == 1] += 8.0
    h[r % 4 == 2] += 64.0
    h[r % 4 == 3, min(7, K - 1)] = 60.0
    return h


def walk_start(H, Q, device):
    """The empty state of an online-softmax walk over [H][Q] rows: (m, l, O, Ab, Em, Ed, dbar, nbar), see `walk_step`."""
    z = lambda n: torch.zeros(H, Q, n, dtype=torch.float64, device=device)  # noqa: E731
    return (torch.full((H, Q, 1), -math.inf, dtype=torch.float64, device=device), z(1), z(64), z(64), z(64), z(64), z(1), z(1))


def walk_step(state, st, dt, vt, dtype, sum_rounded, exact=False):
    """One key tile of the walk a flash-attention kernel makes: scores st [H][Q][n] (-inf: not visible), their relative fp32-level
    distance dt from the kernel's, values vt [H][n][64] (float64 of the storage type).  The running maximum moves, the state is
    rescaled, P = exp(s - m) is rounded to the storage type for the product with V (not with exact=True), and the normaliser l
    sums the rounded P (sum_rounded) or the unrounded one.  Next to O the state carries the ingredients of the bound:
    Ab = sum P |v|; Em = sum near_j ulp_T(P_j) |v_j| with near_j flagging a P_j whose rounding the kernel's fp32 value may take the
    other way (within dt P of a midpoint); Ed = sum P dt |v|; dbar = sum P dt; nbar = sum near_j ulp_T(P_j).
    Returns (state, near)."""
    m, l, O, Ab, Em, Ed, dbar, nbar = state
    mn = torch.maximum(m, st.max(-1, keepdim=True).values)
    ms = torch.where(torch.isinf(mn), torch.zeros_like(mn), mn)
    corr = torch.where(torch.isinf(m), torch.zeros_like(m), torch.exp(m - ms))
    P = torch.exp(st - ms)
    Pr = P if exact else P.to(dtype).double()
    near = ((0.5 * ulp(P, dtype) - (P - Pr).abs()) <= dt * P) & (P > 0)
    if exact:
        near = torch.zeros_like(near)
    flip = torch.where(near, ulp(P, dtype), torch.zeros_like(P))
    va = vt.abs()
    return (mn, l * corr + (Pr if sum_rounded else P).sum(-1, keepdim=True), O * corr + Pr @ vt, Ab * corr + Pr @ va,
            Em * corr + flip @ va, Ed * corr + (P * dt) @ va, dbar * corr + (P * dt).sum(-1, keepdim=True),
            nbar * corr + flip.sum(-1, keepdim=True)), near
