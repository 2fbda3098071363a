"""The yardstick of the fit's training attention (ittf_attn_fwd / ittf_attn_bwd): a float64 restatement of
the ragged causal attention and of its gradient, written out from the formulas (no autograd), the same graph in fp32 torch on the CPU
as FitEngine._forward's loop states it (autograd), and the builder of the kernel tests' cases.  Shared by tests/test_fit_attn_*.py;
nothing here calls the library.

Layout, as include/indextts_fit.h: qkv [M, ld] with q of head h at columns 64 h .. 64 h + 63, k at D + 64 h, v at 2 D + 64 h
(D = 64 H); out and dout [M, ldo] with head h at column 64 h; lse [H, M]; segments = [(first row, row count)]: rows of one segment
attend causally to one another only, rows outside every segment belong to nobody.

THE ERROR RULE (tests/test_fit_engine_gpu.py's): per output tensor over a whole case e32 = max |x32 - x64| / max |x64| with x32 the
fp32 CPU graph; the device may err max(4 e32, 2^-18) on the same norm; lse absolutely 2^-18 max(1, max |lse64|).
"""
import torch

FLOOR = 2.0 ** -18
SENTINEL = -12345.0
TILE = 16          # the kernels' tile: the case lengths 15 / 16 / 17, 63 / 64 / 65 are those around it and around a 64-row block
LENGTHS = (1, 2, 15, 16, 17, 63, 64, 65, 130, 257)


def attention64(qkv, dout, segments, H, scale=0.125, dtype=torch.float64):
    """-> out [M, D], lse [H, M], dqkv [M, 3 D] in `dtype` from the formulas; rows outside the segments are zero."""
    D = 64 * H
    x, g = qkv[:, : 3 * D].to(dtype), dout[:, :D].to(dtype)
    M = x.shape[0]
    out, lse, dx = torch.zeros(M, D, dtype=dtype), torch.zeros(H, M, dtype=dtype), torch.zeros(M, 3 * D, dtype=dtype)
    for f, n in segments:
        keep = torch.ones(n, n, dtype=torch.bool).tril()
        for h in range(H):
            c = slice(64 * h, 64 * h + 64)
            q, k, v = x[f: f + n, c], x[f: f + n, D + 64 * h: D + 64 * h + 64], x[f: f + n, 2 * D + 64 * h: 2 * D + 64 * h + 64]
            s = (q @ k.t() * scale).masked_fill(~keep, float("-inf"))
            m = s.max(dim=1, keepdim=True).values
            l = torch.exp(s - m).sum(dim=1, keepdim=True)
            lse[h, f: f + n] = (m + torch.log(l))[:, 0]
            p = torch.exp(s - m) / l
            o = p @ v
            out[f: f + n, c] = o
            do = g[f: f + n, c]
            delta = (do * o).sum(dim=1, keepdim=True)
            ds = p * (do @ v.t() - delta)
            dx[f: f + n, c] = scale * (ds @ k)
            dx[f: f + n, D + 64 * h: D + 64 * h + 64] = scale * (ds.t() @ q)
            dx[f: f + n, 2 * D + 64 * h: 2 * D + 64 * h + 64] = p.t() @ do
    return out, lse, dx


def attention_graph(qkv, dout, segments, H, dtype=torch.float32):
    """The loop of FitEngine._forward on the CPU in `dtype`, its backward by autograd -> out [M, D], dqkv [M, 3 D] (uncovered rows
    zero).  The scale is the loop's own 0.125."""
    D = 64 * H
    x = qkv[:, : 3 * D].to(dtype).clone().requires_grad_(True)
    M = x.shape[0]
    out = torch.zeros(M, D, dtype=dtype)
    with torch.enable_grad():
        parts = []
        for f, n in segments:
            causal = torch.ones(n, n, dtype=torch.bool).tril()
            q, k, v = x[f: f + n].view(n, 3, H, 64).permute(1, 2, 0, 3)
            sc = (torch.matmul(q, k.transpose(-1, -2)) * 0.125).masked_fill(~causal, float("-inf"))
            a = torch.matmul(torch.softmax(sc, dim=-1), v).permute(1, 0, 2).reshape(n, D)
            parts.append((f, n, a))
        total = sum((a * dout[f: f + n, :D].to(dtype)).sum() for f, n, a in parts)
        total.backward()
    for f, n, a in parts:
        out[f: f + n] = a.detach()
    return out, x.grad.detach()


def split(dx, segments, H):
    """dqkv [M, 3 D] -> (dq, dk, dv), each the covered rows' [sum n, D]."""
    D = 64 * H
    rows = torch.cat([torch.arange(f, f + n) for f, n in segments])
    return tuple(dx[rows][:, j * D: (j + 1) * D] for j in range(3))


def layout(lengths, first=5, gap=3):
    """Segments of `lengths` with first rows that are no multiple of 16 and gaps between them -> (segments, M with a tail)."""
    segs, at = [], first
    for n in lengths:
        if at % 16 == 0:
            at += 1
        segs.append((at, n))
        at += n + gap
    return segs, at + 2


def case(lengths, H, std_qk=1.0, seed=0, first=5, gap=3, pad_ld=8, pad_ldo=4, spike=None):
    """A case of the kernel tests: q, k of standard deviation std_qk, v and dout of 1, every uncovered entry of qkv and dout NaN
    (rows in the gaps and the tail, and the columns past 3 D / D of every row).  spike = (segment index, key row): that key is
    200 u and every query of the segment gets 8 u added (u a unit vector per head): its score stands about 200 above the others'."""
    g = torch.Generator().manual_seed(seed)
    D = 64 * H
    segs, M = layout(lengths, first, gap)
    ld, ldo = 3 * D + pad_ld, D + pad_ldo
    qkv, dout = torch.full((M, ld), float("nan")), torch.full((M, ldo), float("nan"))
    for i, (f, n) in enumerate(segs):
        x = torch.randn(n, 3 * D, generator=g)
        x[:, : 2 * D] *= std_qk
        if spike is not None and spike[0] == i:
            u = torch.randn(H, 64, generator=g)
            u = (u / u.norm(dim=1, keepdim=True)).reshape(D)
            x[:, :D] = torch.randn(n, D, generator=g) + 8.0 * u
            x[:, D: 2 * D] = torch.randn(n, D, generator=g)
            x[spike[1], D: 2 * D] = 200.0 * u
        qkv[f: f + n, : 3 * D] = x
        dout[f: f + n, :D] = torch.randn(n, D, generator=g)
    return dict(qkv=qkv, dout=dout, segments=segs, M=M, H=H, ld=ld, ldo=ldo)


def clean(c):
    """(qkv [M, 3 D], dout [M, D]) of a case with zeros in the place of the NaNs: what the references take."""
    D = 64 * c["H"]
    return torch.nan_to_num(c["qkv"][:, : 3 * D], nan=0.0), torch.nan_to_num(c["dout"][:, :D], nan=0.0)


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-300))
