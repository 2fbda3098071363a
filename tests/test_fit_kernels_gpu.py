"""libindextts_fit.so (include/indextts_fit.h) against float64 on the kernels' own operands, within the bounds tests/fit_refs.py
derives: ittf_lora_wgrad over every shape class (below, at and above a tile; more than one row chunk; ranks across the 16-row tiles),
ittf_sqnorm and ittf_adamw_step over segment tables, and every refusal of the header as a message."""
import ctypes as C
import itertools

import pytest
import torch

import fit_refs as FR

pytestmark = pytest.mark.gpu
DEV = "cuda"
MS = (1, 15, 16, 17, 63, 64, 65, 257, 1000)
RS = (1, 4, 16, 17, 64)
CS = (16, 80, 1280)
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
SENT = 7.25        # the sentinel around G and the workspace


@pytest.fixture(scope="module")
def nf():
    from indextts import _native_fit
    _native_fit.lib()
    return _native_fit


def operands(M, r, Cn, dtype, seed, extra_rows=3):
    """s [M + extra, r + 5] and z [M + extra, C + 3] of `dtype` (leading dimensions larger than the widths); the rows past M hold 1e30
    (s) and NaN (z); the columns past r / C hold values that must not reach G either."""
    g = torch.Generator().manual_seed(seed)
    s = torch.randn(M + extra_rows, r + 5, generator=g).to(dtype)
    z = torch.randn(M + extra_rows, Cn + 3, generator=g).to(dtype)
    s[M:] = 1e30
    z[M:] = float("nan")
    return s.to(DEV), z.to(DEV)


def run(nf, s, z, M, r, Cn, accumulate=False, scale=1.0, G0=None, ws_pad=64):
    """-> (G [r, C] as the kernel left it, the guard cells around G and ws intact?)"""
    G = torch.full((r + 2, Cn + 4), SENT, dtype=torch.float32, device=DEV)
    if G0 is not None:
        G[1: r + 1, 2: Cn + 2] = G0.to(DEV)
    need = nf.wgrad_ws_bytes(M, r, Cn)
    assert need == nf.lib().ittf_wgrad_ws_bytes(M, r, Cn)
    ws = torch.full((need + 2 * ws_pad,), 0x5A, dtype=torch.uint8, device=DEV)
    nf.lora_wgrad(s[:, :r], z[:, :Cn], G[1: r + 1, 2: Cn + 2], ws[ws_pad: ws_pad + need], M=M, accumulate=accumulate, scale=scale)
    out = G[1: r + 1, 2: Cn + 2].clone()
    G[1: r + 1, 2: Cn + 2] = SENT
    intact = bool((G == SENT).all()) and bool((ws[:ws_pad] == 0x5A).all()) and bool((ws[ws_pad + need:] == 0x5A).all())
    return out, intact


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "bf16", "f16"))
def test_wgrad_against_float64(nf, dtype):
    worst = 0.0
    for k, (M, r, Cn) in enumerate(itertools.product(MS, RS, CS)):
        s, z = operands(M, r, Cn, dtype, 100 + k)
        G, intact = run(nf, s, z, M, r, Cn)
        want, bound = FR.wgrad64(s, z, M, r, Cn)
        err = (G.double().cpu() - want).abs()
        assert torch.isfinite(G).all() and intact, (M, r, Cn)
        assert (err <= bound).all(), (M, r, Cn, float((err - bound).max()))
        worst = max(worst, float((err / bound.clamp_min(1e-30)).max()))
        if k % 7 == 0:                     # accumulate on, with a scale, onto a G of its own; and the same bits on a second run
            G0 = torch.randn(r, Cn, generator=torch.Generator().manual_seed(k))
            G1, intact = run(nf, s, z, M, r, Cn, accumulate=True, scale=0.37, G0=G0)
            want, bound = FR.wgrad64(s, z, M, r, Cn, scale=0.37, G0=G0)
            assert intact and ((G1.double().cpu() - want).abs() <= bound).all(), (M, r, Cn, "accumulate")
            G2, _ = run(nf, s, z, M, r, Cn, accumulate=True, scale=0.37, G0=G0)
            assert torch.equal(G1, G2)
            # other values in the rows past M: not one bit changes
            s2, z2 = s.clone(), z.clone()
            s2[M:], z2[M:] = float("nan"), 1e30
            assert torch.equal(run(nf, s2, z2, M, r, Cn)[0], G)
    print(f"{dtype}: worst |G - G64| / bound {worst:.3f}")


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "bf16", "f16"))
def test_wgrad_negative_controls_land_outside_the_bound(nf, dtype):
    """What the bound must catch: a row dropped, the last chunk skipped, the two leading dimensions swapped."""
    M, r, Cn = 600, 16, 80                                           # three chunks, the last of 88 rows
    s, z = operands(M, r, Cn, dtype, 9)
    want, bound = FR.wgrad64(s, z, M, r, Cn)
    G, _ = run(nf, s, z, M, r, Cn)
    assert ((G.double().cpu() - want).abs() <= bound).all()
    dropped, _ = run(nf, s, z, M - 1, r, Cn)                         # the last row left out
    assert ((dropped.double().cpu() - want).abs() > bound).any()
    skipped, _ = run(nf, s, z, 512, r, Cn)                           # the last chunk left out
    assert ((skipped.double().cpu() - want).abs() > bound).any()
    # leading dimensions swapped: s read at z's pitch (inside its buffer: as many rows as fit)
    flat_s = s.reshape(-1)
    lds, ldz = s.stride(0), z.stride(0)
    rows = flat_s.numel() // ldz
    s_sw = flat_s[: rows * ldz].view(rows, ldz)
    assert lds < Cn                                                  # (z cannot be read at a pitch under its width: s alone moves)
    sw, _ = run(nf, s_sw, z[:rows], rows, r, Cn)
    w_sw, b_sw = FR.wgrad64(s[:rows], z[:rows], rows, r, Cn)
    assert ((sw.double().cpu() - w_sw).abs() > b_sw).any()


def make_table(nf, lengths, dtype, seed, with_copy=True):
    g = torch.Generator().manual_seed(seed)
    entries, guards = [], []
    for i, n in enumerate(lengths):
        bufs = [torch.randn(n + 2, generator=g) for _ in range(4)]
        bufs[3] = bufs[3].abs() * 1e-3                                # v >= 0
        bufs[2] = bufs[2] * 1e-2
        bufs = [b.to(DEV) for b in bufs]
        t = torch.full((n + 2,), SENT, dtype=dtype, device=DEV) if with_copy and i % 3 != 2 else None
        guards.append((bufs, t))
        entries.append(tuple(b[1: n + 1] for b in bufs) + (None if t is None else t[1: n + 1], i % 2))
    return nf.SegmentTable(entries, DEV), guards


LENGTHS = (1, 3, 4, 5, 1023, 1024, 1025, 4096, 5000)


def test_sqnorm_against_float64(nf):
    for lengths in (LENGTHS, (1,), (5000, 1, 4095)):
        tab, guards = make_table(nf, lengths, torch.float32, 3)
        got = float(nf.sqnorm(tab).item())
        want = sum(float((b[1][1:-1].double() ** 2).sum()) for b, _ in guards)
        n = sum(lengths)
        assert abs(got - want) <= (n + 2) * FR.U * want, (lengths, got, want)
        assert float(nf.sqnorm(tab).item()) == got                    # the same bits
    assert nf.lib().ittf_sqnorm_ws_floats(4097) == 2


@pytest.mark.parametrize("dtype", DTYPES, ids=("f32", "bf16", "f16"))
@pytest.mark.parametrize("t,clip,wd", ((1, 1.0, 0.0), (1000, 0.37, 0.01), (1, 0.37, 0.1)))
def test_adamw_step_against_float64(nf, dtype, t, clip, wd):
    tab, guards = make_table(nf, LENGTHS, dtype, 11 + t)
    before = [[b.clone() for b in bufs] for bufs, _ in guards]
    lr = (1e-3, 2e-3)
    nf.adamw_step(tab, lr, (wd, wd), t, clip=clip)
    for i, ((bufs, tc), old) in enumerate(zip(guards, before)):
        p, g, m, v = (b[1:-1] for b in old)
        p2, m2, v2, dp, dm, dv = FR.adamw64(p, g, m, v, lr[i % 2], wd, t, clip=clip)
        for name, new, want, bound in (("p", bufs[0], p2, dp), ("m", bufs[2], m2, dm), ("v", bufs[3], v2, dv)):
            err = (new[1:-1].double().cpu() - want).abs()
            assert (err <= bound).all(), (i, name, float((err / bound).max()))
            assert new[0] == old[{"p": 0, "m": 2, "v": 3}[name]][0] and new[-1] == old[{"p": 0, "m": 2, "v": 3}[name]][-1]   # nothing past a segment
        assert torch.equal(bufs[1], old[1])                           # the gradient is read only
        assert not torch.equal(bufs[0][1:-1], old[0][1:-1])
        if tc is not None:                                            # the T copy: the device's master rounded once
            assert torch.equal(tc[1:-1], bufs[0][1:-1].to(dtype)) and float(tc[0]) == SENT and float(tc[-1]) == SENT


def test_refusals_are_messages(nf):
    L = nf.lib()

    def msg():
        return L.ittf_last_error().decode()
    s, z = operands(40, 4, 16, torch.float32, 1)
    G = torch.zeros(4, 16, device=DEV)
    ws = torch.zeros(nf.wgrad_ws_bytes(40, 4, 16) + 16, dtype=torch.uint8, device=DEV)

    def args(**kw):
        a = nf.WgradArgs()
        a.s, a.z, a.G, a.ws, a.ws_bytes = s.data_ptr(), z.data_ptr(), G.data_ptr(), ws.data_ptr(), ws.numel() - 16
        a.M, a.r, a.C, a.lds, a.ldz, a.ldg, a.dtype, a.accumulate, a.scale = 40, 4, 16, s.stride(0), z.stride(0), 16, nf.F32, 0, 1.0
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    assert L.ittf_lora_wgrad(C.byref(args()), None) == 0
    for kw, text in ((dict(s=None), "null pointer"), (dict(ws=None), "null pointer"), (dict(G=G.data_ptr() + 2), "aligned"),
                     (dict(ws=ws.data_ptr() + 4), "aligned"), (dict(s=s.data_ptr() + 2), "aligned"), (dict(r=0), "r = 0"),
                     (dict(r=65), "r = 65"), (dict(M=0), "M must be"), (dict(C=0), "C = 0"), (dict(lds=3), "lds = 3"),
                     (dict(ldz=15), "ldz = 15"), (dict(ldg=15), "ldg = 15"), (dict(dtype=3), "dtype = 3"),
                     (dict(ws_bytes=nf.wgrad_ws_bytes(40, 4, 16) - 1), "ws too small"), (dict(G=s.data_ptr()), "overlaps")):
        assert L.ittf_lora_wgrad(C.byref(args(**kw)), None) == 1, kw
        assert text in msg(), (kw, msg())
    assert L.ittf_lora_wgrad(None, None) == 1 and "null argument struct" in msg()
    assert L.ittf_wgrad_ws_bytes(0, 4, 16) == 0 and L.ittf_wgrad_ws_bytes(40, 65, 16) == 0
    tab, _ = make_table(nf, (5, 7), torch.float32, 2)
    out, w = torch.zeros(1, device=DEV), torch.zeros(4, device=DEV)
    sq = L.ittf_sqnorm
    assert sq(tab.table.data_ptr(), 2, 12, w.data_ptr(), 4, out.data_ptr(), None) == 0
    for a, text in (((None, 2, 12, w.data_ptr(), 4, out.data_ptr()), "null segment table"),
                    ((tab.table.data_ptr() + 8, 2, 12, w.data_ptr(), 4, out.data_ptr()), "16-byte aligned"),
                    ((tab.table.data_ptr(), 0, 12, w.data_ptr(), 4, out.data_ptr()), "n_seg = 0"),
                    ((tab.table.data_ptr(), 2, 0, w.data_ptr(), 4, out.data_ptr()), "total = 0"),
                    ((tab.table.data_ptr(), 2, 12, None, 4, out.data_ptr()), "null pointer"),
                    ((tab.table.data_ptr(), 2, 12, w.data_ptr(), 0, out.data_ptr()), "ws too small"),
                    ((tab.table.data_ptr(), 2, 12, w.data_ptr(), 4, w.data_ptr()), "overlaps")):
        assert sq(*a, None) == 1, a
        assert text in msg(), (a, msg())

    def adam(**kw):
        a = nf.AdamwArgs()
        a.table, a.n_seg, a.dtype, a.total = tab.table.data_ptr(), 2, nf.F32, 12
        a.lr[0] = a.lr[1] = 1e-3
        a.beta1, a.beta2, a.eps, a.bc1, a.bc2_sqrt, a.clip = 0.9, 0.999, 1e-8, 0.1, 0.03, 1.0
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    assert L.ittf_adamw_step(C.byref(adam()), None) == 0
    for kw, text in ((dict(table=None), "null segment table"), (dict(n_seg=70000), "n_seg"), (dict(dtype=5), "dtype = 5"),
                     (dict(beta1=1.0), "beta1"), (dict(eps=0.0), "eps"), (dict(bc1=0.0), "bias corrections"), (dict(clip=1.5), "clip")):
        assert L.ittf_adamw_step(C.byref(adam(**kw)), None) == 1, kw
        assert text in msg(), (kw, msg())
    torch.cuda.synchronize()
