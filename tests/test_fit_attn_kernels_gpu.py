"""ittf_attn_fwd / ittf_attn_bwd through the C ABI (include/indextts_fit.h) against the float64 restatement of
tests/fit_attn_refs.py on the same fp32 operands, under the project's measured rule: per output tensor over a whole case
e32 = max |x32 - x64| / max |x64| with x32 the fp32 torch graph on the CPU, and the device may err max(4 e32, 2^-18); lse absolutely
2^-18 max(1, max |lse64|).  Every run reads operands whose uncovered rows and columns are NaN and writes into buffers pre-filled with
a sentinel, with guard floats past ld M and ldo M: every covered entry must come out finite and every other one intact.
The measured figures are recorded in profiles/fit_attn.txt."""
import ctypes as C

import pytest
import torch

import fit_attn_refs as AR

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 64
# lengths from AR.LENGTHS (the kernels' tile is 16: 15 / 16 / 17 are the lengths around it), several per launch, every case with a
# segment of at least 17 rows; q and k at standard deviation 1 and 4
CASES = {
    "h1_small": dict(lengths=(1, 2, 15, 16, 17, 63), H=1, std_qk=1.0, seed=1),
    "h3_std4": dict(lengths=(64, 65, 130, 17), H=3, std_qk=4.0, seed=2),
    "h20": dict(lengths=(257, 1, 17), H=20, std_qk=1.0, seed=3),
    "h3_long_std4": dict(lengths=(130, 257, 16, 2), H=3, std_qk=4.0, seed=4, first=21, gap=1),
    "spike_late": dict(lengths=(130, 17), H=1, seed=5, spike=(0, 100)),
    "spike_first": dict(lengths=(130, 17), H=1, seed=6, spike=(0, 3)),
}


def guarded(t):
    """A host tensor [M, ld] -> (flat device buffer with GUARD sentinel floats behind it, its [M, ld] view)."""
    flat = torch.full((t.numel() + GUARD,), AR.SENTINEL, dtype=torch.float32, device=DEV)
    flat[: t.numel()] = t.reshape(-1).to(DEV)
    return flat, flat[: t.numel()].view(t.shape)


def run(c, scale=0.125):
    """One forward and one backward of a case on the device -> dict(out [M, D], lse, dqkv [M, 3 D]) on the host, after the checks
    every run gets: covered entries finite, every sentinel intact."""
    from indextts import _native_fit as nf
    M, H, ld, ldo, D = c["M"], c["H"], c["ld"], c["ldo"], 64 * c["H"]
    rows = nf.AttnRows(c["segments"], M, DEV)
    qf, qkv = guarded(c["qkv"])
    gf, dout = guarded(c["dout"])
    of, out = guarded(torch.full((M, ldo), AR.SENTINEL))
    xf, dqkv = guarded(torch.full((M, ld), AR.SENTINEL))
    lf, lse = guarded(torch.full((H, M), AR.SENTINEL))
    nf.attn_fwd(qkv, rows, H, scale, out=out, lse=lse)
    nf.attn_bwd(qkv, lse, dout, rows, H, scale, dqkv=dqkv)
    torch.cuda.synchronize()
    covered = torch.zeros(M, dtype=torch.bool)
    for f, n in c["segments"]:
        covered[f: f + n] = True
    out, dqkv, lse = out.cpu(), dqkv.cpu(), lse.cpu()
    assert torch.isfinite(out[covered][:, :D]).all() and torch.isfinite(dqkv[covered][:, : 3 * D]).all() and torch.isfinite(lse[:, covered]).all()
    sent = lambda t: bool((t == AR.SENTINEL).all())                                         # noqa: E731
    assert sent(out[~covered]) and sent(out[:, D:]) and sent(dqkv[~covered]) and sent(dqkv[:, 3 * D:]) and sent(lse[:, ~covered])
    for flat, n in ((of, M * ldo), (xf, M * ld), (lf, H * M)):
        assert sent(flat[n:].cpu())
    assert torch.equal(qf.cpu()[: M * ld].view(M, ld).nan_to_num(7.0), c["qkv"].nan_to_num(7.0))   # (the inputs are as they were)
    assert torch.equal(gf.cpu()[: M * ldo].view(M, ldo).nan_to_num(7.0), c["dout"].nan_to_num(7.0))
    return dict(out=out[:, :D].clone(), lse=lse.clone(), dqkv=dqkv[:, : 3 * D].clone())


@pytest.fixture(scope="module")
def refs():
    """Per case, computed once: (case, float64 (out, lse, dqkv), fp32 graph (out, dqkv))."""
    table = {}
    for name, kw in CASES.items():
        c = AR.case(**kw)
        qkv, dout = AR.clean(c)
        table[name] = (c, AR.attention64(qkv, dout, c["segments"], c["H"]), AR.attention_graph(qkv, dout, c["segments"], c["H"]))
    return table


@pytest.mark.parametrize("name", list(CASES))
def test_kernels_against_float64(refs, name):
    """Measured on an MI355X (profiles/fit_attn.txt): every tensor of every case is inside the rule, the worst at 0.32 of what is
    allowed (the spike cases at 0.03 .. 0.10).  With delta = rowsum(dout o out) in the place of sum_j p dP the two spike cases
    missed it on dq alone, 4.2 and 4.7 times the allowance: behind the spike ds = dP - delta is a difference of equal numbers, which
    sum_j p dP cancels bit for bit and rowsum(dout o out) only to the rounding of out, and dq multiplies it by the spike key."""
    c, (o64, lse64, dx64), (o32, dx32) = refs[name]
    assert max(n for _, n in c["segments"]) >= 17 and all(f % 16 for f, _ in c["segments"]) and c["ld"] > 192 * c["H"] and c["ldo"] > 64 * c["H"]
    got = run(c)
    segs, H = c["segments"], c["H"]
    rows = torch.cat([torch.arange(f, f + n) for f, n in segs])
    pairs = [("out", got["out"][rows], o64[rows], o32[rows])]
    pairs += [(nm, g, w, x) for nm, g, w, x in zip(("dq", "dk", "dv"), AR.split(got["dqkv"], segs, H), AR.split(dx64, segs, H), AR.split(dx32, segs, H))]
    bad = []
    for nm, g, w, x in pairs:
        e32, ed = AR.rel(x, w), AR.rel(g, w)
        allowed = max(4 * e32, AR.FLOOR)
        print(f"{name} {nm}: e32 {e32:.3e}, device {ed:.3e}, allowed {allowed:.3e}, ratio {ed / allowed:.3f}")
        if not ed <= allowed:
            bad.append((nm, e32, ed))
    el = float((got["lse"][:, rows].double() - lse64[:, rows]).abs().max())
    al = AR.FLOOR * max(1.0, float(lse64[:, rows].abs().max()))
    print(f"{name} lse: max |lse| {float(lse64[:, rows].abs().max()):.3f}, device error {el:.3e}, allowed {al:.3e}, ratio {el / al:.3f}")
    assert not bad and el <= al, (bad, el, al)


@pytest.mark.parametrize("name", ["spike_late", "spike_first"])
def test_spike_cases_run_the_rescale_with_an_underflowing_factor(refs, name):
    """What makes the spike cases what they are, from the float64 scores: in every query tile at or behind the spike its score
    exceeds every earlier key's by more than 80 -- exp(-80) of the running sums is left -- and by more than 104, where the fp32
    factor is zero, in at least one."""
    c = refs[name][0]
    (f, n), j = c["segments"][0], CASES[name]["spike"][1]
    q, k = c["qkv"][f: f + n, :64].double(), c["qkv"][f: f + n, 64: 128].double()
    s = q @ k.t() * 0.125
    margins = []
    for i in range(j if j else 1, n):
        if j:
            margins.append(float(s[i, j] - s[i, :j].max()))
        others = torch.cat([s[i, :j], s[i, j + 1: i + 1]])
        assert float(s[i, j] - others.max()) > 80, (i, float(s[i, j] - others.max()))
    assert not j or (min(margins) > 80 and max(margins) > 104)
    assert (j // 16 > 0) == (name == "spike_late")


def test_same_operands_same_bits(refs):
    c = refs["h3_std4"][0]
    a, b = run(c), run(c)
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_a_segment_gives_the_same_bits_alone_and_among_others(refs):
    """The 130-row segment of h3_std4 alone at row 0 with ld = 3 D and ldo = D against the same rows among three others at row 149
    under ld = 3 D + 8 and ldo = D + 4; and the 257-row segment of h20 likewise."""
    for name, idx in (("h3_std4", 2), ("h20", 0)):
        c = refs[name][0]
        f, n = c["segments"][idx]
        H, D = c["H"], 64 * c["H"]
        assert f > 0 and len(c["segments"]) > 1
        alone = dict(qkv=c["qkv"][f: f + n, : 3 * D].clone(), dout=c["dout"][f: f + n, :D].clone(), segments=[(0, n)], M=n, H=H, ld=3 * D, ldo=D)
        among, single = run(c), run(alone)
        assert torch.equal(among["out"][f: f + n], single["out"]) and torch.equal(among["lse"][:, f: f + n], single["lse"])
        assert torch.equal(among["dqkv"][f: f + n], single["dqkv"])


def test_one_row_segment_has_zero_dq_and_dk(refs):
    c = refs["h20"][0]
    f, n = c["segments"][1]
    assert n == 1
    got = run(c)
    D = 64 * c["H"]
    # p = 1, so out = v and dv = dout bit for bit; delta = fma(1, dP, 0) is dP itself, ds = dP - delta = 0 and dq = dk = 0
    assert torch.equal(got["dqkv"][f, 2 * D:], c["dout"][f, :D]) and torch.equal(got["out"][f], c["qkv"][f, 2 * D: 3 * D])
    assert not got["dqkv"][f, : 2 * D].any()


def test_refusals():
    """Every refusal of the header as ITTF_ERR_INVALID with its message; a valid call returns 0 first."""
    from indextts import _native_fit as nf
    L = nf.lib()
    H, M, D = 2, 40, 128
    rows = nf.AttnRows([(3, 20), (25, 9)], M, DEV)
    qkv = torch.randn(M, 3 * D, device=DEV)
    out, lse = torch.zeros(M, D, device=DEV), torch.zeros(H, M, device=DEV)
    dout, dqkv = torch.randn(M, D, device=DEV), torch.zeros(M, 3 * D, device=DEV)
    ws = torch.empty(nf.attn_ws_bytes(M, H), dtype=torch.uint8, device=DEV)

    def args(**kw):
        a = nf.AttnArgs()
        a.qkv, a.out, a.lse, a.dout, a.dqkv, a.ws = (t.data_ptr() for t in (qkv, out, lse, dout, dqkv, ws))
        a.ws_bytes, a.table, a.M, a.n_seg, a.max_len, a.H, a.ld, a.ldo, a.scale = ws.numel(), rows.table.data_ptr(), M, 2, 20, H, 3 * D, D, 0.125
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    assert L.ittf_attn_fwd(C.byref(args()), None) == 0 and L.ittf_attn_bwd(C.byref(args()), None) == 0
    assert L.ittf_attn_bwd(C.byref(args(out=None)), None) == 0                                # (the backward does not read out)
    torch.cuda.synchronize()
    both, fwd, bwd = (L.ittf_attn_fwd, L.ittf_attn_bwd), (L.ittf_attn_fwd,), (L.ittf_attn_bwd,)
    for fns, kw, msg in ((both, dict(qkv=None), "null pointer (qkv, out, lse, table)"), (fwd, dict(out=None), "null pointer (qkv"),
                         (both, dict(lse=None), "null pointer (qkv"), (both, dict(table=None), "null pointer (qkv"),
                         (bwd, dict(dout=None), "null pointer (dout, dqkv, ws)"), (bwd, dict(dqkv=None), "null pointer (dout"),
                         (bwd, dict(ws=None), "null pointer (dout"),
                         (both, dict(H=0), "H = 0"), (both, dict(H=nf.ATTN_MAX_HEADS + 1), "heads of 64 columns"),
                         (both, dict(ld=3 * D - 4), "ld = 380 (the pitch of qkv: >= 3 D = 384"), (both, dict(ld=3 * D + 2), "a multiple of 4"),
                         (both, dict(ldo=D - 4), "ldo = 124 (the pitch of out: >= D = 128"), (both, dict(ldo=D + 1), "a multiple of 4"),
                         (both, dict(qkv=qkv.data_ptr() + 4), "must be 16-byte aligned"), (fwd, dict(out=out.data_ptr() + 8), "must be 16-byte aligned"),
                         (both, dict(lse=lse.data_ptr() + 2), "lse 4-byte aligned"), (both, dict(table=rows.table.data_ptr() + 8), "16-byte aligned"),
                         (bwd, dict(dout=dout.data_ptr() + 4), "dout and dqkv must be 16-byte aligned"),
                         (bwd, dict(dqkv=dqkv.data_ptr() + 4), "dout and dqkv must be 16-byte aligned"),
                         (fwd, dict(out=qkv.data_ptr()), "out or lse overlaps"), (fwd, dict(lse=out.data_ptr()), "out or lse overlaps"),
                         (bwd, dict(dqkv=qkv.data_ptr()), "dqkv or ws overlaps"), (bwd, dict(ws=dout.data_ptr()), "dqkv or ws overlaps"),
                         (bwd, dict(ws=dqkv.data_ptr()), "dqkv overlaps ws"),
                         (both, dict(max_len=nf.ATTN_MAX_SEG + 1), f"a segment has 1 .. {nf.ATTN_MAX_SEG} rows"), (both, dict(max_len=0), "max_len = 0"),
                         (both, dict(n_seg=0), "n_seg = 0"), (both, dict(n_seg=nf.ATTN_MAX_NSEG + 1), "n_seg = 65536"),
                         (both, dict(M=0), "M must be in [1, 2^31)"), (both, dict(M=2 ** 31), "M must be in [1, 2^31)"),
                         (both, dict(scale=0.0), "scale = 0"), (both, dict(scale=float("nan")), "finite and > 0"),
                         (bwd, dict(ws_bytes=ws.numel() - 1), "ws too small")):
        for fn in fns:
            assert fn(C.byref(args(**kw)), None) == 1, (kw, msg)
            assert msg in L.ittf_last_error().decode(), (kw, msg, L.ittf_last_error().decode())
    for fn in both:
        assert fn(None, None) == 1 and "null argument struct" in L.ittf_last_error().decode()
    assert L.ittf_attn_ws_bytes(M, H) == 4 * M * H and L.ittf_attn_ws_bytes(M, 0) == 0 and L.ittf_attn_ws_bytes(2 ** 31, H) == 0
    with pytest.raises(ValueError, match="the longest the kernels take"):
        nf.AttnRows([(0, nf.ATTN_MAX_SEG + 1)], 2 * nf.ATTN_MAX_SEG, DEV)
    torch.cuda.synchronize()
    assert not out[:3].any() and not dqkv[23:25].any()                                       # (the valid call wrote the covered rows only)
