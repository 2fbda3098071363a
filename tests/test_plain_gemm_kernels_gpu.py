"""fp64 parity of every kernel form itts_gemm_conv runs at taps = 1 (csrc/gemm_conv.hip: gemm_plain_kernel in its two tile shapes,
with and without split-K, and the tiled convolution kernel's forms a plain GEMM reaches), element by element, with derived bounds --
the counterpart of test_vocoder_kernels_gpu.py, test_decode_kernels_gpu.py and test_frontend_kernels_gpu.py for the GEMM of the GPT
prefill, the latent pass, the conditioner's embed projection and the adapter bank.

Every case (tests/plain_gemm_refs.py: CASES, with the reference, the bounds and the controls; tests/test_plain_gemm_refs_cpu.py proves
on the CPU that the reference is torch's float64 formula and that every control leaves its bound) draws its operands in float64,
rounds them to the storage type, makes ONE launch and compares it with the float64 reference on those rounded operands:
  * itts_last_kernel() must name the form tests/plain_forms.py derives from dispatch_conv's rules for that shape; the form goes
    into PINNED, the epilogue kind into KINDS.  test_plain_every_reachable_form_is_pinned holds PINNED against every form string
    dispatch_conv can return for taps = 1 in the three dtypes (the narrow forms are the vocoder file's);
  * y is prefilled with a finite non-zero sentinel (7 .. 11 by element index) -- or with the seeded previous values where the
    epilogue reads it (accumulate, resid = y) -- and is followed by 16 guard rows that must come back bit for bit;
  * x is followed by 128 rows of NaN: rows >= M of a tile are read through a range-checked descriptor, and a kernel that read them
    (or a neighbouring batch element's, or a neighbouring K slice's columns) would put NaN, or a wrong sum, into an output;
  * the bound is per element (fp64_check.check names the worst one): ulp_T(ref) + 2^-21 S for a T output, 2^-21 S for an fp32 one,
    1.13 * 2^-21 S + 2^-21 |ref| more behind gelu_new, and the derived term G32 for gelu_new into fp32 (plain_gemm_refs);
  * split-K: every slab is held to the product over its own K slice, with its own S;
  * negative controls (plain_gemm_refs.CONTROLS) on the first case of every family at which they can differ: each re-evaluates
    the reference only, and must fail.

The shapes are the smallest that reach each path: M around one 128-row tile; K of 1 - 5 k-steps (every path through the prologue
and the 4-step chunks), a half-empty k-step, 1280 + 32 and 5120; 5 and 9 m-blocks under L2 patches of 4 and 8; slices of 13 / 13 / 14
steps, of one step, and 64 of them; the first row count at which the round rule picks 128 x 160 tiles on the part the test runs on.

test_production_plain_gemms_are_pinned_and_hold_fp64 records every gemm_conv call of a bf16 prefill and latent pass of 32 rows (two
full-width layers: every block makes the same four calls), with and without an adapter bank, and of the conditioner, requires
every form and epilogue kind to be a pinned one, and re-runs every distinct signature against the reference at its own size.

Every check prints one line `fp64 | kind | case | worst err / bound`; profiles/plain_gemm_fp64.txt is that output.
"""
import inspect

import pytest
import torch

import plain_forms as forms
import plain_gemm_refs as R
from fp64_check import bad, ok

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, F16, BF16 = R.F32, R.F16, R.BF16
GUARD, NAN_ROWS = 16, 128
PINNED = set()          # form strings of the cases that have run
KINDS = set()           # their epilogue kinds
GMS = set()             # L2 patch heights of the tile-order cases that have run
RUNS = [(i, dt) for i, c in enumerate(R.CASES) for dt in c.dts]


@pytest.fixture(scope="module")
def nat():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from indextts import _native
    _native.lib()
    return _native


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def sentinel(n, dtype):
    return (torch.arange(n, device=DEV) % 5 + 7).to(dtype)


def run_case(nat, c, dtype, pin=True):
    """One launch of case c against its float64 reference; returns the form that ran."""
    what = f"{R.TAG[dtype]} {c}"
    o = R.operands(c, dtype, device=DEV)
    yt, nb = c.out_dtype(dtype), max(c.B, c.ks)
    n = nb * c.M * c.N
    ybuf = sentinel(n + GUARD * c.N, yt)
    y = ybuf[:n].view(nb, c.M, c.N)
    if c.acc:
        y.copy_(o["y_prev"])
    if c.resid == "alias":
        y.copy_(o["resid"])
    xbuf = torch.full((c.B * c.M + NAN_ROWS, c.K), float("nan"), dtype=dtype, device=DEV)
    xbuf[:c.B * c.M] = o["x"].view(c.B * c.M, c.K)
    wp = nat.pack_weight(o["w"])
    resid = y if c.resid == "alias" else o["resid"]
    nat.gemm_conv(dtype, c.B, c.M, c.M, c.K, c.N, wp, xbuf, y, bias=o["bias"], bias2=o["bias2"], act=c.act, y_f32=c.y_f32 or c.ks > 1,
                  resid=resid, accumulate=c.acc, scale=c.scale, ksplit=c.ks)
    form = nat.last_kernel()
    want = forms.form(R.TAG[dtype], c.B, c.M, c.N, c.K, c.ks, cus())
    assert form == want, f"{what}: ran {form}, dispatch_conv's rules give {want}"
    if pin:
        PINNED.add(form)
        KINDS.add(c.kind)
    what = f"{what} [{form}]"
    assert torch.equal(ybuf[n:], sentinel(n + GUARD * c.N, yt)[n:]), f"{what}: the guard rows behind y were written"
    assert torch.isfinite(y).all(), f"{what}: a NaN row behind x reached the output"
    ref, S, pre = R.plain_ref(c, dtype, o)
    bound = R.bound(c, dtype, ref, S, pre)
    ok(what, y, ref, bound)
    for name in c.ctl:
        bad(what, R.CONTROLS[name], y, R.plain_ref(c, dtype, o, ctl=name)[0], bound)
    return form


@pytest.mark.parametrize("run", RUNS, ids=lambda r: f"{R.TAG[r[1]]}-{R.CASES[r[0]]}".replace(" ", "_"))
def test_plain_gemm_fp64(nat, run):
    """One case of plain_gemm_refs.CASES in one dtype (see the module docstring)."""
    i, dtype = run
    c = R.CASES[i].at(cus())
    form = run_case(nat, c, dtype)
    tag = R.TAG[dtype]
    if c.fam in ("m-edge", "k-edge", "tile-order", "split-k") or (c.fam in ("epilogue", "fp32") and c.N in (128, 256)):
        assert form == f"gemm_plain<{tag},2,4,4,2>", form
    if c.fam == "wide":
        assert form == (f"gemm_plain<{tag},4,2,2,5>" if c.M > 300 else f"gemm_plain<{tag},2,4,4,2>"), form
    if R.CASES[i].M == "wide":
        assert form == f"gemm_plain<{tag},4,2,2,5>" and c.M % 128 == 128 - 57, (form, c.M)
    if c.fam == "n64":
        assert form == (f"gemm_conv<{tag},4,2,4,2,4,0>" if c.B == 150 else f"gemm_conv<{tag},4,2,2,2,4,0>"), form
    if c.fam == "fall-through" or c.N == 1282:
        assert form == {96: f"gemm_conv<{tag},2,2,4,3,2,64,persist>", 144: f"gemm_conv<{tag},4,1,4,3,2,64>"}.get(c.N, f"gemm_conv<{tag},4,1,4,2,2,64>"), form
    if c.fam == "tile-order":
        gm, mb = forms.l2_patch_gm(128, c.K // forms.kstep(tag)), (c.M + 127) // 128
        assert mb > gm and mb % gm != 0 and (mb * (c.N // 128)) % 8 != 0     # one full patch, one partial, a grid that is no multiple of 8
        GMS.add(gm)


def test_plain_tile_order_ran_under_both_patch_heights():
    """l2_patch_gm gives 4 m-blocks per patch at K = 64 and 8 at K = 1664 (the rule is restated in plain_forms): both ran."""
    if not GMS:
        pytest.skip("no tile-order case ran in this process (the cases above fill GMS: run the whole file)")
    assert GMS == {4, 8}, GMS


def test_plain_split_k_refuses_a_bias(nat):
    """Slabs carry no bias, residual or activation: refused, nothing launched, nothing written."""
    M, N, K = 129, 128, 1280
    x = torch.zeros(M, K, dtype=BF16, device=DEV)
    wp = nat.pack_weight(torch.zeros(K, N, dtype=BF16, device=DEV))
    slab = sentinel(2 * M * N, F32)
    b = torch.zeros(N, device=DEV)
    for kw in (dict(bias=b), dict(act=1), dict(resid=slab), dict(accumulate=True)):
        with pytest.raises(nat.NativeError):
            nat.gemm_conv(BF16, 1, M, M, K, N, wp, x, slab, y_f32=True, ksplit=2, **kw)
        assert nat.last_kernel() == ""
    with pytest.raises(nat.NativeError):
        nat.gemm_conv(BF16, 1, M, M, K, N, wp, x, slab, ksplit=2)                  # slabs are fp32
    with pytest.raises(nat.NativeError):
        nat.gemm_conv(BF16, 1, M, M, K, N, wp, x, slab, y_f32=True, ksplit=41)     # more slices than k-steps
    assert torch.equal(slab, sentinel(2 * M * N, F32))


def test_plain_every_reachable_form_is_pinned():
    """PINNED against every form string dispatch_conv can return for taps = 1 (plain_forms.REACHABLE), in the three dtypes."""
    if not PINNED:
        pytest.skip("no case ran in this process (the cases of this file fill PINNED: run the whole file)")
    assert PINNED <= forms.REACHABLE, sorted(PINNED - forms.REACHABLE)
    missing = sorted(forms.REACHABLE - PINNED)
    assert not missing, f"reachable forms no case pins: {missing}"


# ------------------------------------------------------------------------------------------------- production
def call_kind(a, y):
    """The epilogue kind of a recorded call, named as plain_gemm_refs.Case.kind names a case's."""
    if a["ksplit"] > 1:
        return "slab"
    r = a["resid"]
    parts = [n for n, on in (("bias", a["bias"] is not None), ("bias2", a["bias2"] is not None), ("gelu", a["act"] == 1),
                             ("resid=" + ("alias" if r is not None and r.data_ptr() == y.data_ptr() else "own"), r is not None),
                             ("scale", a["scale"] != 1.0), ("acc", bool(a["accumulate"]))) if on]
    return "+".join(parts or ["store"]) + ("->f32" if a["y_f32"] else "->T")


@pytest.fixture(scope="module")
def production(nat):
    """(form, M, N, K, kind, ksplit, dtype) of every taps = 1 gemm_conv call of: the conditioner on a 300-frame prompt, the prefill of 32
    rows (texts of 20 - 60 tokens) and the latent pass over 80 codes per row, on a bf16 engine of two full-width layers (D = 1280,
    synthetic weights) -- then the prefill and the latent pass once more with a bank of 8 rank-16 adapters (K = D + Kx, Kx = 128)."""
    import test_configs_gpu as cfg
    import test_lora_bank_gpu as lb
    import weights
    sd = weights.gpt_state_dict(2)
    m = lb.make_model(sd, BF16)
    real, sig, seen = nat.gemm_conv, inspect.signature(nat.gemm_conv), []

    def rec(*a, **kw):
        b = sig.bind(*a, **kw)
        b.apply_defaults()
        v = b.arguments
        real(*a, **kw)
        if v["taps"] == 1:
            assert v["B"] == 1 and v["Tin"] == v["Tout"]
            seen.append((nat.last_kernel(), v["Tout"], v["N"], v["Cin"], call_kind(v, v["y"]), max(1, v["ksplit"]), v["dtype"]))

    texts = cfg._texts(2, 20, 60)
    text = cfg._batch(texts).to(DEV)
    lens = torch.tensor([int(t.numel()) for t in texts])
    codes = torch.randint(0, 8192, (32, 80), generator=torch.Generator().manual_seed(5)).to(DEV)
    ids = [i % 9 - 1 for i in range(32)]
    nat.gemm_conv = rec
    try:
        conds = m.get_conditioning(cfg._cond_mel(), None)
        n_cond = len(seen)
        for kw in ({}, dict(adapter_ids=ids)):
            if kw:
                m.attach_lora_bank(lb.make_bank(sd, (16,) * 8, (1.0,) * 8)[0])
            emb, pad = m.prefix_rows(conds, text)
            m.engine.prefill(emb, pad, 8, **kw)
            lat = m(None, text, lens, codes, torch.tensor([80 * 1024] * 32), return_latent=True, conds=conds, **kw)
            assert torch.isfinite(lat).all()
        torch.cuda.synchronize()
        kx = m.engine.bank.Kx
    finally:
        nat.gemm_conv = real
    del m
    return n_cond, kx, seen


def test_production_plain_gemms_are_pinned_and_hold_fp64(nat, production):
    """Every recorded call runs a pinned form with a pinned epilogue kind (run the whole file: the cases fill PINNED), and every
    distinct signature passes the fp64 check of run_case at its own size, on operands of its own seed."""
    if not PINNED:
        pytest.skip("no case ran in this process (the cases of this file fill PINNED: run the whole file)")
    n_cond, kx, seen = production
    assert n_cond >= 1 and len(seen) - n_cond >= 2 * 2 * 2 * 4, (n_cond, len(seen))      # 2 configurations x 2 passes x 2 layers x 4 GEMMs
    assert kx > 0 and {s[3] for s in seen} >= {1280, 5120, 1280 + kx, 5120 + kx}, (kx, sorted({s[3] for s in seen}))
    missing = []
    for s in sorted(set(seen), key=str):
        form, M, N, K, kind, ks, dtype = s
        pinned = form in PINNED and kind in KINDS
        print(f"production | {form} | M={M} N={N} K={K} ksplit={ks} {kind} | {seen.count(s)} calls | {'pinned' if pinned else 'NOT PINNED'}")
        if not pinned:
            missing.append(s)
    assert not missing, f"production calls whose form or epilogue kind no case pins: {missing}"
    for form, M, N, K, kind, ks, dtype in sorted(set(seen), key=str):
        c = R.Case("production", M, N, K, ks=ks, bias="bias" in kind.split("+")[0], act=int("gelu" in kind), y_f32=kind.endswith("->f32"),
                   resid="alias" if "resid=alias" in kind else "own" if "resid=own" in kind else None)
        assert c.kind == kind, (c.kind, kind)
        assert run_case(nat, c, dtype, pin=False) == form
