"""The float64 references of tests/fp32_refs.py are right, their bounds admit an honest fp32 evaluation and discriminate -- all shown
without a GPU.

Part 1 holds every reference to torch's own float64 operators (F.linear, F.gelu(approximate="tanh"), F.scaled_dot_product_attention
with an explicit mask, F.layer_norm) on the operands the GPU cases use, at 1e-12 relative.  Part 2 lets a plain float32 evaluation of
the same operation stand in for the kernel -- torch CPU fp32 doing the matmul, the softmax over the visible keys and the layer norm --:
it passes `check` under each family's bound, and every negative control fails `must_fail` against it, the very comparison the GPU test
makes.  Part 3 holds the case lists against what they are there for: every fp32 form key, the K / N / M edges, the slot counts and
pads of the decode launches."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fp32_refs as R
from fp64_check import check, must_fail
from skinny_forms import F32_K, F32_M, F32_N, REACHABLE_F32, first_n_with_tiles, form_key

F32 = torch.float32


@pytest.fixture(scope="module")
def nat():
    from indextts import _native
    _native.lib()
    return _native


def close(what, ref, want):
    assert ref.shape == want.shape, what
    if ref.numel() == 0:      # (S = 65 behind 70 padding positions: no row has a key)
        return
    err, lim = (ref - want).abs().max().item(), 1e-12 * max(1.0, want.abs().max().item())
    assert err <= lim, f"{what}: {err:.3e} > {lim:.3e}"


def resolve(nat, case):
    M, N, K, key, opt = case
    if isinstance(N, str):
        N = first_n_with_tiles(nat, F32, int(N[1]))
    return M, N, K, key, opt


# ----------------------------------------------------------------------------------------------------------- skinny GEMM
def test_gemm_cases_reach_every_fp32_form_and_edge(nat):
    cases = [resolve(nat, c) for c in R.GEMM_CASES]
    keys = set()
    for M, N, K, key, opt in cases:
        got = form_key(nat, F32, M, N, K, opt.get("ksplit", 1), 0, opt.get("wide", False), False)
        assert got == key, (M, N, K, opt, got)
        keys.add(got)
    assert keys == REACHABLE_F32, keys ^ REACHABLE_F32
    assert {c[2] for c in cases} >= set(F32_K) and {c[1] for c in cases} >= set(F32_N) and {c[0] for c in cases} >= set(F32_M)
    n2, n3 = first_n_with_tiles(nat, F32, 2), first_n_with_tiles(nat, F32, 3)
    assert nat.skinny_plan(F32, 1, n2 - 1, 16)["tiles_per_wg"] == 1 and nat.skinny_plan(F32, 1, n3 - 1, 16)["tiles_per_wg"] == 2
    assert {c[4]["epi"] for c in cases} == set(R.EPIS)
    for epi in R.EPIS:      # every epilogue runs behind a second and a third row chunk
        assert any(c[4]["epi"] == epi and c[0] > 16 for c in cases), epi
    first = {}
    for c in cases:
        first.setdefault(c[4]["epi"] in ("slab", "qkv") and c[4]["epi"] or "plain", c)
    assert all(c[4].get("controls") for c in first.values()), "the first case of a family carries no control"
    assert R.slices(80, 2) == [(0, 48), (48, 80)] and R.slices(112, 3) == [(0, 48), (48, 96), (96, 112)]


def stand_in_gemm(x, w, bias, epi, h0, ksplit):
    """The operation in plain torch fp32."""
    if epi == "slab":
        return torch.stack([x[:, k0:k1] @ w[k0:k1] + (bias if s == 0 else 0.0) for s, (k0, k1) in enumerate(R.slices(x.shape[1], ksplit))])
    y = x @ w + bias
    if epi == "gelu":
        y = F.gelu(y, approximate="tanh")
    if epi == "resid":
        y = y + h0
    return y


@pytest.mark.parametrize("case", range(len(R.GEMM_CASES)), ids=lambda i: "%d-M%s-N%s-K%s" % ((i,) + R.GEMM_CASES[i][:3]))
def test_gemm_reference_bound_and_controls(nat, case):
    M, N, K, key, opt = resolve(nat, R.GEMM_CASES[case])
    epi, ksplit = opt["epi"], opt.get("ksplit", 1)
    x, w, bias, h0 = R.gemm_operands(M, N, K, seed=100 + 10 * case)
    ref, bound = R.gemm_ref(x, w, bias, epi, resid=h0, ksplit=ksplit)
    xd, wd, bd = x.double(), w.double(), bias.double()
    if epi == "slab":
        want = torch.stack([xd[:, k0:k1] @ wd[k0:k1] + (bd if s == 0 else 0.0) for s, (k0, k1) in enumerate(R.slices(K, ksplit))])
        close("slab sum", ref.sum(0), F.linear(xd, wd.t(), bd))
    else:
        want = F.linear(xd, wd.t(), bd)
        if epi == "gelu":
            want = F.gelu(want, approximate="tanh")
        if epi == "resid":
            want = want + h0.double()
    close(f"gemm {epi} M={M} N={N} K={K}", ref, want)
    y = stand_in_gemm(x, w, bias, epi, h0, ksplit)
    what = f"fp32 stand-in, gemm {epi} M={M} N={N} K={K} ksplit={ksplit}"
    r = check(what, y, ref, bound)
    print(f"fp64 | stand-in | {what} | {r:.3f}")
    if not opt.get("controls"):
        return
    for ctl, text in R.GEMM_CONTROLS.items():
        if ctl == "rows16_shift" and M <= 16:
            continue
        must_fail(what, text, y, R.gemm_ref(x, w, bias, epi, resid=h0, ksplit=ksplit, ctl=ctl)[0], bound)
    if epi == "slab":
        check(what + " summed", y.double().sum(0), ref.sum(0), bound.sum(0))
        must_fail(what + " summed", R.SLAB_MISSING, y.double().sum(0), ref[:-1].sum(0), bound.sum(0))


# ----------------------------------------------------------------------------------------------------------- decode attention
def test_decode_launches_cover_the_slot_counts_and_pads():
    slots, pads = set(), set()
    for pos, ps in R.DECODE_LAUNCHES:
        slots |= {R.decode_slots(pos, p) for p in ps[:-1]}
        pads |= set(ps[:-1])
        assert ps[0] + R.SHARE_C <= pos + 9 and all(p <= pos for p in ps)
    assert slots >= R.DECODE_SLOTS and pads >= R.DECODE_PADS, (R.DECODE_SLOTS - slots, R.DECODE_PADS - pads)
    assert any(R.decode_slots(pos, p) > R.PASS for pos, ps in R.DECODE_LAUNCHES[:1] for p in ps), "the control launch has no second pass"


@pytest.mark.parametrize("launch", range(len(R.DECODE_LAUNCHES)))
def test_decode_reference_bound_and_controls(launch):
    pos, pads = R.DECODE_LAUNCHES[launch]
    H = 2
    q, k, v, smax = R.decode_case(pads, pos, H, seed=500 + launch)
    B = len(pads)
    ref, A = R.decode_ref(q, k, v, pads, pos)
    j = torch.arange(smax)[None, :]
    vis = (j >= torch.tensor(pads)[:, None]) & (j <= pos)
    want = F.scaled_dot_product_attention(q.double()[:, :, None], k.double(), v.double(), attn_mask=vis[:, None, None, :], scale=0.125)
    close(f"decode launch {launch}", ref, want.reshape(B, H * 64))
    s = torch.einsum("bhd,bhjd->bhj", q * 0.125, k).masked_fill(~vis[:, None, :], float("-inf"))
    y = torch.einsum("bhj,bhjd->bhd", torch.softmax(s, -1), v).reshape(B, H * 64)
    bound = R.decode_bound(ref, A)
    what = f"fp32 stand-in, attn_decode pos={pos} pads={pads}"
    r = check(what, y, ref, bound)
    print(f"fp64 | stand-in | {what} | {r:.3f}")
    for text, wrong in R.decode_controls(q, k, v, pads, pos).items():
        fin = torch.isfinite(wrong).all(1, keepdim=True)
        must_fail(what, text, y, torch.nan_to_num(wrong), bound, fin)
    # weight sits on the boundary keys: every marked key of a long row carries at least 1 % of the row's weight
    p = torch.softmax(s.double(), -1)
    b = int(np.argmax([R.decode_slots(pos, p_) for p_ in pads]))
    assert p[b, :, pads[b]].min() > 0.01 and p[b, :, pos].min() > 0.01


# ----------------------------------------------------------------------------------------------------------- prefill attention
@pytest.mark.parametrize("S", [65, 130])
def test_prefill_reference_bound_and_controls(S):
    H = 2
    qkv = R.prefill_inputs(S, H, seed=700 + S)
    q, k, v = R.split_qkv(qkv, H)
    qpos = torch.arange(S)
    j = torch.arange(S)[None, :]
    for pad in (0, 5, 63, 64, 70):
        ref, bound, nvis = R.prefill_ref(q, k, v, qpos, pad)
        vis = (j >= pad) & (j <= qpos[:, None])
        some = nvis > 0
        assert torch.equal(nvis, vis.sum(-1)) and (ref[~some] == 0).all()
        qt, kt, vt = (t.transpose(0, 1) for t in (q, k, v))
        want = F.scaled_dot_product_attention(qt.double()[:, some], kt.double(), vt.double(), attn_mask=vis[some][None], scale=0.125)
        close(f"prefill S={S} pad={pad}", ref[some], want.transpose(0, 1).reshape(-1, H * 64))
        s = (torch.einsum("qhd,jhd->hqj", q * 0.125, k)).masked_fill(~vis[None], float("-inf"))[:, some]
        y = torch.zeros(S, H * 64)
        y[some] = (torch.softmax(s, -1) @ vt).transpose(0, 1).reshape(-1, H * 64)
        what = f"fp32 stand-in, attn_prefill S={S} pad={pad}"
        r = check(what, y, ref, bound)
        print(f"fp64 | stand-in | {what} | {r:.3f}")
        if S == 130 and pad in (5, 70):
            valid = some[:, None]
            must_fail(what, "key i + 1 visible to query i", y, R.prefill_ref(q, k, v, qpos, pad, causal_shift=1)[0], bound, valid)
            must_fail(what, "the key at pad - 1 let in", y, R.prefill_ref(q, k, v, qpos, pad - 1)[0], bound, valid)
            if pad == 5:
                must_fail(what, "the key at position 64 left out", y, R.prefill_ref(q, k, v, qpos, pad, drop=[64])[0], bound, valid)


# ----------------------------------------------------------------------------------------------------------- row kernels
@pytest.mark.parametrize("M", [1, 13])
def test_ln_reference_bound_and_controls(M):
    for ci, (D, nslab, has_bias, lr, two) in enumerate(R.ln_reduce_configs(M, False)):
        o = R.ln_reduce_operands(M, D, nslab, has_bias, lr, two, seed=3000 + 20 * ci + M)
        h = R.slab_sum(o["h0"], o["slab"], list(range(nslab)), D, o["bias"], o["lora_b"])
        if nslab and not lr:      # the fixed-order sum is a sum: within a few ulp of the float64 one
            want = o["h0"].double() + (o["bias"].double() if has_bias else 0.0) + o["slab"][:nslab, :, :D].double().sum(0)
            assert ((h.double() - want).abs() <= 2.0 ** -21 * (want.abs() + 1.0)).all()
        ref, bound = R.ln_pair(h, o["lw"], o["lb"], o["lw2"], o["lb2"])
        want = F.layer_norm(h.double(), (D,), o["lw"].double(), o["lb"].double(), 1e-5)
        y = F.layer_norm(h, (D,), o["lw"], o["lb"], 1e-5)
        if two:
            want = F.layer_norm(want, (D,), o["lw2"].double(), o["lb2"].double(), 1e-5)
            y = F.layer_norm(y, (D,), o["lw2"], o["lb2"], 1e-5)
        close(f"layer norm M={M} D={D} two={two}", ref, want)
        what = f"fp32 stand-in, ln_reduce M={M} D={D} nslab={nslab} r={lr} ln2={two}"
        r = check(what, y, ref, bound)
        print(f"fp64 | stand-in | {what} | {r:.3f}")
        if M != 13:
            continue
        must_fail(what, "statistics over D - 4 columns", y, R.ln_pair(h, o["lw"], o["lb"], o["lw2"], o["lb2"], cols=D - 4)[0], bound)
        must_fail(what, "eps of 1e-6", y, R.ln_pair(h, o["lw"], o["lb"], o["lw2"], o["lb2"], eps=1e-6)[0], bound)
        if nslab:
            h1 = R.slab_sum(o["h0"], o["slab"], list(range(nslab - 1)), D, o["bias"], o["lora_b"])
            must_fail(what, "one slab missing", y, R.ln_pair(h1, o["lw"], o["lb"], o["lw2"], o["lb2"])[0], bound)


def test_kv_share_expected_moves_only_the_ranges():
    c = R.KVS
    cache = torch.arange(c["L"] * 4 * c["H"] * c["smax"] * 64, dtype=torch.float64).view(c["L"], 4, c["H"], c["smax"], 64)
    for C in (1, 5, 32):
        want = R.kv_share_expected(cache, c["B"], C, c["p0"], c["pads"])
        moved = want != cache
        for b in range(4):
            lo = c["pads"][b] if 1 <= b < c["B"] else 0
            n = C if 1 <= b < c["B"] else 0
            assert moved[:, b, :, lo:lo + n].all() and int(moved[:, b].sum()) == c["L"] * c["H"] * n * 64
            if n:
                assert torch.equal(want[:, b, :, lo:lo + n], cache[:, 0, :, c["p0"]:c["p0"] + n])
        assert c["p0"] not in c["pads"] and c["p0"] // c["bs"] != (c["p0"] + 4) // c["bs"]
        assert all(p // c["bs"] != (p + 4) // c["bs"] for p in c["pads"][1:])
