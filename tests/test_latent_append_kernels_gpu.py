"""The cached-prefix append form of itts_attn_prefill_shared (pre_row0 = NULL; _native.attn_prefill_append): queries behind
the keys / values of a cache row, own rows appended to that row.  Both kernel forms (the 16-query tile and the 64-query tile)
against itts_attn_prefill_packed over the whole sequences, bit for bit; the cache writes byte for byte; chunked appends
against one append; fp32 against the fp64 reference of the other prefill forms (tests/fp32_refs.py, tests/fp64_check.py)."""
import numpy as np
import pytest
import torch

import fp32_refs as R
from fp64_check import ok

pytestmark = pytest.mark.gpu

DEV = "cuda"
H, SMAX, D = 2, 256, 128
PRE, NEW = [0, 63, 64, 130], [70, 1, 16, 17]      # no prefix | a tile edge crossed | one short of / on a 64 boundary | 16 + 1 rows
W_ROW, W_POS0 = [2, 0, 3, 1], [5, 72, 64, 150]    # the prefix sits in front of w_pos0 of another row each: [w_pos0 - pre, w_pos0)
TOT = [a + b for a, b in zip(PRE, NEW)]
OFF_F = np.concatenate([[0], np.cumsum(TOT)])
OFF = np.concatenate([[0], np.cumsum(NEW)])
FORMS = {"attn_append<16>": max(NEW), "attn_append<64>": SMAX}     # the Smax that selects each form (<= 128: the narrow one)


@pytest.fixture(scope="module")
def nat():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from indextts import _native
    _native.lib()
    return _native


def i32(v):
    return torch.tensor(np.asarray(v), dtype=torch.int32, device=DEV)


@pytest.fixture(scope="module")
def whole():
    """the whole sequences' qkv in fp32 (computed once; every dtype rounds it)"""
    return R.prefill_inputs(int(OFF_F[-1]), H, seed=910, device=DEV)


def case(nat, whole, dtype):
    """(qkv of the new rows, the packed form's rows for them, caches with the prefixes in place and 7.0 elsewhere, the caches
    expected after the append)"""
    full = whole.to(dtype)
    out_f = torch.empty(full.shape[0], D, dtype=dtype, device=DEV)
    nat.attn_prefill_packed(full, out_f, None, None, i32(OFF_F), None, len(TOT), max(TOT), H, SMAX)
    kc = torch.full((4, H, SMAX, 64), 7.0, dtype=dtype, device=DEV)
    vc = torch.full((4, H, SMAX, 64), 7.0, dtype=dtype, device=DEV)
    q_rows = []
    for e in range(4):
        blk = full[OFF_F[e]: OFF_F[e + 1]].view(TOT[e], 3, H, 64)
        p0 = W_POS0[e] - PRE[e]
        kc[W_ROW[e], :, p0: W_POS0[e]] = blk[: PRE[e], 1].transpose(0, 1)
        vc[W_ROW[e], :, p0: W_POS0[e]] = blk[: PRE[e], 2].transpose(0, 1)
        q_rows.append(torch.arange(OFF_F[e] + PRE[e], OFF_F[e + 1]))
    want_k, want_v = kc.clone(), vc.clone()
    for e in range(4):
        blk = full[OFF_F[e]: OFF_F[e + 1]].view(TOT[e], 3, H, 64)
        want_k[W_ROW[e], :, W_POS0[e]: W_POS0[e] + NEW[e]] = blk[PRE[e]:, 1].transpose(0, 1)
        want_v[W_ROW[e], :, W_POS0[e]: W_POS0[e] + NEW[e]] = blk[PRE[e]:, 2].transpose(0, 1)
    q_rows = torch.cat(q_rows).to(DEV)
    return full[q_rows].contiguous(), out_f[q_rows], kc, vc, want_k, want_v


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_both_forms_equal_the_packed_form_and_append_the_rows(nat, whole, dtype):
    qkv, want, kc0, vc0, want_k, want_v = case(nat, whole, dtype)
    outs = {}
    for name, smax_arg in FORMS.items():
        kc, vc = kc0.clone(), vc0.clone()
        out = torch.full_like(want, 3.0)
        nat.attn_prefill_append(qkv, out, kc, vc, i32(OFF), i32(PRE), i32(W_ROW), i32(W_POS0), 4, smax_arg, H, SMAX)
        assert nat.last_kernel() == name
        torch.cuda.synchronize()
        assert torch.isfinite(out.float()).all()
        for e in range(4):
            rows = slice(int(OFF[e]), int(OFF[e + 1]))
            assert torch.equal(out[rows], want[rows]), f"{name} {dtype}: element {e} (pre {PRE[e]}, rows {NEW[e]}) differs from the packed form"
        assert torch.equal(kc, want_k) and torch.equal(vc, want_v), f"{name} {dtype}: the caches are not prefix | appended rows | untouched"
        outs[name] = out
    assert torch.equal(*outs.values())
    if dtype == torch.float32:      # and the rows hold the fp64 reference's bound, as the other prefill forms do
        for e in range(4):
            q, k, v = R.split_qkv(whole[OFF_F[e]: OFF_F[e + 1]], H)
            ref, bound, _ = R.prefill_ref(q[PRE[e]:], k, v, PRE[e] + torch.arange(NEW[e], device=DEV), 0)
            ok(f"attn_prefill_append f32 pre={PRE[e]} rows={NEW[e]}", outs["attn_append<16>"][int(OFF[e]): int(OFF[e + 1])], ref, bound)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
def test_chunked_appends_give_the_rows_of_one_append(nat, whole, dtype):
    """70 rows as chunks of 7, 16, 1 and 46 in four calls: every call reads what the earlier ones appended."""
    n = 70
    qkv = whole[:n].to(dtype).contiguous()
    one, kc1, vc1 = torch.empty(n, D, dtype=dtype, device=DEV), *(torch.full((2, H, SMAX, 64), 7.0, dtype=dtype, device=DEV) for _ in range(2))
    nat.attn_prefill_append(qkv, one, kc1, vc1, i32([0, n]), i32([0]), i32([1]), i32([9]), 1, n, H, SMAX)
    got, kc, vc = torch.empty_like(one), torch.full_like(kc1, 7.0), torch.full_like(vc1, 7.0)
    at = 0
    for c in (7, 16, 1, 46):
        part = torch.empty(c, D, dtype=dtype, device=DEV)
        nat.attn_prefill_append(qkv[at: at + c].contiguous(), part, kc, vc, i32([0, c]), i32([at]), i32([1]), i32([9 + at]), 1, c, H, SMAX)
        assert nat.last_kernel() == "attn_append<16>"
        got[at: at + c] = part
        at += c
    assert torch.equal(got, one) and torch.equal(kc, kc1) and torch.equal(vc, vc1)
    if dtype == torch.float32:
        q, k, v = R.split_qkv(whole[:n], H)
        ref, bound, _ = R.prefill_ref(q, k, v, torch.arange(n, device=DEV), 0)
        ok("attn_prefill_append f32 chunked 7|16|1|46", got, ref, bound)


def test_refusals_launch_nothing(nat):
    qkv, out = torch.zeros(4, 3 * D, device=DEV), torch.zeros(4, D, device=DEV)
    kc, vc = torch.full((1, H, 64, 64), 7.0, device=DEV), torch.full((1, H, 64, 64), 7.0, device=DEV)
    args = (i32([0, 4]), i32([0]), i32([0]), i32([0]), 1)
    with pytest.raises(nat.NativeError, match="kv_tab"):
        nat.attn_prefill_append(qkv, out, kc, vc, *args, 4, H, 64, kv_tab=i32([0] * 64), kv_bs=16)
    with pytest.raises(nat.NativeError, match="bad shape"):      # more rows than the cache row holds: the C side's own check
        nat.attn_prefill_append(torch.zeros(80, 3 * D, device=DEV), torch.zeros(80, D, device=DEV), kc, vc, i32([0, 80]), *args[1:], 80, H, 64)
    torch.cuda.synchronize()
    assert (kc == 7.0).all() and (vc == 7.0).all() and (out == 0).all()
