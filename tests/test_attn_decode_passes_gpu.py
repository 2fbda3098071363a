"""Decode attention: the context-sized first key pass against the full pass.

itts_attn_decode requests only the chunks of a key pass that a row's context reaches (2, 4, 6 or 8 per wave; 16-bit types,
no beam row table) instead of always 8 with the dead ones clamped onto the last key.  A dead chunk contributes exactly zero
(score -inf, weight 0), the key-to-lane assignment and each lane's order of operations are unchanged, so the output must be
BIT-EQUAL to the full-pass form.  That form stays reachable in the diagnostic build only (itts_debug_set(7, 1),
include/indextts_hip_diag.h); the product library is what is under test, the diagnostic library's own sized form is held to
the same.  Both are also held to the fp32 torch reference at the tolerance tests/test_kernels_gpu.py::test_attn_decode uses
for 16-bit storage (2e-2).

Cases: bf16 / fp16; contiguous cache and paged cache (block size 16 / 32); with and without kv_share; a skipped row; left
paddings that are not multiples of 8; key slots (context end - first key group) in every arm and on both sides of every arm
boundary: 1, 8, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 300.  One launch shares the cache position among
its rows, so the slot counts are dealt to four launches by their residue mod 8 (the first key group starts at a multiple of 8).
"""
import ctypes
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
SLOTS = [1, 8, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 300]
H, SMAX, C_SHARE = 3, 352, 37
TOL_16BIT = 2e-2   # tests/test_kernels_gpu.py::test_attn_decode


@pytest.fixture(scope="module")
def nat():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from indextts import _native
    _native.lib()
    return _native


@pytest.fixture(scope="module")
def diag(nat):
    path = os.path.join(os.path.dirname(nat.LIB_PATH), "libindextts_hip_diag.so")
    assert os.path.exists(path), f"{path} not found: __graft_entry__.build() makes it (make -C index-tts-lora_amd/csrc diag)"
    L = ctypes.CDLL(path)
    res, args = nat._SIGNATURES["itts_attn_decode"]
    L.itts_attn_decode.restype, L.itts_attn_decode.argtypes = res, args
    L.itts_debug_set.restype, L.itts_debug_set.argtypes = ctypes.c_int, [ctypes.c_int, ctypes.c_int]
    L.itts_last_error.restype = ctypes.c_char_p
    yield L
    L.itts_debug_set(7, 0)


def launches():
    """[(ctx, [(slots, pad)], ...)]: one launch per residue of the slot count mod 8; pad = first key group + d, d varying."""
    out = []
    for r in sorted({n % 8 for n in SLOTS}):
        ctx = 320 + r
        rows = []
        for k, n in enumerate([n for n in SLOTS if n % 8 == r]):
            d = min(n - 1, (3, 5, 0, 7, 1, 6)[k % 6])     # pad < ctx; mostly not a multiple of 8
            rows.append((n, ctx - n + d))
        out.append((ctx, rows))
    return out


def test_cases_cover_every_arm_and_boundary():
    seen = sorted(n for _, rows in launches() for n, _ in rows)
    assert seen == SLOTS
    for ctx, rows in launches():
        for n, pad in rows:
            assert ctx - (pad & ~7) == n and pad < ctx
    assert any(pad % 8 for _, rows in launches() for _, pad in rows)


@pytest.mark.parametrize("share", [False, True])
@pytest.mark.parametrize("bs", [0, 16, 32])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_sized_pass_is_bit_equal_to_the_full_pass(nat, diag, dtype, bs, share):
    for li, (ctx, rows) in enumerate(launches()):
        pads = [p for _, p in rows] + [ctx - 100]          # the last row is skipped
        B = len(pads)
        g = torch.Generator().manual_seed(1000 + li)
        q = torch.randn(B, H * 64, generator=g).to(dtype).to(DEV)
        kc = torch.randn(B, H, SMAX, 64, generator=g).to(dtype).to(DEV)
        vc = torch.randn(B, H, SMAX, 64, generator=g).to(dtype).to(DEV)
        word = None
        if share:                                          # make the promise true: the first C keys of every row are row 0's
            for b in range(1, B):
                n = min(C_SHARE, ctx - pads[b], ctx - pads[0])
                kc[b, :, pads[b]:pads[b] + n] = kc[0, :, pads[0]:pads[0] + n]
                vc[b, :, pads[b]:pads[b] + n] = vc[0, :, pads[0]:pads[0] + n]
            word = torch.tensor([(pads[0] << 8) | min(C_SHARE, ctx - pads[0])], dtype=torch.int32, device=DEV)
        pad = torch.tensor(pads, dtype=torch.int32, device=DEV)
        pos = torch.tensor([ctx - 1], dtype=torch.int32, device=DEV)
        skip = torch.tensor([0] * (B - 1) + [1], dtype=torch.int32, device=DEV)
        kw = dict(skip_rows=skip, kv_share=word)
        kk, vv, smax = kc, vc, SMAX
        if bs:                                             # the same bytes in a block pool behind a shuffled block table
            nb = SMAX // bs
            ids = (torch.randperm(B * nb, generator=g) + 1).view(B, nb)      # block 0: the scratch block of unused entries
            tab = torch.zeros(B, 64, dtype=torch.int32)
            tab[:, :nb] = ids.to(torch.int32)
            kk = torch.zeros(B * nb + 1, H, bs, 64, dtype=dtype, device=DEV)
            vv = torch.zeros_like(kk)
            idx = ids.view(-1).to(DEV)
            kk[idx] = kc.view(B, H, nb, bs, 64).permute(0, 2, 1, 3, 4).reshape(B * nb, H, bs, 64)
            vv[idx] = vc.view(B, H, nb, bs, 64).permute(0, 2, 1, 3, 4).reshape(B * nb, H, bs, 64)
            kw.update(kv_tab=tab.to(DEV), kv_bs=bs)
            smax = 0

        def via_diag(full):
            assert diag.itts_debug_set(7, int(full)) == 0
            o = torch.full((B, H * 64), 7.0, dtype=dtype, device=DEV)
            p = nat._p
            rc = diag.itts_attn_decode(p(q), p(kk), p(vv), p(o), p(pad), p(pos), B, H, smax, nat.dt(dtype), 0, None, None, p(skip),
                                       p(word), p(kw.get("kv_tab")), int(kw.get("kv_bs", 0)), nat._stream())
            assert rc == 0, diag.itts_last_error().decode()
            return o

        o_full = via_diag(True)
        o_sized = via_diag(False)
        o_prod = torch.full((B, H * 64), 7.0, dtype=dtype, device=DEV)
        nat.attn_decode(q, kk, vv, o_prod, pad, pos, B, H, smax, **kw)
        torch.cuda.synchronize()
        what = f"launch {li} (ctx {ctx}, slots {[n for n, _ in rows]})"
        assert torch.equal(o_prod, o_full), f"product library, {what}"
        assert torch.equal(o_sized, o_full), f"diagnostic library, {what}"
        assert (o_prod[B - 1] == 7.0).all()                # the skipped row's slice is not written
        # fp32 reference over the rows' own (contiguous) copies
        sc = (q.float().view(B, H, 1, 64) @ kc.float().transpose(-1, -2)) / 8.0
        j = torch.arange(SMAX, device=DEV)[None, None, None, :]
        vis = (j < ctx) & (j >= pad[:, None, None, None])
        ref = (torch.softmax(sc.masked_fill(~vis, float("-inf")), -1) @ vc.float()).view(B, H * 64)
        for name, o in (("sized", o_prod), ("full", o_full)):
            err = (o.float() - ref)[: B - 1].abs().max().item()
            print(f"{what} {name}: max |err| vs fp32 = {err:.3e}")
            assert err < TOL_16BIT, f"{name} pass, {what}"
