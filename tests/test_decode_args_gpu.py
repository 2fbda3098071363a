"""The decode step's kernels take their arguments in two parts: leading scalars and pointers that the hardware preloads into SGPRs at
wave launch, and a trailing part fetched by a scalar load.  An argument that arrives at the wrong offset shows as a wrong
result at the smallest shape that uses it, so the shapes here are the smallest ones that use every argument:

  * skinny GEMM: M in {1, 17, 32}, alone and as the last chunk of a 96 + M row call (a non-zero row0), a packed y at a y_row0 that is
    not row0, split-K 1 and 3, every epilogue once, the paged K / V append on both sides of a block edge;
  * attn_decode: contexts of 1, 9 and 65 keys and a skipped row, over a contiguous, a paged and a row-table cache;
  * ln_reduce with slabs and the bump words, embed_step with the bump word, sample with a forced stop.

Every case is held to the fp64 helpers of test_decode_kernels_gpu.py (the same bounds), run eagerly, and run as a captured graph that
is replayed twice: each replay must equal the eager run bit for bit (a replayed node reads its own argument buffer; the device words --
position, step, flags -- are read at replay time, so the block-edge case moves the position word between the two replays)."""
import numpy as np
import pytest
import torch

import test_decode_kernels_gpu as dk
from fp64_check import ok, tname, ulp
from skinny_forms import form_key
from test_decode_kernels_gpu import DEV, TAB, decode_case, decode_ref, gemm_pre, i32, ln_ref, paged_pool, rnd

pytestmark = pytest.mark.gpu
BF16, F16 = torch.bfloat16, torch.float16


@pytest.fixture(scope="module")
def nat():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from indextts import _native
    _native.lib()
    return _native


def eager_and_replays(what, make, launch, before=(None, None)):
    """launch(state) eagerly on a fresh make(), then captured on another fresh make() and replayed twice (the state is restored to
    its fresh values in front of each replay; before[i](state) may then move a device word).  Every tensor of the state must come out
    of replay i equal, bit for bit, to the eager run that started from the same words.  Returns the eager states of both rounds."""
    eager = []
    for i in range(2):
        st = make()
        if before[i] is not None:
            before[i](st)
        launch(st)
        eager.append(st)
    fresh, st = make(), make()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        launch(st)
    for i in range(2):
        for t, f in zip(st, fresh):
            t.copy_(f)
        if before[i] is not None:
            before[i](st)
        g.replay()
        torch.cuda.synchronize()
        for j, (a, b) in enumerate(zip(st, eager[i])):
            assert torch.equal(a, b), f"{what}: tensor {j} of replay {i} differs from the eager run"
    return eager


# ------------------------------------------------------------------------------------------------- skinny GEMM
N_, K_ = 192, 96      # one head of q | k | v; three k-steps: one per slice at split-K 3
GEMM_FP64 = [
    # (M, epi, options of run_gemm): every epilogue once, M in {1, 17, 32} and the same as the last chunk behind 96 rows
    (1, "store", {}), (17, "gelu", {}), (32, "silu", {}), (17, "relu_affine", {}), (32, "relu_affine_tanh", {}),
    (1, "store_f32", {}), (17, "resid", dict(ypk=True, y_row0=16)), (32, "slab", dict(ksplit=3)), (17, "qkv", dict(bs=16)),
    (32, "qkv", {}), (17, "store", dict(fold=True, ypk=True, y_row0=32)),
    (97, "store", {}), (113, "slab", dict(ksplit=3)), (128, "resid", {}),
]


@pytest.mark.parametrize("dtype", [BF16, F16], ids=tname)
@pytest.mark.parametrize("case", range(len(GEMM_FP64)), ids=lambda i: "M%d-%s" % GEMM_FP64[i][:2])
def test_skinny_gemm_arguments_fp64(nat, dtype, case):
    M, epi, opt = GEMM_FP64[case]
    K = 128 if opt.get("fold") else K_
    key = form_key(nat, dtype, M, N_, K, opt.get("ksplit", 1), 0, False, opt.get("fold", False))
    dk.run_gemm(nat, dtype, M, N_, K, key, epi=epi, seed=7000 + case, pin=False, **opt)


def gemm_operands(nat, dtype, M, seed):
    x = rnd(M, K_, seed=seed).to(dtype)
    w = (rnd(K_, N_, seed=seed + 1) / K_ ** 0.5).to(dtype)
    bias = rnd(N_, seed=seed + 2).float()
    return x, w, bias, nat.pack_weight(w)


@pytest.mark.parametrize("dtype", [BF16, F16], ids=tname)
def test_skinny_gemm_replays_equal_eager(nat, dtype):
    """Packed y at y_row0 != row0 (M = 17), the residual update with its copy (M = 32), split-K 3 slabs of the second chunk of a
    113-row call (row0 = 96, 17 rows) with the bump word, the fp32 store (M = 1)."""
    for M, seed in ((17, 7100), (32, 7101), (113, 7102), (1, 7103)):
        x, w, bias, wp = gemm_operands(nat, dtype, M, seed)
        xp = nat.pack_activation(x)
        pre, S, _ = gemm_pre(x, w, bias)
        if M == 17:
            ymtp = 4
            make = lambda: [torch.full((ymtp * 16 * N_,), 7.0, dtype=dtype, device=DEV)]  # noqa: E731
            launch = lambda st: nat.gemm_skinny(dtype, M, N_, K_, wp, bias, x=xp, x_packed=True, y=st[0], y_packed=True,  # noqa: E731
                                                y_row0=32, y_mtp=ymtp)
            (y,), _ = eager_and_replays(f"gemm store packed-y M={M}", make, launch)
            full = nat.unpack_activation(y, ymtp * 16, N_)
            ok(f"gemm {tname(dtype)} replay case store M={M}", full[32:32 + M], pre, ulp(pre, dtype) + 2.0 ** -21 * S)
            assert (torch.cat([full[:32], full[32 + M:]]) == 7.0).all()
        elif M == 32:
            h0 = rnd(M, N_, seed=seed + 3, scale=2.0).float()
            make = lambda: [h0.clone(), torch.full((M, N_), 7.0, dtype=dtype, device=DEV)]  # noqa: E731
            launch = lambda st: nat.gemm_skinny(dtype, M, N_, K_, wp, bias, x=x, epi=nat.EPI_RESID_F32, yf=st[0], y=st[1])  # noqa: E731
            (yf, yc), _ = eager_and_replays(f"gemm resid M={M}", make, launch)
            ok(f"gemm {tname(dtype)} replay case resid M={M}", yf, pre + h0.double(), 2.0 ** -21 * (S + h0.double().abs()))
            assert torch.equal(yc, yf.to(dtype))
        elif M == 113:
            make = lambda: [torch.full((3, M, N_), 7.0, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)]  # noqa: E731
            launch = lambda st: nat.gemm_skinny(dtype, M, N_, K_, wp, bias, x=x, epi=nat.EPI_SLAB_F32, yf=st[0], ksplit=3,  # noqa: E731
                                                bump=st[1])
            (slab, word), _ = eager_and_replays(f"gemm slab M={M}", make, launch)
            assert word.item() == 1
            for i in range(3):
                p_i, S_i, _ = gemm_pre(x[:, 32 * i:32 * i + 32], w[32 * i:32 * i + 32], bias if i == 0 else None)
                ok(f"gemm {tname(dtype)} replay case slab {i} M={M}", slab[i], p_i, 2.0 ** -21 * S_i + 1e-300)
        else:
            make = lambda: [torch.full((M, N_), 7.0, device=DEV)]  # noqa: E731
            launch = lambda st: nat.gemm_skinny(dtype, M, N_, K_, wp, bias, x=x, epi=nat.EPI_STORE_F32, yf=st[0])  # noqa: E731
            (yf,), _ = eager_and_replays(f"gemm store_f32 M={M}", make, launch)
            ok(f"gemm {tname(dtype)} replay case store_f32 M={M}", yf, pre, 2.0 ** -21 * S + 1e-300)


@pytest.mark.parametrize("dtype", [BF16, F16], ids=tname)
@pytest.mark.parametrize("M", [1, 17, 32])
def test_qkv_append_across_a_block_edge(nat, dtype, M):
    """The QKV epilogue into a paged cache (blocks of 16) at position 15, the last of a block, and at 16, the first of the next: the
    position word moves between the two replays of one captured launch.  Nothing but that position of the row's own block is written."""
    bs, H = 16, 1
    D = H * 64
    x, w, bias, wp = gemm_operands(nat, dtype, M, 7200 + M)
    tab = np.zeros((M, TAB), dtype=np.int32)
    tab[:, 0:2] = np.random.default_rng(M).permutation(np.arange(1, 1 + 2 * M)).reshape(M, 2)
    tab_d = i32(tab)
    nblk = 1 + 2 * M
    make = lambda: [torch.full((M, D), 7.0, dtype=dtype, device=DEV), torch.full((nblk, H, bs, 64), 7.0, dtype=dtype, device=DEV),  # noqa: E731
                    torch.full((nblk, H, bs, 64), 7.0, dtype=dtype, device=DEV), i32([15])]
    launch = lambda st: nat.gemm_skinny(dtype, M, N_, K_, wp, bias, x=x, epi=nat.EPI_QKV_CACHE, y=st[0], kcache=st[1],  # noqa: E731
                                        vcache=st[2], pos=st[3], heads=H, smax=0, kv_tab=tab_d, kv_bs=bs)
    rounds = eager_and_replays(f"gemm qkv paged M={M}", make, launch, before=(None, lambda st: st[3].fill_(16)))
    pre, S, _ = gemm_pre(x, w, bias)
    for pos, (q, kc, vc, _) in zip((15, 16), rounds):
        blk = torch.from_numpy(tab[:, pos // bs].astype(np.int64)).to(DEV)
        got = torch.cat([q, kc[blk, :, pos % bs].reshape(M, D), vc[blk, :, pos % bs].reshape(M, D)], 1)
        ok(f"gemm {tname(dtype)} qkv paged16 M={M} pos={pos}", got, pre, ulp(pre, dtype) + 2.0 ** -21 * S)
        for cache in (kc, vc):
            t = cache.clone()
            t[blk, :, pos % bs] = 7.0
            assert (t == 7.0).all(), f"M={M} pos={pos}: a cache position other than *pos was written"


# ------------------------------------------------------------------------------------------------- attn_decode
@pytest.mark.parametrize("dtype", [BF16, F16], ids=tname)
@pytest.mark.parametrize("form", ["contiguous", "paged16", "row-table"])
def test_attn_decode_arguments(nat, dtype, form):
    pos, pads, H = 64, [64, 56, 0, 21], 2      # contexts of 1, 9 and 65 keys; the last row is skipped
    B = len(pads)
    q, k, v, smax = decode_case(dtype, pads, pos, H, seed=7300)
    qf = q.reshape(B, H * 64).contiguous()
    posd, padd = i32([pos]), i32(pads)
    skip = i32([0, 0, 0, 1])
    make = lambda: [torch.full((B, H * 64), 7.0, dtype=dtype, device=DEV)]  # noqa: E731
    if form == "paged16":
        pk, pv, tab = paged_pool(k, v, pads, pos, 16, seed=3)
        tab_d = i32(tab)
        launch = lambda st: nat.attn_decode(qf, pk, pv, st[0], padd, posd, B, H, 0, skip_rows=skip, kv_tab=tab_d, kv_bs=16)  # noqa: E731
    elif form == "row-table":
        g = torch.Generator().manual_seed(5)
        t1 = torch.stack([torch.randperm(B, generator=g) for _ in range(smax)], 1).to(DEV)
        kp, vp = torch.zeros_like(k), torch.zeros_like(v)
        jj = torch.arange(smax, device=DEV)[None, :].expand(B, smax)
        kp[t1, :, jj], vp[t1, :, jj] = k.permute(0, 2, 1, 3), v.permute(0, 2, 1, 3)
        tbl = torch.stack([torch.roll(t1, 1, 0), t1]).to(torch.int32).contiguous()
        one = i32([1])
        launch = lambda st: nat.attn_decode(qf, kp, vp, st[0], padd, posd, B, H, smax, skip_rows=skip, kv_rows=tbl, kv_step=one)  # noqa: E731
    else:
        launch = lambda st: nat.attn_decode(qf, k, v, st[0], padd, posd, B, H, smax, skip_rows=skip)  # noqa: E731
    what = f"attn_decode {tname(dtype)} {form} contexts 1 / 9 / 65"
    (out,), _ = eager_and_replays(what, make, launch)
    assert (out[3] == 7.0).all(), f"{what}: the skipped row was written"
    valid = torch.tensor([[True], [True], [True], [False]], device=DEV)
    ref, A = decode_ref(q, k, v, pads, pos)
    ok(what, out, ref, ulp(ref, dtype) + dk.C_ATTN * A, valid)


# ------------------------------------------------------------------------------------------------- ln_reduce, embed_step, sample
@pytest.mark.parametrize("dtype", [BF16, F16], ids=tname)
def test_ln_reduce_slabs_and_bump(nat, dtype):
    M, D, nslab = 13, 1280, 3
    h0 = (rnd(M, D, seed=7400, scale=2.0) + 0.3).float()
    slab = rnd(nslab, M, D, seed=7401, scale=0.5).float()
    bias = (rnd(D, seed=7402) * 0.001).float()
    lw, lb = (1 + 0.1 * rnd(D, seed=7403)).float(), (0.1 * rnd(D, seed=7404)).float()
    make = lambda: [h0.clone(), torch.full((M, D), 7.0, dtype=dtype, device=DEV), i32([4, 9])]  # noqa: E731
    launch = lambda st: nat.ln_reduce(st[0], lw, lb, st[1], slab=slab, nslab=nslab, bias=bias, state_bump=st[2])  # noqa: E731
    (h, out, words), _ = eager_and_replays("ln_reduce slabs", make, launch)
    h_ref = h0 + bias
    for i in range(nslab):
        h_ref = h_ref + slab[i]
    assert torch.equal(h, h_ref), "h is not the fixed-order fp32 sum"
    assert words.tolist() == [5, 10]
    ref, E = ln_ref(h_ref, lw, lb)
    ok(f"ln_reduce {tname(dtype)} M={M} D={D} nslab={nslab} bump", out, ref, ulp(ref, dtype) + E)


@pytest.mark.parametrize("dtype", [BF16, F16], ids=tname)
def test_embed_step_bump(nat, dtype):
    B, D, V, PR, step, pos_add = 17, 1280, 50, 20, 7, 1
    table, ptab = rnd(V, D, seed=7500).float(), rnd(PR, D, seed=7501).float()
    tok = torch.randint(0, V, (B,), generator=torch.Generator().manual_seed(B)).to(torch.int32).to(DEV)
    s0 = [(0, 100, -10000, 3, 8, 7, -12, 9)[i % 8] for i in range(B)]
    s0d, stepd = i32(s0), i32([step])
    mtp = (B + 15) // 16
    make = lambda: [torch.full((B, D), 7.0, device=DEV), torch.full((mtp * 16 * D,), 7.0, dtype=dtype, device=DEV), i32([3])]  # noqa: E731
    launch = lambda st: nat.embed_step(tok, table, ptab, stepd, pos_add, st[0], bump=st[2], row_step0=s0d, h_packed=st[1])  # noqa: E731
    (h, hp, word), _ = eager_and_replays("embed_step", make, launch)
    p = torch.tensor([min(max(step - v + pos_add, 0), PR - 1) for v in s0], device=DEV)
    ref = table[tok.long()] + ptab[p]      # one fp32 addition: the fp64 sum rounded to fp32 is the same value
    assert torch.equal(h, (table[tok.long()].double() + ptab[p].double()).float()) and torch.equal(h, ref)
    assert torch.equal(nat.unpack_activation(hp, B, D), ref.to(dtype))
    assert word.item() == 4


def test_sample_forced_stop(nat):
    """Greedy selection (the fp64 argmax of the logits, which the kernel leaves untouched at penalty 1) for rows 0 and 2, the stop
    token for row 1 (force_stop[1] = 2 <= its step 2) and row 3 (already finished); the history, the finished flags and the loop
    state follow."""
    B, V, cap, stop, step = 4, 8194, 8, 8193, 2
    logits = rnd(B, V, seed=7600).float()
    force = i32([-1, 2, 5, -1])
    make = lambda: [torch.full((B,), -1, dtype=torch.int32, device=DEV), torch.full((B, cap), -1, dtype=torch.int32, device=DEV),  # noqa: E731
                    i32([0, 0, 0, 1]), i32([step, 11, 1, 0, 0, 0, 0, 0])]
    launch = lambda st: nat.sample(logits, st[0], st[1], st[2], st[3], None, force, 1.0, 1.0, 0, 1.0, False, 0, stop)  # noqa: E731
    (tok, hist, fin, state), _ = eager_and_replays("sample", make, launch)
    best = logits.double().argmax(1).to(torch.int32)
    want = torch.stack([best[0], torch.tensor(stop, dtype=torch.int32, device=DEV), best[2],
                        torch.tensor(stop, dtype=torch.int32, device=DEV)])
    assert torch.equal(tok, want)
    assert torch.equal(hist[:, step], want) and (hist[:, :step] == -1).all() and (hist[:, step + 1:] == -1).all()
    assert fin.tolist() == [0, 1, 0, 1]
    assert state.tolist()[:4] == [step + 1, 12, 2, 0]      # step and position advanced once, one more row finished, the counter reset
