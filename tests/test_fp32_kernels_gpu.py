"""fp64 parity of the fp32 forms of the GPT half -- the sixth pin family, the parity mode's counterpart of test_decode_kernels_gpu.py.

fp32 is the mode every "< 1e-3 against the reference" figure runs in, and its kernels are instantiations of their own: Elem<float> has
E = 4 and KS = 16 (one k-step is four v_mfma_f32_16x16x4_f32; packed weights and activations are 16 columns wide), itts_gemm_skinny
runs MT = 1 and cuts the rows 16 at a time (M = 17 is two launches: x, y, yf, the cache rows, the table rows and the slab rows of the
second chunk come from skinny_params_of), attn_decode_kernel<float> has LPR = 16, RPW = 4 and a 128-key pass that is never
context-sized, attn_prefill_kernel<float> uses the exact-fp32 MFMA and does not round P, kv_share_rows_kernel moves 16 chunks per row.

Every case generates its operands in float64, rounds them to fp32, runs one HIP launch (one entry-point call) on them and compares it
element by element with the float64 references of tests/fp32_refs.py (module docstring there: the bounds and where they come from;
tests/test_fp32_refs_cpu.py holds those references to torch's float64 operators and shows that an honest fp32 evaluation passes and
every control fails).  Outputs are filled with the sentinel 7.0 and what a launch must not write is asserted untouched.  The first
case of every family evaluates the same assertion against a reference that is wrong in one small way; every one must fail.

Skinny GEMM: every case asserts its form key from nat.skinny_plan and adds it to PINNED; test_skinny_every_fp32_form_is_pinned holds
PINNED equal to skinny_forms.REACHABLE_F32.  The production test records the launches of a 2-layer full-width fp32 engine (prefill,
a decode step at batch 1 and 32, a 2 x 3-beam step) and requires every skinny form key and epilogue and every attention form to be a
pinned one.

Every check prints one line `fp64 | kind | case | worst err / bound`; profiles/fp32_kernels_fp64.txt is that output."""
import numpy as np
import pytest
import torch

import fp32_refs as R
from fp64_check import bad, ok
from skinny_forms import REACHABLE_F32, first_n_with_tiles, form_key

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
TAB = R.TAB
PINNED = set()          # form key of every skinny-GEMM case that has run
EPIS_PINNED = set()     # ... and its epilogue
ATTN_PINNED = set()     # decode attention: (template form, packed output, shared first keys); prefill: the entry point's name


@pytest.fixture(scope="module")
def nat():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from indextts import _native
    _native.lib()
    return _native


def i32(v):
    return torch.tensor(np.asarray(v), dtype=torch.int32, device=DEV)


def full(shape, dtype=F32):
    return torch.full(shape, 7.0, dtype=dtype, device=DEV)


# ------------------------------------------------------------------------------------------------- skinny GEMM
def run_gemm(nat, M, N, K, key, epi="store", ksplit=1, wide=False, ypk=False, y_row0=0, copy=True, bs=0, controls=False, seed=0, pin=True):
    """One itts_gemm_skinny call (ceil(M / 16) launches) against the fp64 reference; asserts the form key; packed and row-major x give
    equal bits; the bump word advances once per call."""
    k = form_key(nat, F32, M, N, K, ksplit, 0, wide, False)
    assert k == key, f"M={M} N={N} K={K} ksplit={ksplit} wide={wide}: planned {k}, case built for {key}"
    if pin:
        PINNED.add(k)
        EPIS_PINNED.add(epi)
    what = f"gemm f32 {k} M={M} N={N} K={K} {epi}" + (f" ksplit={ksplit}" if ksplit > 1 else "") + (" wide" if wide else "") + \
        (f" packed-y row0={y_row0}" if ypk else "") + (f" paged{bs}" if bs else "")
    x, w, bias, h0 = R.gemm_operands(M, N, K, seed, DEV)
    wp, xp = nat.pack_weight(w), nat.pack_activation(x)
    mtp = (M + 15) // 16
    ymtp = mtp + y_row0 // 16 + (1 if y_row0 else 0)
    code = dict(store=nat.EPI_STORE, gelu=nat.EPI_GELU_STORE, qkv=nat.EPI_QKV_CACHE, resid=nat.EPI_RESID_F32, slab=nat.EPI_SLAB_F32,
                store_f32=nat.EPI_STORE_F32)[epi]

    def both(make_out, names, **kw):
        """Run with the row-major and the packed operand into fresh outputs; equal bits; one bump each; returns the first's outputs."""
        o1, o2 = make_out(), make_out()
        for xa, packed, outs in ((x, False, o1), (xp, True, o2)):
            word = torch.zeros(1, dtype=torch.int32, device=DEV)
            nat.gemm_skinny(F32, M, N, K, wp, bias, x=xa, x_packed=packed, epi=code, ksplit=ksplit, wide_wg=wide, bump=word,
                            **dict(zip(names, outs)), **kw)
            assert word.item() == 1, f"{what}: the bump word was advanced {word.item()} times by one call"
        for a, b in zip(o1, o2):
            assert torch.equal(a, b), f"{what}: packed and row-major x differ"
        return o1

    def unpacked(y):
        """Rows [y_row0, y_row0 + M) of a packed y; every other row of the operand still holds the sentinel."""
        t = nat.unpack_activation(y, ymtp * 16, N)
        assert (torch.cat([t[:y_row0], t[y_row0 + M:]]) == 7.0).all(), f"{what}: rows of the packed operand outside [y_row0, y_row0 + M) were written"
        return t[y_row0:y_row0 + M]
    pk = dict(y_packed=True, y_row0=y_row0, y_mtp=ymtp) if ypk else {}
    tab = None
    if epi in ("store", "gelu"):
        (y,) = both(lambda: (full((ymtp * 16 * N,) if ypk else (M, N)),), ("y",), **pk)
        got = unpacked(y) if ypk else y
    elif epi == "store_f32":
        (got,) = both(lambda: (full((M, N)),), ("yf",))
    elif epi == "resid":      # resid aliases yf: the stream is updated in place
        if copy:
            yf, yc = both(lambda: (h0.clone(), full((ymtp * 16 * N,) if ypk else (M, N))), ("yf", "y"), **pk)
            assert torch.equal(unpacked(yc) if ypk else yc, yf), f"{what}: the T copy is not the new fp32 row"
        else:
            (yf,) = both(lambda: (h0.clone(),), ("yf",))
        got = yf
    elif epi == "slab":
        (got,) = both(lambda: (full((ksplit, M, N)),), ("yf",))
    else:
        H = N // 192
        D, pos = H * 64, 37
        if bs:
            e = (pos // bs) % TAB
            tab = np.zeros((M, TAB), dtype=np.int32)      # unmapped entries name the scratch block 0
            blocks = np.random.default_rng(seed).permutation(np.arange(1, 1 + 3 * M)).reshape(M, 3)
            for j in range(3):
                tab[:, (e - 1 + j) % TAB] = blocks[:, j]
            mk = lambda: (full((M, D)), full((1 + 3 * M, H, bs, 64)), full((1 + 3 * M, H, bs, 64)))  # noqa: E731
            kw = dict(pos=i32([pos]), heads=H, smax=0, kv_tab=i32(tab), kv_bs=bs)
        else:
            smax = 48
            mk = lambda: (full((M, D)), full((M, H, smax, 64)), full((M, H, smax, 64)))  # noqa: E731
            kw = dict(pos=i32([pos]), heads=H, smax=smax)
        q, kc, vc = both(mk, ("y", "kcache", "vcache"), **kw)

        def appended(cache, entry_off=0):
            if bs:
                blk = torch.from_numpy(tab[:, (e + entry_off) % TAB].astype(np.int64)).to(DEV)
                return cache[blk, :, pos % bs].reshape(M, D)
            return cache[:, :, pos].reshape(M, D)
        for cache in (kc, vc):                            # nothing but position *pos of each row's own cache row / block was touched
            t = cache.clone()
            if bs:
                t[torch.from_numpy(tab[:, e].astype(np.int64)).to(DEV), :, pos % bs] = 7.0
            else:
                t[:, :, pos] = 7.0
            assert (t == 7.0).all(), f"{what}: a cache position other than *pos of the row's own block was written"
        got = torch.cat([q, appended(kc), appended(vc)], 1)
    ref, bound = R.gemm_ref(x, w, bias, epi, resid=h0, ksplit=ksplit)
    ok(what, got, ref, bound)
    if M > 16:      # the chunks behind the first on their own: the worst row of chunk 0 must not hide them
        ok(what + " rows 16..", got[..., 16:, :], ref[..., 16:, :], bound[..., 16:, :])
    if epi == "qkv":      # the same form storing row-major fp32 adds in the same order: q and the appended k / v rows equal it bit for bit
        plain = full((M, N))
        nat.gemm_skinny(F32, M, N, K, wp, bias, x=x, epi=nat.EPI_STORE_F32, yf=plain, wide_wg=wide)
        assert torch.equal(got, plain), f"{what}: q | appended k | appended v differ from the STORE_F32 rows of the same GEMM"
    if epi == "slab":
        ok(what + " summed", got.double().sum(0), ref.sum(0), bound.sum(0))
    if not controls:
        return
    for ctl, text in R.GEMM_CONTROLS.items():
        if ctl == "rows16_shift" and M <= 16:
            continue
        bad(what, text, got, R.gemm_ref(x, w, bias, epi, resid=h0, ksplit=ksplit, ctl=ctl)[0], bound)
    if epi == "slab":
        bad(what + " summed", R.SLAB_MISSING, got.double().sum(0), ref[:-1].sum(0), bound.sum(0))
    if tab is not None:
        bad(what, "the append placed one block entry off", torch.cat([q, appended(kc, 1), appended(vc, 1)], 1), ref, bound)


def resolve(nat, case):
    M, N, K, key, opt = case
    if isinstance(N, str):
        N = first_n_with_tiles(nat, F32, int(N[1]))
    return M, N, K, key, opt


@pytest.mark.parametrize("case", range(len(R.GEMM_CASES)), ids=lambda i: "%d-M%s-N%s-K%s" % ((i,) + R.GEMM_CASES[i][:3]))
def test_skinny_gemm_fp32_fp64(nat, case):
    """One fp32 form at one edge of the K walk, the column tiling or the row chunking against the fp64 reference (fp32_refs.GEMM_CASES)."""
    M, N, K, key, opt = resolve(nat, R.GEMM_CASES[case])
    run_gemm(nat, M, N, K, key, seed=100 + 10 * case, **opt)


def test_skinny_every_fp32_form_is_pinned(nat):
    """Every fp32 instantiation plan_skinny can ask launch_skinny_mt for has a case above (run the whole file: the cases fill PINNED),
    no case pins a form the enumeration does not know, and every epilogue ran."""
    if not PINNED:
        pytest.skip("no skinny-GEMM case ran in this process (the cases of this file fill PINNED: run the whole file)")
    assert PINNED == REACHABLE_F32, (sorted(PINNED - REACHABLE_F32), sorted(REACHABLE_F32 - PINNED))
    assert EPIS_PINNED == set(R.EPIS)


# ------------------------------------------------------------------------------------------------- decode attention
@pytest.mark.parametrize("form", R.DECODE_FORMS)
@pytest.mark.parametrize("launch", range(len(R.DECODE_LAUNCHES)))
def test_attn_decode_fp32_fp64(nat, form, launch):
    """Every template form of attn_decode_kernel<float> with rows whose key-slot counts sit at the edges of the 128-key pass
    (fp32_refs.DECODE_LAUNCHES); the last row is skipped and keeps its sentinel.  Negative controls on launch 0 (a second, third and
    fourth pass exist there) for every form."""
    pos, pads = R.DECODE_LAUNCHES[launch]
    H = 3 if form == "contiguous" else 2
    B = len(pads)
    skip_row = B - 1
    shared = form.endswith("share")
    q, k, v, smax = R.decode_case(pads, pos, H, seed=500 + launch, device=DEV, same_q=shared)
    C, p0 = 0, 0
    share = None

    def shared_n(b):
        return max(0, min(C, pos + 1 - pads[b]))
    if shared:          # the first C keys of every row are row 0's positions [p0, p0 + C)
        C, p0 = R.SHARE_C, pads[0]
        for b in range(1, B):
            n = shared_n(b)
            k[b, :, pads[b]:pads[b] + n] = k[0, :, p0:p0 + n]
            v[b, :, pads[b]:pads[b] + n] = v[0, :, p0:p0 + n]
        share = i32([(p0 << 8) | C])
    posd, padd = i32([pos]), i32(pads)
    skip = torch.zeros(B, dtype=torch.int32, device=DEV)
    skip[skip_row] = 1
    packed = "packed-out" in form
    out = full(((B + 15) // 16 * 16 * H * 64,) if packed else (B, H * 64))
    qf = q.reshape(B, H * 64).contiguous()
    kc, vc = k, v
    if C:       # the rows' own copies of the shared keys hold garbage: they must be read from row 0
        kc, vc = k.clone(), v.clone()
        for b in range(1, B):
            kc[b, :, pads[b]:pads[b] + shared_n(b)] = 3.0
            vc[b, :, pads[b]:pads[b] + shared_n(b)] = 3.0
    tab = bs = None
    if form.startswith("paged"):
        bs = int(form[5:7])
        pk, pv, tab = R.paged_pool(kc, vc, bs, seed=launch)
        nat.attn_decode(qf, pk, pv, out, padd, posd, B, H, 0, out_packed=packed, skip_rows=skip, kv_share=share, kv_tab=i32(tab), kv_bs=bs)
        ATTN_PINNED.add((f"paged{bs}", packed, shared))
    elif form.startswith("row-table"):  # position j of logical row b lives in physical row table[parity][b][j]
        g = torch.Generator().manual_seed(launch)
        t1 = torch.stack([torch.randperm(B, generator=g) for _ in range(smax)], 1).to(DEV)      # [B][smax], a permutation per position
        kp, vp = torch.zeros_like(k), torch.zeros_like(v)
        jj = torch.arange(smax, device=DEV)[None, :].expand(B, smax)
        kp[t1, :, jj], vp[t1, :, jj] = k.permute(0, 2, 1, 3), v.permute(0, 2, 1, 3)
        t0 = torch.roll(t1, 1, 0)                                                                 # the other parity: another row's table
        tbl = torch.stack([t0, t1]).to(torch.int32).contiguous()
        nat.attn_decode(qf, kp, vp, out, padd, posd, B, H, smax, out_packed=packed, skip_rows=skip, kv_rows=tbl, kv_step=i32([1]))
        ATTN_PINNED.add(("row-table", packed, False))
    else:
        nat.attn_decode(qf, kc, vc, out, padd, posd, B, H, smax, out_packed=packed, skip_rows=skip, kv_share=share)
        ATTN_PINNED.add(("contiguous", packed, shared))
    got = nat.unpack_activation(out, B, H * 64) if packed else out
    what = f"attn_decode f32 {form} pos={pos} pads={pads}"
    assert (got[skip_row] == 7.0).all(), f"{what}: the skipped row was written"
    if packed:
        assert (nat.unpack_activation(out, (B + 15) // 16 * 16, H * 64)[B:] == 7.0).all(), f"{what}: padding rows of the packed output were written"
    valid = torch.ones(B, 1, dtype=torch.bool, device=DEV)
    valid[skip_row] = False
    ref, A = R.decode_ref(q, k, v, pads, pos)
    bound = R.decode_bound(ref, A)
    ok(what, got, ref, bound, valid)
    if launch != 0:
        return

    def dbad(control, r):      # a control that leaves a row without any key says nothing about that row
        fin = torch.isfinite(r).all(1, keepdim=True)
        bad(what, control, got, torch.nan_to_num(r), bound, valid & fin)
    for text, wrong in R.decode_controls(q, k, v, pads, pos).items():
        dbad(text, wrong)
    if C:
        k2, v2 = k.clone(), v.clone()
        for b in range(1, B):
            n = shared_n(b)
            k2[b, :, pads[b]:pads[b] + n] = k[0, :, p0 + 1:p0 + 1 + n]
            v2[b, :, pads[b]:pads[b] + n] = v[0, :, p0 + 1:p0 + 1 + n]
        dbad("the shared keys taken from p0 + 1", R.decode_ref(q, k2, v2, pads, pos)[0])
    if form.startswith("row-table"):
        idx = t0[:, None, :, None].expand(B, H, smax, 64)
        dbad("the table of the other parity", R.decode_ref(q, torch.gather(kp, 0, idx), torch.gather(vp, 0, idx), pads, pos)[0])
    if tab is not None and not C:
        t2 = np.roll(tab, 1, axis=0)
        dbad("the neighbour's block table used", R.decode_ref(q, R.unpage(pk, t2, smax, bs), R.unpage(pv, t2, smax, bs), pads, pos)[0])


# ------------------------------------------------------------------------------------------------- prefill attention
def prefill_check(what, out, q, k, v, qpos, lo):
    ref, bound, nvis = R.prefill_ref(q, k, v, qpos, lo)
    ok(what, out, ref, bound)
    return bound, nvis


@pytest.mark.parametrize("S", [65, 130])
def test_attn_prefill_left_padded_fp32_fp64(nat, S):
    """itts_attn_prefill: pads 0, 5, 63, 64, 70 in one launch (a tile wholly inside the padding, a tile straddling it, rows with no
    visible key: exact zeros).  Cache: positions [64 floor(pad / 64), S) hold the k / v thirds bit for bit, the rest its sentinel."""
    H, smax = 2, 136
    pads = [0, 5, 63, 64, 70]
    B, D = len(pads), 128
    qkv = R.prefill_inputs(B * S, H, seed=700 + S, device=DEV).view(B, S, 3 * D)
    out, kc, vc = full((B, S, D)), full((B, H, smax, 64)), full((B, H, smax, 64))
    nat.attn_prefill(qkv, out, kc, vc, i32(pads), B, S, H, smax)
    ATTN_PINNED.add("attn_prefill")
    qpos = torch.arange(S, device=DEV)
    for b, pad in enumerate(pads):
        q, k, v = R.split_qkv(qkv[b], H)
        what = f"attn_prefill f32 S={S} pad={pad}"
        bound, nvis = prefill_check(what, out[b], q, k, v, qpos, pad)
        assert (out[b][nvis == 0] == 0).all(), f"{what}: a row without a visible key is not exact zeros"
        first = min((pad // 64) * 64, S)
        for cache, src in ((kc, k), (vc, v)):
            assert torch.equal(cache[b, :, first:S], src[first:S].transpose(0, 1)), f"{what}: cache rows differ from the k / v thirds"
            assert (cache[b, :, :first] == 7.0).all() and (cache[b, :, S:] == 7.0).all(), f"{what}: a cache position outside the rows was written"
        if S == 130 and pad in (5, 70):
            valid = (nvis > 0)[:, None]
            bad(what, "key i + 1 visible to query i", out[b], R.prefill_ref(q, k, v, qpos, pad, causal_shift=1)[0], bound, valid)
            bad(what, "the key at pad - 1 let in", out[b], R.prefill_ref(q, k, v, qpos, pad - 1)[0], bound, valid)
            if pad == 5:
                bad(what, "the key at position 64 left out", out[b], R.prefill_ref(q, k, v, qpos, pad, drop=[64])[0], bound, valid)


@pytest.mark.parametrize("paged", [0, 16])
def test_attn_prefill_packed_fp32_fp64(nat, paged):
    """itts_attn_prefill_packed: elements of 1, 64 and 65 rows in one launch, cache row of local row i = cache_shift[b] + i."""
    H, smax = 2, 96
    lens, shift = [1, 64, 65], [7, 0, 19]
    B, D = len(lens), 128
    off = np.concatenate([[0], np.cumsum(lens)])
    qkv = R.prefill_inputs(int(off[-1]), H, seed=720, device=DEV)
    out = full((int(off[-1]), D))
    if paged:
        nb = smax // paged
        tab = np.zeros((B, TAB), dtype=np.int32)
        tab[:, :nb] = np.random.default_rng(1).permutation(np.arange(1, 1 + B * nb)).reshape(B, nb)
        kc, vc = full((1 + B * nb, H, paged, 64)), full((1 + B * nb, H, paged, 64))
        nat.attn_prefill_packed(qkv, out, kc, vc, i32(off), i32(shift), B, max(lens), H, 0, kv_tab=i32(tab), kv_bs=paged)
        kl, vl = R.unpage(kc, tab, smax, paged), R.unpage(vc, tab, smax, paged)
        assert (kc[0] == 7.0).all() and (vc[0] == 7.0).all()
    else:
        kc, vc = full((B, H, smax, 64)), full((B, H, smax, 64))
        nat.attn_prefill_packed(qkv, out, kc, vc, i32(off), i32(shift), B, max(lens), H, smax)
        kl, vl = kc, vc
    ATTN_PINNED.add("attn_prefill_packed")
    for b, n in enumerate(lens):
        rows = slice(int(off[b]), int(off[b + 1]))
        q, k, v = R.split_qkv(qkv[rows], H)
        what = f"attn_prefill_packed f32 paged={paged} len={n}"
        qpos = torch.arange(n, device=DEV)
        bound, _ = prefill_check(what, out[rows], q, k, v, qpos, 0)
        for cache, src in ((kl, k), (vl, v)):
            assert torch.equal(cache[b, :, shift[b]:shift[b] + n], src.transpose(0, 1)), f"{what}: cache rows differ from the k / v thirds"
            assert (cache[b, :, :shift[b]] == 7.0).all() and (cache[b, :, shift[b] + n:] == 7.0).all(), f"{what}: stray cache write"
        if n == 65:
            bad(what, "key i + 1 visible to query i", out[rows], R.prefill_ref(q, k, v, qpos, 0, causal_shift=1)[0], bound)
            bad(what, "the key at position 64 left out", out[rows], R.prefill_ref(q, k, v, qpos, 0, drop=[64])[0], bound)


@pytest.mark.parametrize("paged", [0, 32])
def test_attn_prefill_prefix_fp32_fp64(nat, paged):
    """itts_attn_prefill_prefix: prefix lengths 0, 1, 63, 64, 100 read from cache rows (permuted, at an offset), contiguous and paged;
    the caches are read only."""
    H, smax = 2, 128
    pre, mq = [0, 1, 63, 64, 100], [5, 64, 65, 1, 70]
    crow, pos0 = [3, 0, 4, 1, 2], [9, 0, 11, 3, 20]
    B, D = len(pre), 128
    off = np.concatenate([[0], np.cumsum(mq)])
    qkv = R.prefill_inputs(int(off[-1]), H, seed=740, device=DEV)
    ck = R.rnd(B, H, smax, 64, seed=741, device=DEV).float()
    cv = R.rnd(B, H, smax, 64, seed=742, device=DEV).float()
    out = full((int(off[-1]), D))
    if paged:
        pk, pv, tab = R.paged_pool(ck, cv, paged, seed=2)
        pk0, pv0 = pk.clone(), pv.clone()
        nat.attn_prefill_prefix(qkv, out, pk, pv, i32(off), i32(pre), i32(crow), i32(pos0), B, max(mq), H, 0, kv_tab=i32(tab), kv_bs=paged)
        assert torch.equal(pk, pk0) and torch.equal(pv, pv0)
    else:
        ck0, cv0 = ck.clone(), cv.clone()
        nat.attn_prefill_prefix(qkv, out, ck, cv, i32(off), i32(pre), i32(crow), i32(pos0), B, max(mq), H, smax)
        assert torch.equal(ck, ck0) and torch.equal(cv, cv0)
    ATTN_PINNED.add("attn_prefill_prefix")
    for b in range(B):
        rows = slice(int(off[b]), int(off[b + 1]))
        q, k, v = R.split_qkv(qkv[rows], H)
        what = f"attn_prefill_prefix f32 paged={paged} pre={pre[b]} rows={mq[b]}"

        def seq(p_from, n=pre[b], b=b, k=k, v=v):
            kp = ck[crow[b], :, p_from:p_from + n].transpose(0, 1)
            vp = cv[crow[b], :, p_from:p_from + n].transpose(0, 1)
            return torch.cat([kp, k]), torch.cat([vp, v])
        kk, vv = seq(pos0[b])
        qpos = pre[b] + torch.arange(mq[b], device=DEV)
        bound, _ = prefill_check(what, out[rows], q, kk, vv, qpos, 0)
        if pre[b] in (1, 100):
            bad(what, "prefix key pre_len - 1 left out", out[rows], R.prefill_ref(q, kk, vv, qpos, 0, drop=[pre[b] - 1])[0], bound)
            k1, v1 = seq(pos0[b] + 1)
            bad(what, "the prefix read from pre_pos0 + 1", out[rows], R.prefill_ref(q, k1, v1, qpos, 0)[0], bound)


def test_attn_prefill_shared_fp32_fp64(nat):
    """itts_attn_prefill_shared: element 0 is the shared block (prefix length 0), elements 1-3 sit behind prefixes that are rows of qkv
    itself (lengths 63, 64 and 30 -- element 3 behind a different slice of the block); own rows appended to the caches."""
    H, smax = 2, 160
    lens = [70, 1, 65, 64]
    pre, pre_row0 = [0, 63, 64, 30], [0, 0, 0, 5]
    w_row, w_pos0 = [0, 1, 2, 3], [3, 70, 64, 40]
    E, D = len(lens), 128
    off = np.concatenate([[0], np.cumsum(lens)])
    qkv = R.prefill_inputs(int(off[-1]), H, seed=760, device=DEV)
    out, kc, vc = full((int(off[-1]), D)), full((E, H, smax, 64)), full((E, H, smax, 64))
    nat.attn_prefill_shared(qkv, out, kc, vc, i32(off), i32(pre), i32(pre_row0), i32(w_row), i32(w_pos0), E, max(lens), H, smax)
    ATTN_PINNED.add("attn_prefill_shared")
    qa, ka, va = R.split_qkv(qkv, H)
    for e in range(E):
        rows = slice(int(off[e]), int(off[e + 1]))
        what = f"attn_prefill_shared f32 element {e} pre={pre[e]} rows={lens[e]}"

        def seq(r0, e=e, rows=rows):
            return torch.cat([ka[r0:r0 + pre[e]], ka[rows]]), torch.cat([va[r0:r0 + pre[e]], va[rows]])
        kk, vv = seq(pre_row0[e])
        qpos = pre[e] + torch.arange(lens[e], device=DEV)
        bound, _ = prefill_check(what, out[rows], qa[rows], kk, vv, qpos, 0)
        for cache, src in ((kc, ka), (vc, va)):
            assert torch.equal(cache[w_row[e], :, w_pos0[e]:w_pos0[e] + lens[e]], src[rows].transpose(0, 1)), f"{what}: appended rows differ"
            assert (cache[w_row[e], :, :w_pos0[e]] == 7.0).all() and (cache[w_row[e], :, w_pos0[e] + lens[e]:] == 7.0).all(), f"{what}: stray write"
        if e == 2:
            k3, v3 = seq(pre_row0[3])
            bad(what, "pre_row0 of element 3 given to element 2", out[rows], R.prefill_ref(qa[rows], k3, v3, qpos, 0)[0], bound)
            bad(what, "prefix key pre_len - 1 left out", out[rows], R.prefill_ref(qa[rows], kk, vv, qpos, 0, drop=[pre[e] - 1])[0], bound)


# ------------------------------------------------------------------------------------------------- row kernels
@pytest.mark.parametrize("ypk", [False, True], ids=["rowmajor", "packed"])
@pytest.mark.parametrize("M", [1, 13, 32, 96])
def test_ln_reduce_fp32_fp64(nat, M, ypk):
    """itts_ln_reduce into an fp32 output, the configurations of the 16-bit test (fp32_refs.ln_reduce_configs).  h after the slab sum is
    the fixed-order fp32 sum bit for bit; the output is held to ln_ref's budget plus ulp_f32.  Controls on M = 13."""
    for ci, (D, nslab, has_bias, lr, two) in enumerate(R.ln_reduce_configs(M, ypk)):
        o = R.ln_reduce_operands(M, D, nslab, has_bias, lr, two, seed=3000 + 20 * ci + M, device=DEV)
        stride, slab = o["stride"], o["slab"]
        h = o["h0"].clone()
        out = full((nat.packed_rows(M) * D,) if ypk else (M, D))
        nat.ln_reduce(h, o["lw"], o["lb"], out, slab=slab if nslab else None, nslab=nslab, bias=o["bias"], w2=o["lw2"], b2=o["lb2"],
                      y_packed=ypk, slab_stride=stride if stride != D else 0, lora_b=o["lora_b"])
        got = nat.unpack_activation(out, M, D) if ypk else out
        what = f"ln_reduce f32 M={M} D={D} nslab={nslab} bias={has_bias} r={lr} ln2={two} stride={stride} packed={ypk}"
        if ypk:
            assert (nat.unpack_activation(out, nat.packed_rows(M), D)[M:] == 7.0).all(), f"{what}: padding rows of the packed output were written"
        h_of = lambda slabs, lb_=o["lora_b"]: R.slab_sum(o["h0"], slab, slabs, D, o["bias"], lb_)  # noqa: E731
        h_ref = h_of(list(range(nslab)))
        assert torch.equal(h, h_ref), f"{what}: h is not the fixed-order fp32 sum"
        y_of = lambda hh, **kw: R.ln_pair(hh, o["lw"], o["lb"], o["lw2"], o["lb2"], **kw)  # noqa: E731
        ref, bound = y_of(h_ref)
        ok(what, got, ref, bound)
        if M != 13:
            continue
        bad(what, "statistics over D - 4 columns", got, y_of(h_ref, cols=D - 4)[0], bound)
        bad(what, "eps of 1e-6", got, y_of(h_ref, eps=1e-6)[0], bound)
        if nslab:
            bad(what, "one slab missing", got, y_of(h_of(list(range(nslab - 1))))[0], bound)
        if lr:
            sw = o["lora_b"].clone()
            sw[[lr - 2, lr - 1]] = o["lora_b"][[lr - 1, lr - 2]]
            bad(what, "the last two rows of lora_b exchanged", got, y_of(h_of(list(range(nslab)), sw))[0], bound)


@pytest.mark.parametrize("M", [1, 13, 32, 96])
def test_layernorm_fp32_fp64(nat, M):
    """itts_layernorm into an fp32 output, with and without the second pair, D = 1280 and D = 320."""
    for D in (1280, 320):
        for two in (False, True):
            seed = 3500 + M + D
            h = (R.rnd(M, D, seed=seed, scale=2.0, device=DEV) + 0.3).float()
            h[0] = (R.rnd(D, seed=seed + 1, device=DEV) * 0.01 + 0.5).float()
            lw, lb = (1 + 0.1 * R.rnd(D, seed=seed + 4, device=DEV)).float(), (0.1 * R.rnd(D, seed=seed + 5, device=DEV)).float()
            lw2, lb2 = ((1 + 0.1 * R.rnd(D, seed=seed + 6, device=DEV)).float(), (0.1 * R.rnd(D, seed=seed + 7, device=DEV)).float()) if two else (None, None)
            out = full((M, D))
            nat.layernorm(h, lw, lb, out, w2=lw2, b2=lb2)
            ref, bound = R.ln_pair(h, lw, lb, lw2, lb2)
            what = f"layernorm f32 M={M} D={D} ln2={two}"
            ok(what, out, ref, bound)
            if M == 13:
                bad(what, "statistics over D - 4 columns", out, R.ln_pair(h, lw, lb, lw2, lb2, cols=D - 4)[0], bound)
                bad(what, "eps of 1e-6", out, R.ln_pair(h, lw, lb, lw2, lb2, eps=1e-6)[0], bound)


@pytest.mark.parametrize("B", [1, 13, 32, 96])
def test_embed_step_fp32_exact(nat, B):
    """itts_embed_step with an fp32 packed copy: h = table[token] + pos_table[p] is one fp32 addition (bit-exact), the packed copy holds
    the same bits, p = clamp(*step - row_step0[b] + pos_add, 0, rows - 1) is clamped at both ends, the word is bumped once."""
    D, V, PR, step, pos_add = 1280, 50, 20, 7, 1
    table, ptab = R.rnd(V, D, seed=3700, device=DEV).float(), R.rnd(PR, D, seed=3701, device=DEV).float()
    g = torch.Generator().manual_seed(B)
    tok = torch.randint(0, V, (B,), generator=g).to(torch.int32).to(DEV)
    s0 = [(0, 100, -10000, 3, 8, 7, -12, 9)[i % 8] for i in range(B)]          # p = 8, < 0, >= rows, 5, 0, 1, 20 -> 19, -1 -> 0
    mtp = (B + 15) // 16
    h, hp = full((B, D)), full((mtp * 16 * D,))
    word = torch.zeros(1, dtype=torch.int32, device=DEV)
    nat.embed_step(tok, table, ptab, i32([step]), pos_add, h, bump=word, row_step0=i32(s0), h_packed=hp)
    p = torch.tensor([min(max(step - v + pos_add, 0), PR - 1) for v in s0], device=DEV)
    ref = table[tok.long()] + ptab[p]
    assert torch.equal(h, ref), "h is not table[token] + pos_table[p]"
    assert torch.equal(nat.unpack_activation(hp, B, D), ref), "the packed fp32 copy is not the fp32 row"
    assert (nat.unpack_activation(hp, mtp * 16, D)[B:] == 7.0).all(), "padding rows of the packed copy were written"
    assert word.item() == 1
    if B == 13:
        assert not torch.equal(h, table[tok.long()] + ptab[torch.clamp(p + 1, max=PR - 1)])


@pytest.mark.parametrize("dtype", [BF16, F16, F32], ids=["bf16", "f16", "f32"])
@pytest.mark.parametrize("form", ["contiguous", "contiguous-spare-rows", "paged16"])
@pytest.mark.parametrize("C", [1, 5, 32])
def test_kv_share_rows(nat, dtype, form, C):
    """itts_kv_share_rows: rows 1 .. B - 1 receive row 0's positions [p0, p0 + C) at [pad_b, pad_b + C), for K and V and in every
    layer, compared with ==; row 0 and every byte outside the ranges hold what they held; B = 1 writes nothing.
    contiguous-spare-rows: caches with more rows than B, so the layer stride is larger than B H smax 64 (the spare row is untouched).
    paged16: the ranges straddle a block boundary in the source and in both destinations (fp32_refs.KVS)."""
    c = R.KVS
    L, B, H, p0, pads, smax, bs = c["L"], c["B"], c["H"], c["p0"], c["pads"], c["smax"], c["bs"]
    rows = B + 1 if form == "contiguous-spare-rows" else B
    k = R.rnd(L, rows, H, smax, 64, seed=3900 + C, device=DEV).to(dtype)
    v = R.rnd(L, rows, H, smax, 64, seed=3950 + C, device=DEV).to(dtype)
    what = f"kv_share_rows {form} C={C}"
    for caches_b in (1, B):
        want_k, want_v = R.kv_share_expected(k, caches_b, C, p0, pads), R.kv_share_expected(v, caches_b, C, p0, pads)
        if form == "paged16":
            # one table for all layers; a layer's pool is the logical rows dealt to shuffled blocks, sentinel in the scratch block
            pools = [R.paged_pool(k[layer], v[layer], bs, seed=7, fill=7.0) for layer in range(L)]
            tab = pools[0][2]
            pk, pv = torch.stack([p[0] for p in pools]).contiguous(), torch.stack([p[1] for p in pools]).contiguous()
            pk0, pv0 = pk.clone(), pv.clone()
            nat.kv_share_rows(pk, pv, caches_b, H, C, p0, i32(pads), 0, kv_tab=i32(tab), kv_bs=bs)
            for layer in range(L):
                assert torch.equal(R.unpage(pk[layer], tab, smax, bs), want_k[layer]), f"{what}: K of layer {layer}"
                assert torch.equal(R.unpage(pv[layer], tab, smax, bs), want_v[layer]), f"{what}: V of layer {layer}"
            used = torch.zeros(pk.shape[1], dtype=torch.bool, device=DEV)
            used[torch.from_numpy(tab[:, :(smax + bs - 1) // bs].astype(np.int64).ravel()).to(DEV)] = True
            assert torch.equal(pk[:, ~used], pk0[:, ~used]) and torch.equal(pv[:, ~used], pv0[:, ~used]), f"{what}: an unmapped block was written"
            if caches_b == 1:
                assert torch.equal(pk, pk0) and torch.equal(pv, pv0), f"{what}: B = 1 wrote something"
        else:
            kc, vc = k.clone(), v.clone()
            assert kc.stride(0) == rows * H * smax * 64
            nat.kv_share_rows(kc, vc, caches_b, H, C, p0, i32(pads), smax)
            assert torch.equal(kc, want_k), f"{what}: K differs (B = {caches_b})"
            assert torch.equal(vc, want_v), f"{what}: V differs (B = {caches_b})"
            if caches_b == 1:
                assert torch.equal(kc, k) and torch.equal(vc, v), f"{what}: B = 1 wrote something"
    assert not torch.equal(want_k, k) and not torch.equal(want_v, v)
    print(f"fp64 | exact | {what} {dtype}: ranges ==, everything else untouched | 0.000")


# ------------------------------------------------------------------------------------------------- production coverage
@pytest.fixture(scope="module")
def production(nat):
    """The native calls of a 2-layer full-width fp32 engine (D = 1280, H = 20, V = 8194; synthetic weights): a prefill and one decode
    step at batch 1 and at batch 32, and a prefill plus two steps of a 2 x 3-beam search (the row-table form)."""
    import os

    import synth
    import test_lora_bank_gpu as lb
    import weights
    sd = weights.gpt_state_dict(2)
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gpt_small.npz"))
    text1 = torch.from_numpy(g["text"][0:1, :int(g["text_lens"][0])]).to(DEV)
    cond_mel = torch.from_numpy(synth.uniform("in.cond_mel", (1, 100, 120), -6.0, 2.0)).to(DEV)
    names = ("gemm_skinny", "attn_decode", "attn_prefill", "attn_prefill_packed", "attn_prefill_prefix", "attn_prefill_shared",
             "ln_reduce", "layernorm", "embed_step", "kv_share_rows")
    orig = {n: getattr(nat, n) for n in names}
    calls = []
    cfg = [""]

    def wrap(name):
        def wrapped(*a, **k):
            if name == "gemm_skinny":
                dtype, M, N, K = a[:4]
                calls.append((cfg[0], name, dict(dtype=dtype, M=M, N=N, K=K, epi=k.get("epi", 0), ksplit=k.get("ksplit", 1),
                                                 rpw=k.get("rows_per_wg", 0), wide=bool(k.get("wide_wg", False)), fold=k.get("ln_c") is not None,
                                                 ypk=bool(k.get("y_packed", False)), bs=int(k.get("kv_bs", 0)) if k.get("kv_tab") is not None else 0,
                                                 copy=k.get("y") is not None)))
            elif name == "attn_decode":
                paged = k.get("kv_tab") is not None
                form = "row-table" if k.get("kv_rows") is not None else f"paged{int(k['kv_bs'])}" if paged else "contiguous"
                calls.append((cfg[0], name, dict(dtype=a[0].dtype, form=form, packed=bool(k.get("out_packed", False)), B=a[6])))
            elif name.startswith("attn_prefill"):
                calls.append((cfg[0], name, dict(dtype=a[0].dtype)))
            elif name in ("ln_reduce", "layernorm"):
                calls.append((cfg[0], name, dict(dtype=a[3].dtype, M=a[0].shape[0], D=a[0].shape[1], nslab=k.get("nslab", 0),
                                                 two=(k.get("w2") is not None) or len(a) > 4, packed=bool(k.get("y_packed", False)))))
            elif name == "embed_step":
                hp = k.get("h_packed")
                calls.append((cfg[0], name, dict(dtype=F32 if hp is None else hp.dtype, B=a[5].shape[0])))
            else:
                calls.append((cfg[0], name, dict(dtype=a[0].dtype, C=a[4])))
            return orig[name](*a, **k)
        return wrapped
    m = lb.make_model(sd, F32)
    eng = m.engine
    conds = m.get_conditioning(cond_mel, None)
    for n in names:
        setattr(nat, n, wrap(n))
    try:
        for B in (1, 32):
            cfg[0] = f"B={B}"
            emb, pad = m.prefix_rows(conds, text1.repeat(B, 1))
            eng.prefill(emb, pad, 8)
            eng._step_transformer(B)
        cfg[0] = "2 x 3 beams"
        emb, pad = m.prefix_rows(conds, text1.repeat(2, 1))
        eng.prefill_beams(emb, pad, 4, 3)
        eng.decode_beam(2, dict(do_sample=False, top_p=1.0, top_k=0, temperature=1.0, repetition_penalty=10.0, seed=0, length_penalty=0.0), 3,
                        use_graph=False)
        torch.cuda.synchronize()
    finally:
        for n in names:
            setattr(nat, n, orig[n])
    del m
    return calls


def test_production_fp32_forms_are_pinned_and_hold_fp64(nat, production):
    """Every skinny-GEMM call of the fp32 engine maps to a pinned form key and epilogue, every attention call to a pinned form (run the
    whole file: the cases fill the sets), and every distinct skinny signature passes the fp64 check of run_gemm at its own size."""
    if not PINNED or not ATTN_PINNED:
        pytest.skip("no kernel case ran in this process (the cases of this file fill the pinned sets: run the whole file)")
    names = {nat.EPI_STORE: "store", nat.EPI_QKV_CACHE: "qkv", nat.EPI_GELU_STORE: "gelu", nat.EPI_RESID_F32: "resid", nat.EPI_SLAB_F32: "slab",
             nat.EPI_STORE_F32: "store_f32"}
    seen, missing = {}, []
    kinds = {}
    for cfg, name, c in production:
        kinds.setdefault(cfg, set()).add(name)
        assert c["dtype"] == F32, (cfg, name, c)
        if name == "gemm_skinny":
            assert c["epi"] in names and not c["fold"] and c["rpw"] == 0, (cfg, c)
            key = form_key(nat, F32, c["M"], c["N"], c["K"], c["ksplit"], 0, c["wide"], False)
            print(f"production | {cfg} | M={c['M']} N={c['N']} K={c['K']} {names[c['epi']]} ksplit={c['ksplit']} wide={c['wide']} "
                  f"packed-y={c['ypk']} paged={c['bs']} -> {key}")
            if key not in PINNED or names[c["epi"]] not in EPIS_PINNED:
                missing.append((cfg, c, key))
            seen.setdefault(tuple(sorted((k, str(v)) for k, v in c.items())), (c, key))
        elif name == "attn_decode":
            print(f"production | {cfg} | attn_decode {c['form']} packed-out={c['packed']} B={c['B']}")
            if (c["form"], c["packed"], False) not in ATTN_PINNED:      # (the engine's kv_share word is 0 here: no shared rows were promised)
                missing.append((cfg, name, c))
        elif name.startswith("attn_prefill"):
            print(f"production | {cfg} | {name}")
            if name not in ATTN_PINNED:
                missing.append((cfg, name, c))
        else:
            print(f"production | {cfg} | {name} {c}")
    assert not missing, f"production calls whose form no case pins: {missing}"
    for cfg in ("B=1", "B=32", "2 x 3 beams"):
        assert {"gemm_skinny", "attn_decode", "ln_reduce", "embed_step"} <= kinds[cfg] and any(n.startswith("attn_prefill") for n in kinds[cfg]), (cfg, kinds[cfg])
    forms = {c["form"] for _, name, c in production if name == "attn_decode"}
    assert "row-table" in forms and len(forms) >= 2, forms
    assert {c["M"] for c, _ in seen.values()} >= {1, 6, 32}
    for i, (c, key) in enumerate(seen.values()):
        run_gemm(nat, c["M"], c["N"], c["K"], key, epi=names[c["epi"]], ksplit=c["ksplit"], wide=c["wide"], ypk=c["ypk"], copy=c["copy"],
                 bs=c["bs"], seed=9000 + 10 * i, pin=False)
