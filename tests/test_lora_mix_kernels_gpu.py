"""itts_lora_shrink_mix (include/indextts_hip.h): the adapter bank's shrink launch over weighted mixes of up to four voices per
row, at the shapes of test_lora_bank_gpu.py::test_shrink_kernel_against_fp64_on_the_rounded_operands (the smallest that take every
path: rp = 48 -> Kx = 160 with padding to 32, one / several / many pieces per lane, a partial tile and three tiles).

Named slots are held to fp64 on the rounded operands with that test's bound; everything else to exact zeros; the two output forms
and every order of a record's entries to the same bits; a record {a, 1.0} to the bits of itts_lora_shrink."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
RES = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -23}
N, RANKS, RP = 3, (4, 16, 40), 48


def kinds(m):
    """The six kinds of record, the adapters they name turning with the row."""
    a, b = m % N, (m + 1) % N
    return [[], [(a, 1.0)], [(a, 0.35)], [(a, 0.7), (b, 0.3)], [(0, 0.5), (1, -0.75), (2, 1.25)], [(2, 1.25), (0, 0.5), (1, -0.75)]]


def record_set(M, shift):
    return [kinds(m)[(m + shift) % 6] for m in range(M)]


def moved(mix):
    """The same entries in the opposite order, pushed to the END of the record (empty entries in front)."""
    return [[(-1, 0.0)] * (4 - len(r)) + r[::-1] for r in mix]


def upload(nat, mix):
    return torch.from_numpy(nat.pack_lora_mix(mix)).to(DEV)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("K", [64, 1280, 5120])
def test_mix_kernel_against_fp64_on_the_rounded_operands(dtype, K):
    """n = 3 adapters of ranks 4 / 16 / 40, M = 5 and 37, both output forms, the six kinds of record dealt to the rows in rotation
    (three rotations, then the same records with their entries reversed and moved to the end), every set written into the SAME
    buffer, which starts as 7.0: nothing of the call before may survive.
    Named slot of entry (a, w): |got - ref| <= RES[T] |ref| + 1e-5 |w| sum_k |x a|, ref = w (x . a) in fp64 from the rounded
    operands and the fp32 weight: one rounding of T and fp32 accumulation; the weight is one more fp32 multiply in front of that
    rounding, which the second term covers many times over.  Unnamed slots, the rank padding, the Kx padding and the padding
    rows of the packed tail: exactly 0."""
    from indextts import _native as nat
    Kx = nat.lora_kx(N, RP)
    assert Kx == 160
    g = torch.Generator().manual_seed(K)
    A32 = torch.zeros(N, RP, K)
    for a, r in enumerate(RANKS):
        A32[a, :r] = torch.randn(r, K, generator=g) * 0.05 * (a + 1)       # (a + 1): the scaling, folded in at fp32
    A = A32.to(dtype).to(DEV).contiguous()
    Ad = A.double().cpu()
    for M in (5, 37):
        x = torch.randn(M, K, generator=g).to(dtype).to(DEV).contiguous()
        xd = x.double().cpu()
        dots = torch.einsum("ark,mk->mar", Ad, xd)                         # [M, n, rp] fp64
        mags = torch.einsum("ark,mk->mar", Ad.abs(), xd.abs())
        Mp = nat.packed_rows(M)
        packed = torch.cat([nat.pack_activation(x), torch.full((Mp * Kx,), 7.0, dtype=dtype, device=DEV)])
        rows = torch.full((M, K + Kx), 7.0, dtype=dtype, device=DEV)
        rows[:, :K] = x
        seen = set()
        for shift in (0, 1, 2):
            mix = record_set(M, shift)
            seen |= {(m % N, (m + shift) % 6) for m in range(M)}
            tails = []
            for recs in (mix, moved(mix)):
                tab = upload(nat, recs)
                nat.lora_shrink_mix(packed, tab, A, packed[Mp * K:], M, K, x_packed=True, u_packed=True)
                nat.lora_shrink_mix(x, tab, A, rows[:, K:], M, K, ldu=K + Kx)
                whole = nat.unpack_activation(packed, Mp, K + Kx)
                assert torch.equal(whole[:M, :K], x) and torch.equal(rows[:, :K], x)      # the operand's front is not touched
                assert (whole[M:, K:] == 0).all()                                           # padding rows of the tail
                assert torch.equal(whole[:M, K:], rows[:, K:])                              # the two forms: same bits
                tails.append(rows[:, K:].clone())
            assert torch.equal(tails[0], tails[1])                                          # the entries' order moves no bit
            u = tails[0].double().cpu()
            for m, rec in enumerate(mix):
                mask = torch.ones(Kx, dtype=torch.bool)
                for a, w in rec:
                    own = slice(a * RP, (a + 1) * RP)
                    mask[own] = False
                    w32 = float(np.float32(w))
                    ref = w32 * dots[m, a]
                    err = (u[m][own] - ref).abs()
                    assert (err <= RES[dtype] * ref.abs() + 1e-5 * abs(w32) * mags[m, a]).all(), (M, shift, m, a, w, err.max().item())
                    assert (u[m][own][RANKS[a]:] == 0).all()                                # rank padding
                    assert (u[m][own][:RANKS[a]] != 0).any()
                assert (u[m][mask] == 0).all(), (M, shift, m, rec)                          # unnamed slots, Kx padding
        assert M < 18 or len(seen) == 18       # (37 rows: every kind met every adapter rotation)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
@pytest.mark.parametrize("K", [64, 1280, 5120])
def test_one_entry_at_weight_one_gives_the_bits_of_lora_shrink(dtype, K):
    """Records {ids[m], 1.0} (and the empty record for -1), wherever the entry stands in the record, against itts_lora_shrink over
    the same ids: torch.equal tails in both output forms -- the same accumulation order, and the multiply by 1.0 is exact."""
    from indextts import _native as nat
    Kx = nat.lora_kx(N, RP)
    g = torch.Generator().manual_seed(K + 1)
    A32 = torch.zeros(N, RP, K)
    for a, r in enumerate(RANKS):
        A32[a, :r] = torch.randn(r, K, generator=g) * 0.05 * (a + 1)
    A = A32.to(dtype).to(DEV).contiguous()
    for M in (5, 37):
        x = torch.randn(M, K, generator=g).to(dtype).to(DEV).contiguous()
        Mp = nat.packed_rows(M)
        ids = [(i * 7) % 4 - 1 for i in range(M)]
        ids_t = torch.tensor(ids, dtype=torch.int32, device=DEV)
        want_p = torch.cat([nat.pack_activation(x), torch.full((Mp * Kx,), 7.0, dtype=dtype, device=DEV)])
        want_r = torch.full((M, Kx), 7.0, dtype=dtype, device=DEV)
        nat.lora_shrink(want_p, ids_t, A, want_p[Mp * K:], M, K, x_packed=True, u_packed=True)
        nat.lora_shrink(x, ids_t, A, want_r, M, K, ldu=Kx)
        for place in (0, 3):
            recs = [[(-1, 0.0)] * place + ([(a, 1.0)] if a >= 0 else []) for a in ids]
            tab = upload(nat, recs)
            got_p = torch.cat([nat.pack_activation(x), torch.full((Mp * Kx,), 7.0, dtype=dtype, device=DEV)])
            got_r = torch.full((M, Kx), 7.0, dtype=dtype, device=DEV)
            nat.lora_shrink_mix(got_p, tab, A, got_p[Mp * K:], M, K, x_packed=True, u_packed=True)
            nat.lora_shrink_mix(x, tab, A, got_r, M, K, ldu=Kx)
            assert torch.equal(got_p, want_p) and torch.equal(got_r, want_r), (M, place)
        assert (want_r != 0).any()


def test_mix_refuses_shapes_outside_its_limits():
    from indextts import _native as nat
    x = torch.zeros(4, 64, dtype=torch.bfloat16, device=DEV)
    tab = upload(nat, [[(0, 1.0)]] * 4)
    u = torch.zeros(4, 512 + 64, dtype=torch.bfloat16, device=DEV)
    for n, rp in ((1, 80), (9, 64), (1, 24)):              # rank > 64; Kx > 512; rp not a multiple of 16
        with pytest.raises(nat.NativeError):
            nat.lora_shrink_mix(x, tab, torch.zeros(n, rp, 64, dtype=torch.bfloat16, device=DEV), u, 4, 64, ldu=u.shape[1])
    with pytest.raises(nat.NativeError):                   # K % KS != 0
        nat.lora_shrink_mix(x[:, :48].contiguous(), tab, torch.zeros(1, 16, 48, dtype=torch.bfloat16, device=DEV), u, 4, 48, ldu=u.shape[1])
    a16 = torch.zeros(1, 16, 64, dtype=torch.bfloat16, device=DEV)
    with pytest.raises(nat.NativeError):                   # ldu not a multiple of 16 bytes
        nat.lora_shrink_mix(x, tab, a16, u, 4, 64, ldu=36)
    with pytest.raises(nat.NativeError):                   # fewer records than rows
        nat.lora_shrink_mix(x, tab[:3], a16, u, 4, 64, ldu=u.shape[1])
    with pytest.raises(nat.NativeError):                   # records are bytes
        nat.lora_shrink_mix(x, tab.view(torch.int32), a16, u, 4, 64, ldu=u.shape[1])
    with pytest.raises(nat.NativeError):                   # an operand of another type than the bank's
        nat.lora_shrink_mix(x.float(), tab, a16, u, 4, 64, ldu=u.shape[1])
    torch.cuda.synchronize()
