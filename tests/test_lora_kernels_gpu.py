"""Every form of the adapter bank's shrink kernels (csrc/lora.hip) against float64, through indextts._native:
lora_shrink_kernel<T, NCH> (itts_lora_shrink) and lora_shrink_mix_kernel<T, NCH> (itts_lora_shrink_mix), T in fp32 / bf16 / f16,
NCH = rp / 16 in 1 .. 4 -- 24 instances.  The reference, the bound 0.5 ulp_T(|ref| + C mag) + C mag with its derivation, the
records, the ids and the negative controls are lora_refs.py's; test_lora_refs_cpu.py shows without a GPU that every control
exceeds that bound.

Every launch goes out in both output forms -- the packed tail behind a packed x, and a row-major u at column K of an
[M][K + Kx + 16] operand -- into buffers that start as 7.0 and are written again and again: nothing of the call before may
survive, the operand's front and the 16 columns behind Kx keep what they held, the padding rows of the packed tail are zeros, and
the two forms agree bit for bit.  The bank is the leading [:n] of an allocation of n + 2 adapters whose last two hold large
values; ids n, n + 1 and -7 must read nothing and give zero rows, and no id beyond n + 1 is ever passed.
Per form: K = KS (one lane group works), P - KS, P, P + KS (one pass of the workgroup less / exactly / plus one k-step), 1280, 5120;
M = 1, 16, 17; for rp = 32 and 64 also K = 9 P and 9 P + KS, where the mix kernel's x stash ends and piece 9 is requested again by
every entry.  Exact relations: a record {a, 1.0} in entry 0 or 3 gives the bits of the id launch; reversing a record moves no bit.
`-s` prints the `fp64 | kind | case | ratio` lines of profiles/lora_kernels_fp64.txt."""
import pytest
import torch

import lora_refs as R
from fp64_check import bad, ok, tname

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 7.0


class Buffers:
    """x [:M] of a case on the device in both forms, the bank, and the two outputs."""

    def __init__(self, nat, c, M):
        self.nat, self.c, self.M, self.Mp = nat, c, M, nat.packed_rows(M)
        assert nat.lora_kx(c.n, c.rp) == c.Kx
        self.spare = c.bank.to(DEV).contiguous()
        self.A = self.spare[:c.n]                                   # two more adapters stand behind the bank
        self.x = c.x[:M].to(DEV).contiguous()
        self.packed = torch.cat([nat.pack_activation(self.x), torch.full((self.Mp * c.Kx,), SENTINEL, dtype=c.dtype, device=DEV)])
        self.rows = torch.full((M, c.K + c.Kx + 16), SENTINEL, dtype=c.dtype, device=DEV)
        self.rows[:, :c.K] = self.x

    def run(self, table, mix):
        """One launch per output form; returns the tail [M][Kx] after the checks every launch owes."""
        c, M, Mp, nat = self.c, self.M, self.Mp, self.nat
        fn = nat.lora_shrink_mix if mix else nat.lora_shrink
        if mix:
            table = R.raw_records(table)
        else:
            table = torch.tensor(table, dtype=torch.int32)
        table = table.to(DEV)
        fn(self.packed, table, self.A, self.packed[Mp * c.K:], M, c.K, x_packed=True, u_packed=True)
        fn(self.x, table, self.A, self.rows[:, c.K:], M, c.K, ldu=c.K + c.Kx + 16)
        whole = nat.unpack_activation(self.packed, Mp, c.K + c.Kx)
        assert torch.equal(whole[:M, :c.K], self.x) and torch.equal(self.rows[:, :c.K], self.x)     # the operand's front
        assert (self.rows[:, c.K + c.Kx:] == SENTINEL).all()                                         # ldu > Kx: what stands behind
        assert (whole[M:, c.K:] == 0).all()                                                          # padding rows of the tail
        tail = self.rows[:, c.K:c.K + c.Kx].clone()
        assert torch.equal(whole[:M, c.K:], tail)                                                    # the two forms: same bits
        return tail


def both_launches(nat, c, M, what, id_sets, mix_sets):
    """The id launch over `id_sets` (and the records {id, 1.0} in entry 0 and 3 beside it), the mix launch over `mix_sets` (and the
    reversed records beside it); every kind's sets in one check against float64."""
    b = Buffers(nat, c, M)
    rows = list(range(M))
    tails = []
    for ids in id_sets:
        tails.append(b.run(ids, False))
        for place in (0, 3):
            assert torch.equal(b.run(R.as_records(ids, place), True), tails[-1]), (what, ids, place)
    R.verify(f"ids {what}", c, sum((R.as_records(s) for s in id_sets), []), rows * len(id_sets), torch.cat(tails), ok, bad, False)
    tails = []
    for recs in mix_sets:
        tails.append(b.run(recs, True))
        assert torch.equal(b.run(R.moved(recs), True), tails[-1]), (what, recs)
    R.verify(f"mix {what}", c, sum(mix_sets, []), rows * len(mix_sets), torch.cat(tails), ok, bad, True)
    assert (b.spare[c.n:].cpu() == c.bank[c.n:]).all()


def test_raw_records_are_pack_lora_mix_records():
    from indextts import _native as nat
    recs = [r for r in R.mix_sets(17)[0] if len({a for a, _ in r}) == len(r)]
    assert torch.equal(R.raw_records(recs), torch.from_numpy(nat.pack_lora_mix(recs)))


@pytest.mark.parametrize("dtype,rp,K", R.FORMS, ids=R.form_id)
def test_every_form_against_fp64(dtype, rp, K):
    """n = 3 adapters of mixed ranks (lora_refs.RANKS; Kx = 64, 96, 160, 192: with and without padding to 32), M = 1, 16, 17, the id
    sets (-1, the bank's ids, n, n + 1, -7) and the ten kinds of record in rotation, the controls at K = P + KS."""
    from indextts import _native as nat
    c = R.case(dtype, K, rp)
    assert c.Kx == {16: 64, 32: 96, 48: 160, 64: 192}[rp]
    for M in (1, 16, 17):
        both_launches(nat, c, M, f"{tname(dtype)} rp{rp} K{K} M{M}", R.id_sets(M), R.mix_sets(M))


@pytest.mark.parametrize("dtype,rp,K", R.STASH, ids=R.form_id)
def test_stash_boundary_against_fp64(dtype, rp, K):
    """K = 9 P: pieces 1 .. 8 of every lane are read back from LDS by the entries behind a record's first; 9 P + KS: the first
    lanes request piece 9 again in every entry.  M = 3, records of 1, 2 and 4 entries; the controls include a shifted stash slot
    and, where a piece 9 exists, a dropped one."""
    from indextts import _native as nat
    c = R.case(dtype, K, rp, M=3)
    both_launches(nat, c, 3, f"stash {tname(dtype)} rp{rp} K{K} M3", [[0, 1, 2]], [R.stash_mix()])


@pytest.mark.parametrize("dtype,n,rp", R.LIMIT, ids=R.form_id)
def test_kx_limit_against_fp64(dtype, n, rp):
    """Kx = 512, the limit, at both shapes that reach it; ids and records name the first and the last slot."""
    from indextts import _native as nat
    c = R.case(dtype, 1280, rp, M=5, n=n)
    assert c.Kx == 512
    both_launches(nat, c, 5, f"limit {tname(dtype)} n{n} rp{rp} K1280 M5", [R.limit_ids(n)], [R.limit_mix(n)])


@pytest.mark.parametrize("dtype", R.DTYPES, ids=R.form_id)
def test_more_tiles_than_the_rows_need(dtype):
    """M = 17 with x_mtp = 3 and u_mtp = 4: x is the head of a packed operand of 48 rows (the rows behind M hold other values), the
    tail has four tiles.  The 17 rows carry the bits of the plain launch, the padding rows of all four tiles are zeros, x and the
    guard words behind the tail keep what they held."""
    from indextts import _native as nat
    rp, K, M = 32, 1280, 17
    c = R.case(dtype, K, rp)
    want = Buffers(nat, c, M)
    tall = torch.cat([c.x[:M], R.rnd(48 - M, K, seed=5).to(dtype)]).to(DEV)
    xp = nat.pack_activation(tall)
    front = xp.clone()
    A = want.A
    u = torch.full((64 * c.Kx + 64,), SENTINEL, dtype=dtype, device=DEV)
    ids = R.id_sets(M)[0]
    recs = R.mix_sets(M)[0]
    for table, mix in ((ids, False), (recs, True)):
        ref = want.run(table, mix)
        dev_table = (R.raw_records(table) if mix else torch.tensor(table, dtype=torch.int32)).to(DEV)
        (nat.lora_shrink_mix if mix else nat.lora_shrink)(xp, dev_table, A, u, M, K, x_packed=True, x_mtp=3, u_packed=True, u_mtp=4)
        got = nat.unpack_activation(u[:64 * c.Kx], 64, c.Kx)
        assert torch.equal(got[:M], ref) and (ref != 0).any(), mix
        assert (got[M:] == 0).all(), mix
        assert (u[64 * c.Kx:] == SENTINEL).all() and torch.equal(xp, front), mix
        u.fill_(SENTINEL)


def test_refusals_leave_the_output_untouched():
    """x_mtp * 16 < M; u_mtp given with a row-major u; Kx = 512 + 32 (n = 17, rp = 32): NativeError from both entry points, and
    not one word of u written."""
    from indextts import _native as nat
    M, K, dtype = 17, 64, torch.bfloat16
    x = torch.zeros(M, K, dtype=dtype, device=DEV)
    xp = nat.pack_activation(x)
    a3 = torch.ones(3, 32, K, dtype=dtype, device=DEV)
    a17 = torch.ones(17, 32, K, dtype=dtype, device=DEV)
    ids = torch.zeros(M, dtype=torch.int32, device=DEV)
    tab = R.raw_records([[(0, 1.0)]] * M).to(DEV)
    u = torch.full((32, 544 + 64), SENTINEL, dtype=dtype, device=DEV)
    for fn, table in ((nat.lora_shrink, ids), (nat.lora_shrink_mix, tab)):
        with pytest.raises(nat.NativeError):               # a packed x of one tile cannot hold 17 rows
            fn(xp, table, a3, u, M, K, x_packed=True, x_mtp=1, ldu=u.shape[1])
        with pytest.raises(nat.NativeError):               # u_mtp describes a packed u
            fn(x, table, a3, u, M, K, u_mtp=2, ldu=u.shape[1])
        with pytest.raises(nat.NativeError):               # Kx = 544 > 512
            fn(x, table, a17, u, M, K, ldu=u.shape[1])
        torch.cuda.synchronize()
        assert (u == SENTINEL).all(), fn.__name__
