"""lora_refs.py on its own, no GPU: the float32 stand-in of the shrink kernels' order of operations is held to the derived bound at
every case of test_lora_kernels_gpu.py, and every negative control is shown to exceed the bound against the stand-in's output at
every case it is declared for -- so the operands, weights and element counts chosen there make each wrong reference visible on the
reference side alone (`rounded twice` in particular: the weights are no powers of two).  Prints the `fp64 | case | ...` and
`fp64 | control | ...` lines of profiles/lora_kernels_fp64.txt."""
import pytest
import torch

import lora_refs as R
from fp64_check import bad, ok, tname


def launches(c, M):
    """(what, recs, rows, mix) of the launches the GPU file makes over the first M rows: every set of a kind in one check."""
    ids = R.id_sets(M)
    mixes = R.mix_sets(M)
    rows = list(range(M))
    yield "ids", sum((R.as_records(s) for s in ids), []), rows * len(ids), False
    yield "mix", sum(mixes, []), rows * len(mixes), True


def test_the_tree_of_reduce16_sums_every_accumulator_of_every_lane():
    """Integers: every order of addition is exact, so reduce16 must return the plain sum of accumulator j over the 64 lanes at j."""
    v = torch.randint(-1000, 1000, (3, 16, 64), generator=torch.Generator().manual_seed(1)).float()
    assert torch.equal(R.reduce16(v), v.sum(-1))


def test_raw_records_are_the_packed_records():
    rec = R.raw_records([[(2, 0.35)], [], [(0, 0.5), (1, -0.75), (0, 2.0), (5, 1e4)]])
    assert rec.shape == (3, 32) and rec.dtype == torch.uint8
    ids = rec.view(torch.int32).view(3, 4, 2)[..., 0]
    wts = rec.view(torch.float32).view(3, 4, 2)[..., 1]
    assert ids.tolist() == [[2, -1, -1, -1], [-1] * 4, [0, 1, 0, 5]]
    assert wts[2].tolist() == [0.5, -0.75, 2.0, 1e4] and wts[0, 0].item() == R.f32(0.35) and (wts[1] == 0).all()


@pytest.mark.parametrize("dtype,rp,K", R.FORMS, ids=R.form_id)
def test_standin_within_the_bound_and_controls_beyond_it(dtype, rp, K):
    c = R.case(dtype, K, rp)
    for M in (1, 16, 17):
        for kind, recs, rows, mix in launches(c, M):
            R.verify(f"standin {kind} {tname(dtype)} rp{rp} K{K} M{M}", c, recs, rows, R.standin(c, recs, rows), ok, bad, mix)


@pytest.mark.parametrize("dtype,rp,K", R.STASH, ids=R.form_id)
def test_standin_and_controls_at_the_stash_boundary(dtype, rp, K):
    """At 9 P no lane has a piece 9: `stash dropped` is the reference itself there, and is declared at 9 P + KS only."""
    c = R.case(dtype, K, rp, M=3)
    rows = [0, 1, 2]
    what = f"standin stash {tname(dtype)} rp{rp} K{K} M3"
    R.verify(what + " ids", c, R.as_records([0, 1, 2]), rows, R.standin(c, R.as_records([0, 1, 2]), rows), ok, bad, False)
    R.verify(what + " mix", c, R.stash_mix(), rows, R.standin(c, R.stash_mix(), rows), ok, bad, True)
    assert "stash shifted" in R.controls_for(dtype, K, 3, True)
    dropped = R.control(c, "stash dropped", R.stash_mix(), rows)
    if K == 9 * R.P(dtype):
        assert torch.equal(dropped, R.expected(c, R.stash_mix(), rows)[0])
    else:
        assert "stash dropped" in R.controls_for(dtype, K, 3, True)


@pytest.mark.parametrize("dtype,n,rp", R.LIMIT, ids=R.form_id)
def test_standin_at_the_kx_limit(dtype, n, rp):
    c = R.case(dtype, 1280, rp, M=5, n=n)
    assert c.Kx == 512
    rows = list(range(5))
    what = f"standin limit {tname(dtype)} n{n} rp{rp} K1280 M5"
    R.verify(what + " ids", c, R.as_records(R.limit_ids(n)), rows, R.standin(c, R.as_records(R.limit_ids(n)), rows), ok, bad, False)
    R.verify(what + " mix", c, R.limit_mix(n), rows, R.standin(c, R.limit_mix(n), rows), ok, bad, True)


def test_every_instance_and_every_control_is_declared_somewhere():
    """24 (T, NCH) instances per kernel among the forms; every control on some form of every type it is declared for."""
    assert len({(d, rp) for d, rp, _ in R.FORMS}) == 12
    for dtype in R.DTYPES:
        got = set()
        for d, _, K in R.FORMS + R.STASH:
            if d == dtype:
                got |= set(R.controls_for(d, K, 3, True))
        want = set(R.GENERAL + R.MIX_ONLY + ("stash shifted", "stash dropped"))
        assert got == (want - {"rounded twice"} if dtype == torch.float32 else want)
