"""itts_refill_join alone, through the C ABI (include/indextts_hip.h): the one launch that takes staged rows into a running
decode loop equals, bit for bit, the torch scatters and indexed writes it replaces -- on sentinel-filled caches and state, so that an
element written where none should be shows.  M = 58 staged positions over k = 3 rows of 1, 17 and 40 positions, L = 2, bs = 16: a
row inside one block, a row crossing a block boundary, a row over three blocks with non-contiguous block ids."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
L, H, BS, BLOCKS, SLOTS, SMAX, HIST = 2, 3, 16, 12, 6, 64, 24
LENS = [1, 17, 40]
ROWS = [4, 1, 2]                        # the slots the three rows take (0, 3 and 5 are not named)
M = sum(LENS)


def positions(paged):
    """(i_b, i_p) of the 58 staged positions: row j ends at position 47 of its slot (left padding 47 - LENS[j] + 1)."""
    ib, ip = [], []
    tables = {4: {2: 7}, 1: {1: 3, 2: 9}, 2: {0: 11, 1: 2, 2: 6}}            # slot -> {position // bs: block}: non-contiguous ids
    for slot, n in zip(ROWS, LENS):
        for pos in range(48 - n, 48):
            ib.append(tables[slot][pos // BS] if paged else slot)
            ip.append(pos % BS if paged else pos)
    return ib, ip


def make(dtype, paged, seed=0):
    g = torch.Generator().manual_seed(seed)
    shape = (L, BLOCKS, H, BS, 64) if paged else (L, SLOTS, H, SMAX, 64)
    i32 = lambda *s, lo=-90000, hi=-80000: torch.randint(lo, hi, s, generator=g, dtype=torch.int32).to(DEV)   # noqa: E731  sentinels
    d = dict(kc=torch.full(shape, -7.0, dtype=dtype, device=DEV), vc=torch.full(shape, 9.0, dtype=dtype, device=DEV),
             kst=torch.randn(M, L, H, 64, generator=g).to(DEV, dtype), vst=torch.randn(M, L, H, 64, generator=g).to(DEV, dtype),
             tokens=i32(SLOTS), history=i32(SLOTS, HIST), finished=i32(SLOTS), force_stop=i32(SLOTS), row_step0=i32(SLOTS),
             pad=i32(SLOTS), mix=torch.randint(0, 255, (SLOTS, 32), generator=g, dtype=torch.uint8).to(DEV),
             state=torch.tensor([5, 40, 4, 0, 0, 0, 0, 0], dtype=torch.int32, device=DEV),
             tok=i32(3, lo=0, hi=8000), fin=torch.tensor([0, 1, 0], dtype=torch.int32, device=DEV), stops=i32(3, lo=3, hi=30),
             pads=torch.tensor([48 - n for n in LENS], dtype=torch.int32, device=DEV),
             mix_new=torch.randint(0, 255, (3, 32), generator=g, dtype=torch.uint8).to(DEV))
    return d


def by_torch(d, ib, ip, rows, step0):
    """What GPTEngine._join does without the kernel, with out-of-range entries left out by hand."""
    nb, npos = d["kc"].shape[1], d["kc"].shape[3]
    keep = [m for m in range(len(ib)) if 0 <= ib[m] < nb and 0 <= ip[m] < npos]
    b = torch.tensor([ib[m] for m in keep], device=DEV)
    p = torch.tensor([ip[m] for m in keep], device=DEV)
    sel = torch.tensor(keep, device=DEV)
    d["kc"][:, b, :, p] = d["kst"][sel]
    d["vc"][:, b, :, p] = d["vst"][sel]
    ok = [j for j, r in enumerate(rows) if 0 <= r < SLOTS]
    r, j = torch.tensor([rows[j] for j in ok], device=DEV), torch.tensor(ok, device=DEV)
    d["tokens"][r] = d["tok"][j]
    d["history"][r, 0] = d["tok"][j]
    d["finished"][r] = d["fin"][j]
    d["force_stop"][r] = d["stops"][j]
    d["row_step0"][r] = step0
    d["pad"][r] = d["pads"][j]
    d["mix"][r] = d["mix_new"][j]
    d["state"][2:3] -= len(rows)


def by_kernel(d, ib, ip, rows, step0):
    from indextts import _native as nat
    t32 = lambda v: torch.tensor(v, dtype=torch.int32, device=DEV)   # noqa: E731
    nat.refill_join(d["kst"], d["vst"], d["kc"], d["vc"], t32(ib), t32(ip), t32(rows), d["tok"], d["fin"], d["stops"], d["pads"], step0,
                    d["tokens"], d["history"], d["finished"], d["force_stop"], d["row_step0"], d["pad"], d["state"],
                    mix_new=d["mix_new"], mix=d["mix"])
    torch.cuda.synchronize()


WRITTEN = ("kc", "vc", "tokens", "history", "finished", "force_stop", "row_step0", "pad", "mix", "state")


@pytest.mark.parametrize("paged", [True, False], ids=["paged", "rows"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=["bf16", "f16", "f32"])
def test_refill_join_equals_the_torch_scatters(dtype, paged):
    ib, ip = positions(paged)
    assert len(ib) == M == 58
    if paged:
        assert len({ib[m] for m in range(1, 18)}) == 2 and [ib[18], ib[26], ib[57]] == [11, 2, 6]
    want, got, before = make(dtype, paged), make(dtype, paged), make(dtype, paged)
    by_torch(want, ib, ip, ROWS, 17)
    by_kernel(got, ib, ip, ROWS, 17)
    for name in WRITTEN:
        assert torch.equal(got[name], want[name]), name
    # the comparison is not vacuous, and nothing outside the named positions / slots moved (the torch form is exact about both,
    # stated here without it)
    changed = (got["kc"] != before["kc"]).any(-1)                                    # [L, n_b, H, n_p]
    named = torch.zeros_like(changed)
    named[:, torch.tensor(ib, device=DEV), :, torch.tensor(ip, device=DEV)] = True
    assert int(named.sum()) == L * H * M and torch.equal(changed, named)
    assert torch.equal((got["vc"] != before["vc"]).any(-1), named)
    for slot in (0, 3, 5):
        for name in ("tokens", "history", "finished", "force_stop", "row_step0", "pad", "mix"):
            assert torch.equal(got[name][slot], before[name][slot]), (name, slot)
    assert torch.equal(got["history"][:, 1:], before["history"][:, 1:])
    assert got["state"].tolist() == [5, 40, 1, 0, 0, 0, 0, 0]                         # state[2] dropped by exactly k = 3
    assert got["row_step0"][torch.tensor(ROWS, device=DEV)].tolist() == [17] * 3


@pytest.mark.parametrize("paged", [True, False], ids=["paged", "rows"])
def test_out_of_range_entries_are_skipped_and_their_neighbours_written(paged):
    ib, ip = positions(paged)
    nb = BLOCKS if paged else SLOTS
    ib[0], ib[5], ib[30], ip[40] = nb, -1, nb + 1000, (BS if paged else SMAX)       # a block / row and an offset outside the cache
    rows = [4, SLOTS, 2]                                                              # and a slot outside the tables
    want, got = make(torch.bfloat16, paged, 1), make(torch.bfloat16, paged, 1)
    by_torch(want, ib, ip, rows, 3)
    by_kernel(got, ib, ip, rows, 3)
    for name in WRITTEN:
        assert torch.equal(got[name], want[name]), name
    assert got["state"][2].item() == 1 and got["tokens"][4].item() == got["tok"][0].item() and got["tokens"][2].item() == got["tok"][2].item()
    rows[1] = -1
    by_torch(want, ib, ip, rows, 4)
    by_kernel(got, ib, ip, rows, 4)
    for name in WRITTEN:
        assert torch.equal(got[name], want[name]), name


def test_bad_calls_are_reported_without_launching():
    import ctypes
    from indextts import _native as nat
    lib = nat.lib()
    a = nat.RefillJoinArgs()
    a.dtype, a.M, a.L, a.H, a.k = 7, 0, 2, 3, 0
    assert lib.itts_refill_join(ctypes.byref(a), None) == 1 and b"dtype" in lib.itts_last_error()
    a.dtype, a.M = nat.BF16, 4                                                        # positions but no buffers
    assert lib.itts_refill_join(ctypes.byref(a), None) == 1 and b"null" in lib.itts_last_error()
    a.M, a.hist_cap = 0, 1                                                            # nothing to do is not an error
    assert lib.itts_refill_join(ctypes.byref(a), None) == 0
    d = make(torch.bfloat16, True)
    with pytest.raises(nat.NativeError):                                              # int64 indices: the wrapper wants int32
        nat.refill_join(d["kst"], d["vst"], d["kc"], d["vc"], torch.zeros(M, dtype=torch.int64, device=DEV),
                        torch.zeros(M, dtype=torch.int64, device=DEV), torch.tensor(ROWS, dtype=torch.int32, device=DEV), d["tok"], d["fin"],
                        d["stops"], d["pads"], 0, d["tokens"], d["history"], d["finished"], d["force_stop"], d["row_step0"], d["pad"],
                        d["state"], mix_new=d["mix_new"], mix=d["mix"])
