"""itts_lora_shrink on the host side: the symbol is exported at ABI 9 beside the unchanged argument structs, and a call outside its
limits is reported without a launch (no GPU needed: validation comes first)."""
import ctypes


def args(nat, **kw):
    a = nat.LoraShrinkArgs()
    a.dtype, a.M, a.K = nat.BF16, 4, 64
    a.x = a.ids = a.a_bank = a.u = 0x1000          # never dereferenced: every call below fails its checks
    a.n, a.rp, a.Kx, a.ldu = 3, 16, 64, 128
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_lora_shrink_reports_bad_calls_without_launching():
    from indextts import _native as nat
    L = nat.lib()
    assert "itts_lora_shrink" in nat.EXPORTED_SYMBOLS and L.itts_abi_version() == 10
    assert nat.lora_kx(3, 48) == 160 and nat.lora_kx(8, 16) == 128 and nat.lora_kx(1, 16) == 32
    assert L.itts_lora_shrink(ctypes.byref(nat.LoraShrinkArgs()), None) == 1 and b"null" in L.itts_last_error()
    for kw, word in ((dict(n=0, Kx=0), b"adapters"), (dict(rp=80, Kx=256), b"rank"), (dict(rp=24, Kx=96), b"rp"),
                     (dict(n=9, rp=64, Kx=576), b"Kx"), (dict(Kx=96), b"Kx"), (dict(K=48), b"K %"), (dict(dtype=7), b"dtype"),
                     (dict(ldu=32), b"ldu"), (dict(u=0x1004), b"aligned"), (dict(x_mtp=1), b"x_mtp")):
        assert L.itts_lora_shrink(ctypes.byref(args(nat, **kw)), None) == 1, kw
        assert word in L.itts_last_error(), (kw, L.itts_last_error())
