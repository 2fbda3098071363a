"""FP8 KV cache, host side (no GPU): the E4M3 quantiser of keys / values against torch's float8_e4m3fn cast, the power-of-two
scale choice, the precision_config key, and the C ABI's two FP8-cache entry points (include/indextts_hip.h)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALES = (2.0 ** -4, 1.0, 2.0 ** 3)


def torch_cast(x, s):
    """The specification: torch's cast of the clamped, scaled value (x / s exact: s is a power of two and x an fp32 value)."""
    return (x.double() / s).clamp(-448.0, 448.0).to(torch.float32).to(torch.float8_e4m3fn).view(torch.uint8)


def probes(s):
    from indextts.utils import quant
    grid = quant.decode_e4m3(torch.arange(127, dtype=torch.uint8))                   # every non-negative finite value, ascending
    mid = (grid[:-1] + grid[1:]) / 2                                                  # every midpoint between adjacent codes (exact in fp32)
    sub = grid[:9]                                                                    # zero, the 7 subnormals, the smallest normal
    edge = torch.tensor([448.0, 449.0, 464.0, 480.0, 1e6 / s, 0.0, 2.0 ** -10, 2.0 ** -11, 3 * 2.0 ** -11], dtype=torch.float64)
    pos = torch.cat([grid, mid, sub, edge, mid * (1 + 2.0 ** -20), mid * (1 - 2.0 ** -20)])
    x = torch.cat([pos, -pos]) * s
    x = torch.cat([x, torch.tensor([1e6, -1e6, float("inf"), -float("inf"), -0.0], dtype=torch.float64)])
    return x.to(torch.float32)


@pytest.mark.parametrize("s", SCALES)
def test_quantize_kv_equals_the_torch_cast_bit_for_bit(s):
    from indextts.utils import quant
    g = torch.Generator().manual_seed(11)
    x = torch.cat([torch.randn(100_000, generator=g) * 3.0 * s, torch.randn(20_000, generator=g) * 200.0 * s, probes(s)])
    got, want = quant.quantize_kv_e4m3(x, s), torch_cast(x, s)
    assert got.dtype == torch.uint8 and got.shape == x.shape
    bad = (got != want).nonzero().flatten()
    assert bad.numel() == 0, f"scale {s}: x={x[bad[:4]].tolist()} got {got[bad[:4]].tolist()} want {want[bad[:4]].tolist()}"
    assert not ((got & 0x7F) == 0x7F).any(), "a NaN code (0x7f / 0xff) was produced"
    # saturation, not overflow: everything at or beyond +-448 s is the largest finite code
    assert (quant.quantize_kv_e4m3(torch.tensor([448.0 * s, 449.0 * s, 1e6, float("inf")]), s) == 0x7E).all()
    assert (quant.quantize_kv_e4m3(torch.tensor([-448.0 * s, -449.0 * s, -1e6, -float("inf")]), s) == 0xFE).all()
    # 16-bit inputs (what the cache holds before quantisation) and a broadcast scale
    for dt in (torch.bfloat16, torch.float16):
        xt = (torch.randn(4, 3, 64, generator=g) * 2.0).to(dt)
        sc = torch.tensor([s, 2 * s, s / 2])[None, :, None]
        want = (xt.double() / sc.double()).clamp(-448, 448).float().to(torch.float8_e4m3fn).view(torch.uint8)
        assert torch.equal(quant.quantize_kv_e4m3(xt, sc), want)
        assert torch.equal(quant.dequantize_kv(want, sc), quant.decode_e4m3(want) * sc.double())


def test_scales_from_amax():
    from indextts.utils import quant
    g = torch.Generator().manual_seed(5)
    amax = torch.cat([torch.rand(500, generator=g) * 40.0, 10.0 ** (torch.rand(500, generator=g) * 12 - 6),
                      torch.tensor([224.0, 112.0, 7.0, 3.5, 448.0, 1.0, 2.0 ** -20, 223.99, 224.01])])
    s = quant.kv_scales_from_amax(amax)
    assert s.dtype == torch.float32 and s.shape == amax.shape and bool(quant.is_pow2(s).all())
    a, sd = amax.double(), s.double()
    assert bool((2 * a / sd <= 448).all()) and bool((448 < 2 * a / (sd / 2)).all())      # the smallest such power of two
    assert quant.kv_scales_from_amax(torch.zeros(3)).tolist() == [1.0, 1.0, 1.0]
    assert quant.kv_scales_from_amax(torch.tensor([224.0, 224.0 * 1.0000001])).tolist() == [1.0, 2.0]
    assert quant.kv_scales_from_amax(torch.tensor([7.0]), headroom=1.0).item() == 2.0 ** -6
    # quantising the calibration data itself saturates nothing (a condition: headroom >= 1 keeps amax / s <= 448 / headroom)
    x = torch.randn(6, 4, 50, 64, generator=g) * (10.0 ** (torch.rand(6, 4, 1, 1, generator=g) * 4 - 2))
    sc = quant.kv_scales_from_amax(x.abs().amax(dim=(2, 3)))[:, :, None, None]
    codes = quant.quantize_kv_e4m3(x, sc)
    assert int(((codes & 0x7F) == 0x7E).sum()) == 0
    assert not quant.is_pow2(torch.tensor([0.0, -1.0, 3.0, float("inf"), float("nan"), 0.75])).any()
    assert quant.is_pow2(torch.tensor([1.0, 0.5, 2.0 ** -30, 2.0 ** 40])).all()


def test_precision_config_key():
    from indextts import infer
    assert infer._resolve_kv_cache("fp8") == "fp8"
    assert infer._resolve_kv_cache("auto") is None and infer._resolve_kv_cache(None) is None
    assert infer._resolve_kv_cache({"gpt": "bf16"}.get("kv_cache", "auto")) is None          # an absent key
    for wrong in ("int8", "bf16", "e4m3", ""):
        with pytest.raises(ValueError, match="kv_cache"):
            infer._resolve_kv_cache(wrong)


def test_engine_refuses_without_a_gpu_what_it_can():
    from indextts.gpt.engine import GPTEngine
    with pytest.raises(ValueError, match="kv_dtype"):
        GPTEngine({}, 1, 64, 1, kv_dtype="int8")


def test_abi_declares_and_exports_the_kv8_entry_points():
    from indextts import _native as nat
    L = nat.lib()
    assert L.itts_abi_version() == 10
    main = open(os.path.join(ROOT, "include", "indextts_hip.h")).read()
    assert re.search(r"#define ITTS_ABI_VERSION (\d+)", main).group(1) == "10"
    declared = set(re.findall(r"\b(itts_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", main, flags=re.S)))
    # the registry rule (EXPORTED_SYMBOLS is held against the header's prototypes by test_native_abi.py and against the dtype
    # table of test_host_launch_cpu.py): declared, exported, bound
    plain = ctypes.CDLL(nat.LIB_PATH)
    assert all(s_ in declared and hasattr(plain, s_) and s_ in nat.EXPORTED_SYMBOLS for s_ in ("itts_attn_decode_kv8", "itts_kv8_store"))


def test_entry_points_refuse_bad_calls_without_launching():
    from indextts import _native as nat
    L = nat.lib()
    P = 0x1000                                   # never dereferenced: every call below is refused before a launch
    dec = lambda **kw: L.itts_attn_decode_kv8(*[kw.get(k, d) for k, d in (  # noqa: E731
        ("qkv", P), ("kc", P), ("vc", P), ("out", P), ("pad", P), ("pos", P), ("sc", P), ("B", 2), ("H", 2), ("dtype", nat.BF16),
        ("packed", 0), ("skip", None), ("tab", P), ("bs", 16), ("stream", None))])
    sto = lambda **kw: L.itts_kv8_store(*[kw.get(k, d) for k, d in (  # noqa: E731
        ("qkv", P), ("kc", P), ("vc", P), ("sc", P), ("pad", None), ("row_off", None), ("shift", None), ("B", 2), ("S", 8), ("H", 2),
        ("dtype", nat.BF16), ("tab", P), ("bs", 16), ("stream", None))])
    for fn, name, ptrs in ((dec, b"itts_attn_decode_kv8", ("qkv", "kc", "vc", "out", "pad", "pos", "sc", "tab")),
                           (sto, b"itts_kv8_store", ("qkv", "kc", "vc", "sc", "tab"))):
        for p in ptrs:
            assert fn(**{p: None}) == 1 and name + b": null pointer" in L.itts_last_error(), p
        for bs in (0, 8, 24, 128):
            assert fn(bs=bs) == 1 and name in L.itts_last_error() and b"kv_bs" in L.itts_last_error()
        assert fn(dtype=nat.F32) == 1 and name in L.itts_last_error() and b"bf16 / f16" in L.itts_last_error()
        assert fn(dtype=7) == 1 and name in L.itts_last_error() and b"dtype" in L.itts_last_error()
        assert fn(B=0) == 1 and b"bad shape" in L.itts_last_error()
