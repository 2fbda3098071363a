"""Weight-only FP8 quantisation for the decode-step GEMMs: OCP E4M3 ("e4m3fn") codes with one fp32 scale per output column.

    W[k, n] ~ scale[n] * decode(codes[k, n]),   scale[n] = max_k |W[k, n]| / 448   (1.0 for an all-zero column)

E4M3: 1 sign bit, 4 exponent bits (bias 7), 3 mantissa bits; subnormals m * 2^-9; largest finite value 448 (0x7e); 0x7f / 0xff are
NaN and are never produced here.  The rounding is round-to-nearest-even on the E4M3 grid, done on float64 values (one rounding: no
detour through fp32), and equals torch's float8_e4m3fn cast of the same values (tests/test_w8_cpu.py pins that).  Host code: the
engine quantises once at load time; the kernel side is include/indextts_hip.h."""
import torch

E4M3_MAX = 448.0


def _table():
    """The 127 non-negative finite E4M3 values by code (float64, ascending), and 480 in the NaN slot 0x7f for indexing only."""
    c = torch.arange(128, dtype=torch.float64)
    e, m = torch.floor(c / 8), c % 8
    return torch.where(e == 0, m * 2.0 ** -9, (1.0 + m / 8.0) * torch.pow(torch.tensor(2.0, dtype=torch.float64), e - 7.0))


def _e4m3_codes(x):
    """float64 values already clamped to [-448, 448] -> uint8 codes: round-to-nearest-even onto the E4M3 grid."""
    a = x.abs()
    _, ex = torch.frexp(a)                                              # a = f * 2^ex, f in [0.5, 1): the binade's exponent is ex - 1
    # grid spacing at a (subnormal spacing 2^-9 below 2^-6), looked up in a table made on the host: a device's ldexp / pow need not
    # be exact, and a spacing one ulp off moves q off the grid
    steps = torch.tensor([2.0 ** (e - 3) for e in range(-6, 9)], dtype=torch.float64).to(x.device)
    step = steps[(torch.clamp(ex - 1, min=-6, max=8) + 6).long()]
    q = torch.round(a / step) * step                                    # torch.round: half to even; exact in float64
    codes = torch.searchsorted(_table()[:127].to(x.device), q.contiguous())   # q is a grid value: its index is its code
    codes = codes + 128 * torch.signbit(x)                              # (a negative value below half the smallest subnormal: -0, as the cast gives)
    return codes.to(torch.uint8)


def quantize_e4m3_cols(w_kn):
    """w_kn [K, N] (fp32 / fp64, any device) -> (codes uint8 [K, N], scale fp32 [N])."""
    w = w_kn.detach().to(torch.float64)
    amax = w.abs().amax(0)
    scale = torch.where(amax > 0, amax / E4M3_MAX, torch.ones_like(amax)).to(torch.float32)
    scale = torch.where(scale > 0, scale, torch.ones_like(scale))       # a column whose maximum underflows fp32 / 448
    x = (w / scale.to(torch.float64)).clamp(-E4M3_MAX, E4M3_MAX)
    codes = _e4m3_codes(x)
    return codes, scale


def decode_e4m3(codes):
    """uint8 codes -> float64 values (scale 1)."""
    c = codes.to(torch.int64)
    v = _table().to(codes.device)[c & 127]
    return torch.where(c >= 128, -v, v)


def dequantize(codes, scale):
    """(codes uint8 [K, N], scale [N]) -> float64 [K, N] = scale * decode(codes)."""
    return decode_e4m3(codes) * scale.to(torch.float64)


def dequantized_gpt_weights(W, layers):
    """The 16-bit-servable model an FP8 engine (GPTEngine(weight_dtype="fp8")) computes with, as a state dict (fp32): every
    decode-step weight replaced by its dequantised values.  The QKV and FC projections are quantised with their LayerNorm's gamma
    folded in (gamma . W), so the equivalent block has a LayerNorm without affine (ones, zeros), the dequantised gamma . W as the
    weight and beta W + b as the bias; out-projection, FC2 and mel_head are quantised as they are.  Quantising this dict again gives
    the same codes: an FP8 engine built from it and a 16-bit engine built from it serve the same model."""
    out = {k: v.detach().clone() for k, v in W.items()}

    def deq(w_kn):
        return dequantize(*quantize_e4m3_cols(w_kn))
    for i in range(layers):
        p = f"gpt.h.{i}."
        for ln, proj in (("ln_1", "attn.c_attn"), ("ln_2", "mlp.c_fc")):
            g, bt = W[p + ln + ".weight"].double(), W[p + ln + ".bias"].double()
            Wm = W[p + proj + ".weight"].double()
            out[p + proj + ".weight"] = deq(g[:, None] * Wm).float()
            out[p + proj + ".bias"] = (bt @ Wm + W[p + proj + ".bias"].double()).float()
            out[p + ln + ".weight"], out[p + ln + ".bias"] = torch.ones_like(W[p + ln + ".weight"]), torch.zeros_like(W[p + ln + ".bias"])
        for proj in ("attn.c_proj", "mlp.c_proj"):
            out[p + proj + ".weight"] = deq(W[p + proj + ".weight"].double()).float()
    out["mel_head.weight"] = deq(W["mel_head.weight"].double().t()).t().contiguous().float()
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# FP8 KV cache (include/indextts_hip.h): the same E4M3 codes, one fp32 POWER-OF-TWO scale per (layer,
# K | V, head).  Multiplying by the inverse of a power of two is exact, so these host functions and the device quantiser
# (csrc/kv8.hip) give the same code for every input, and dequantisation commutes with every sum.
# ---------------------------------------------------------------------------------------------------------------------------------
def is_pow2(scale):
    """True where `scale` is a positive finite power of two (elementwise)."""
    s = torch.as_tensor(scale).detach().to(torch.float64)
    fr, _ = torch.frexp(s)
    return torch.isfinite(s) & (s > 0) & (fr == 0.5)


def quantize_kv_e4m3(x, scale):
    """x (any float dtype, finite or +-inf) and scale (power of two, broadcastable to x) -> uint8 codes of x's shape:
    clamp(x / scale, +-448), then round-to-nearest-even onto the E4M3 grid.  The clamp comes first: torch's cast and the
    hardware's conversion do not agree on what lies beyond 448, and nothing here rests on either rule; an outlier saturates to
    +-448 and stays finite.  0x7f / 0xff (NaN) are never produced.  Equals torch.float8_e4m3fn casting of the clamped value bit
    for bit (tests/test_kv8_cpu.py)."""
    s = torch.as_tensor(scale, device=x.device).to(torch.float64)
    return _e4m3_codes((x.detach().to(torch.float64) / s).clamp(-E4M3_MAX, E4M3_MAX))


def dequantize_kv(codes, scale):
    """codes uint8, scale broadcastable -> float64 = scale * decode(codes) (exact: every product is a float64 value)."""
    return decode_e4m3(codes) * torch.as_tensor(scale, device=codes.device).to(torch.float64)


def kv_scales_from_amax(amax, headroom=2.0):
    """amax (>= 0, any shape) -> fp32 scales of that shape: the smallest power of two s with headroom * amax / s <= 448; s = 1
    where amax == 0.  The headroom of 2 is a choice, not a measurement: positions generated later may exceed the calibration
    prompt's maximum, and what still exceeds the range saturates (quantize_kv_e4m3)."""
    a = torch.as_tensor(amax).detach().to(torch.float64) * float(headroom) / E4M3_MAX
    fr, ex = torch.frexp(a)                       # a = fr * 2^ex, fr in [0.5, 1): the smallest power of two >= a is 2^ex, or 2^(ex-1) at fr = 0.5
    e = torch.where(fr == 0.5, ex - 1, ex)
    s = torch.ldexp(torch.ones_like(a), e)
    return torch.where(a > 0, s, torch.ones_like(a)).to(torch.float32)
