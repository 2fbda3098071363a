"""The algorithm of voice extraction (indextts/gpt/voice_extract.py) in float64 torch on the CPU, over an
EXPLICIT difference matrix: the yardstick of tests/test_voice_extract_cpu.py and tests/test_voice_extract_gpu.py.  Written on its
own (nothing of the module is called), plus the synthetic checkpoints the CPU tests share."""
import torch

import refill_voices


def orth(y):
    return torch.linalg.qr(y, mode="reduced")[0]


def extract_ref(delta, max_rank=16, gap=8.0, omega=None, seed=0, index=0):
    """delta float64 [K, N] -> (A [r, K], B [N, r], dict(r, sigma_r, sigma_next, ratio, q: the basis Q [K, c])) in float64; ValueError where the module
    refuses.  omega: the probe [N, c] (default: drawn as the module draws it for target number `index`)."""
    delta = delta.double()
    K, N = delta.shape
    c = 16 * ((max_rank + 15) // 16) + 16
    if omega is None:
        g = torch.Generator().manual_seed(seed * 1000003 + index)
        omega = torch.randn(N, c, generator=g, dtype=torch.float32)
    q = orth(delta @ omega.double())
    q = orth(delta.t() @ q)
    q = orth(delta @ q)
    bt = delta.t() @ q
    u, s, vh = torch.linalg.svd(bt.t(), full_matrices=False)
    ratios = s[:-1] / s[1:]
    i = int(torch.argmax(ratios))
    r, ratio = i + 1, float(ratios[i])
    if ratio < gap or r > max_rank:
        raise ValueError(f"not low-rank: ratio {ratio:.3g} at rank {r}")
    root = s[:r].sqrt()
    return ((q @ u[:, :r]) * root).t(), vh[:r].t() * root, dict(r=r, sigma_r=float(s[r - 1]), sigma_next=float(s[r]), ratio=ratio, q=q)


def fp64_project(key, wb, wt):
    """make_project of voice_extract.extract over the explicit float64 difference (CPU)."""
    delta = wt.double() - wb.double()

    def project(x, trans):
        return (delta.t() if trans else delta) @ x.double()
    return project


# ------------------------------------------------------------------------------------------------ synthetic checkpoints (CPU)
SHAPES = {"attn.c_attn": (128, 384), "attn.c_proj": (128, 128), "mlp.c_fc": (128, 512), "mlp.c_proj": (512, 128)}


def small_base(layers=1, seed=5):
    """A state dict with the four targets of every layer (entries 0.02 N(0,1) rounded to fp16, held in fp16), their biases and
    one tensor outside the targets."""
    g = torch.Generator().manual_seed(seed)
    sd = {"mel_embedding.weight": (torch.randn(64, 128, generator=g) * 0.02).half()}
    for i in range(layers):
        for name, (k, n) in SHAPES.items():
            sd[f"gpt.h.{i}.{name}.weight"] = (torch.randn(k, n, generator=g) * 0.02).half()
            sd[f"gpt.h.{i}.{name}.bias"] = torch.zeros(n, dtype=torch.float16)
    return sd


def merged_checkpoint(sd, rank, scaling, save_dtype, layers=1, seed=3):
    """(the merged checkpoint stored in save_dtype the way train.py stores it, {target: true difference s A^T B^T in float64})."""
    (ad, sc), = refill_voices.make_factors(sd, (rank,), (scaling,), layers=layers, seed=seed)
    ms = refill_voices.merged_state(sd, [(ad, sc)], {0: 1.0})
    true = {k: (A.double().t() @ B.double().t()) * sc for k, (A, B) in ad.items()}
    return {k: v.to(save_dtype) for k, v in ms.items()}, true
