"""The yardstick of voice fitting: a float64 torch-autograd restatement, written on its own, of the adapted
GPT (y = x W + b + (drop(x) A^T) B^T alpha / r on the four Conv1D targets of every block), the reference's loss
(text_weight loss_text + (1 - text_weight) loss_mel with UnifiedVoice.forward's padding and alignment, model.py:565-604), LoRA+ AdamW
(two groups, decoupled decay), global-norm clipping and the cosine schedule with warm-up; and the bounds the kernel tests hold
libindextts_fit.so to.  Shared by tests/test_fit_*.py; nothing here calls the library or indextts/gpt/fit.py's trainer.

`peft` is not importable where this was written, so no fixture of the reference's own trainer exists (tests/golden/fit_small.npz is
not recorded).  The restatement is anchored instead on tests/golden/score_small.npz -- with B = 0 its losses must be the
reference's loss_text_64 / loss_mel_64 -- and on torch.optim.AdamW with two parameter groups (tests/test_fit_cpu.py).

BOUNDS.
ittf_lora_wgrad:  (M + 2) 2^-24 sum_m |s z| |scale| per entry (+ one rounding of the old G when accumulating): M exact-or-once-rounded
    products summed in fp32 in any order, one multiplication by scale, one addition.
ittf_sqnorm:  (n + 2) 2^-24 sum g^2: n products and additions in fp32 in any order.
ittf_adamw_step, per element, U = 2^-24, from the operations of one update in the header's order, each rounded once:
    p1 = p (1 - lr wd): the host's factor is rounded (U) and the product (U): 2 U |p|
    m' = m + (g' - m) b1c: g' = clip g (U), the difference (U), the product with a rounded 1 - beta1 (2 U), the sum (U):
         dm <= U (|m'| + 4 |g' - m| b1c + |g'| b1c)
    v' = v beta2 + g'^2 b2c: dv <= U (|v| beta2 + 5 g'^2 b2c + v')            (g' twice, b2c, two products, the sum)
    step = lr / bc1 (2 U relative, the host's), denom = sqrt(v') / bc2s + eps: relative error of sqrt(v') is dv / (2 v') + U, of the
         quotient one more U plus the host's rounding of bc2s (U), the sum U: d(denom) <= denom U + sqrt(v') / bc2s (dv / (2 v') + 3 U)
    q = m' / denom: dq <= |q| (dm / |m'| + d(denom) / denom + U);   p' = p1 - step q: dp <= 2 U |p| + step (dq + 3 U |q|) + U |p'|
    ADAM_MARGIN = 2 covers what the count leaves to first order.  The T copy is p' (the device's own fp32 bits) rounded once to T:
    compared EXACTLY against the device's master, not against float64.
"""
import math
import os

import numpy as np
import torch
import torch.nn.functional as F

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "score_small.npz")
TARGETS = ("attn.c_attn", "attn.c_proj", "mlp.c_fc", "mlp.c_proj")
U = 2.0 ** -24
ADAM_MARGIN = 2.0
START_TEXT, STOP_TEXT, START_MEL, STOP_MEL = 0, 1, 8192, 8193
# the overfit set (three ragged utterances of the fixture, 9 / 4 / 6 codes) and the budget under which the float64 trajectory alone
# more than halves loss_mel (9.2041 -> 2.1910 on the ragged batch; tests/test_fit_cpu.py asserts it): what the device test then asks
OVERFIT = dict(rank=4, alpha=8.0, lr=1e-3, steps=24, warmup_ratio=0.1, text_weight=0.1, max_grad_norm=1.0, weight_decay=0.01)


def fixture():
    return np.load(FIXTURE)


# ----------------------------------------------------------------------------------------------------------- kernel references
def wgrad64(s, z, M, r, C, scale=1.0, G0=None):
    """(G, bound) of ittf_lora_wgrad in float64 on the kernel's own operands (any float tensors, rows < M, columns < r / < C)."""
    s64, z64 = s[:M, :r].double().cpu(), z[:M, :C].double().cpu()
    G = float(scale) * (s64.t() @ z64)
    mag = abs(float(scale)) * (s64.abs().t() @ z64.abs())
    bound = (M + 2) * U * mag
    if G0 is not None:
        G = G + G0.double().cpu()
        bound = bound + U * G.abs()
    return G, bound


def adamw64(p, g, m, v, lr, wd, t, clip=1.0, beta1=0.9, beta2=0.999, eps=1e-8):
    """One update of the header's AdamW in float64 -> (p', m', v', bound on |p' - device p'|, bound on m', bound on v')."""
    p, g, m, v = (x.double().cpu() for x in (p, g, m, v))
    g1 = clip * g
    b1c, b2c = 1.0 - beta1, 1.0 - beta2
    bc1, bc2s = 1.0 - beta1 ** t, math.sqrt(1.0 - beta2 ** t)
    p1 = p * (1.0 - lr * wd)
    m1 = m + (g1 - m) * b1c
    v1 = v * beta2 + g1 * g1 * b2c
    step = lr / bc1
    root = v1.sqrt() / bc2s
    denom = root + eps
    q = m1 / denom
    p2 = p1 - step * q
    dm = U * (m1.abs() + 4 * (g1 - m).abs() * b1c + g1.abs() * b1c)
    dv = U * (v.abs() * beta2 + 5 * g1 * g1 * b2c + v1)
    dden = denom * U + root * (dv / (2 * v1).clamp_min(1e-300) + 3 * U)
    dq = dm / denom + q.abs() * (dden / denom + U)
    dp = 2 * U * p.abs() + step * (dq + 3 * U * q.abs()) + U * p2.abs()
    tiny = 2.0 ** -126                                        # (one subnormal step: a result next to zero)
    return p2, m1, v1, ADAM_MARGIN * dp + tiny, ADAM_MARGIN * dm + tiny, ADAM_MARGIN * dv + tiny


def cosine_with_warmup(step, warmup, total):
    """get_cosine_schedule_with_warmup's lambda (num_cycles = 0.5), restated."""
    if step < warmup:
        return step / max(1, warmup)
    progress = (step - warmup) / max(1, total - warmup)
    return max(0.0, 0.5 * (1.0 + math.cos(math.pi * progress)))


# ----------------------------------------------------------------------------------------------------------- the adapted model
def conds64(sd, cond_mel):
    """The conditioning latents [1, 32, D] of a prompt mel [1, 100, T] in float64 on the CPU: the project's functional conditioner
    (frozen in a fit; the fp32 model runs the same functions)."""
    from indextts.gpt.conformer_encoder import conformer_encode
    from indextts.gpt.perceiver import perceiver_resample
    W = {k: v.detach().cpu().double() for k, v in sd.items()
         if k.startswith(("conditioning_encoder.", "perceiver_encoder.")) and not k.endswith("pos_enc.pe")}
    x, _ = conformer_encode(W, cond_mel.detach().cpu().double().transpose(1, 2), None, heads=8)
    return perceiver_resample(W, x, None, heads=8)


def init_factors(sd, layers, r, seed, targets=TARGETS):
    """peft's initialisation in the trainer's draw order: per block and target A [r, in] uniform in +- 1 / sqrt(in) from one CPU
    generator, B [out, r] zero."""
    gen = torch.Generator().manual_seed(seed)
    out = {}
    for i in range(layers):
        for name in TARGETS:
            if name not in targets:
                continue
            K, N = sd[f"gpt.h.{i}.{name}.weight"].shape
            A = (torch.rand(r, K, generator=gen, dtype=torch.float32) * 2.0 - 1.0) * (1.0 / math.sqrt(K))
            out[f"gpt.h.{i}.{name}"] = (A, torch.zeros(N, r))
    return out


def aligned(tokens, lengths, stop):
    ar = torch.arange(tokens.shape[1])[None]
    return F.pad(torch.where(ar < lengths.reshape(-1, 1), tokens, torch.full_like(tokens, stop)), (0, 2), value=stop)


class Model:
    """The adapted GPT over a state dict, in `dtype` on the CPU.  factors: {key: (A, B)} leaf tensors that may require grad."""

    def __init__(self, sd, layers, dtype=torch.float64, heads=20):
        self.sd = {k: v.detach().cpu().to(dtype) for k, v in sd.items() if v.is_floating_point() and not k.startswith(("conditioning_encoder.", "perceiver_encoder."))}
        self.layers, self.heads, self.dtype = layers, heads, dtype

    def linear(self, x, key, factors, scaling, masks):
        W, b = self.sd[key + ".weight"], self.sd[key + ".bias"]
        y = x @ W + b
        if factors is not None and key in factors:
            A, B = factors[key]
            xd = x if masks is None or key not in masks else x * masks[key]
            y = y + (xd @ A.t()) @ B.t() * scaling
        return y

    def losses(self, conds, text, text_lengths, codes, wav_lengths, factors=None, scaling=1.0, masks=None):
        """-> dict(loss_text, loss_mel, text_nll [B, L + 2], mel_nll [B, T + 2]) as UnifiedVoice.forward computes them."""
        sd, dt, H = self.sd, self.dtype, self.heads
        text, codes = text.long(), codes.long()
        ml = torch.ceil(wav_lengths.double() / 1024).long() + 1
        tt, mt = aligned(text, text_lengths.long(), STOP_TEXT), aligned(codes, ml, STOP_MEL)
        ti, mi = F.pad(tt[:, :-1], (1, 0), value=START_TEXT), F.pad(mt[:, :-1], (1, 0), value=START_MEL)
        te = sd["text_embedding.weight"][ti] + sd["text_pos_embedding.emb.weight"][: ti.shape[1]]
        me = sd["mel_embedding.weight"][mi] + sd["mel_pos_embedding.emb.weight"][: mi.shape[1]]
        B = text.shape[0]
        c = conds.to(dt)
        h = torch.cat([c.expand(B, -1, -1) if c.shape[0] == 1 else c, te, me], dim=1)
        S, D = h.shape[1], h.shape[2]
        causal = torch.ones(S, S, dtype=torch.bool).tril()
        for i in range(self.layers):
            p = f"gpt.h.{i}."
            x = F.layer_norm(h, (D,), sd[p + "ln_1.weight"], sd[p + "ln_1.bias"], 1e-5)
            q, k, v = self.linear(x, p + "attn.c_attn", factors, scaling, masks).view(B, S, 3, H, D // H).permute(2, 0, 3, 1, 4)
            w = (q @ k.transpose(-1, -2)) / math.sqrt(D // H)
            a = torch.softmax(w.masked_fill(~causal, float("-inf")), dim=-1) @ v
            h = h + self.linear(a.permute(0, 2, 1, 3).reshape(B, S, D), p + "attn.c_proj", factors, scaling, masks)
            x = F.layer_norm(h, (D,), sd[p + "ln_2.weight"], sd[p + "ln_2.bias"], 1e-5)
            f = self.linear(x, p + "mlp.c_fc", factors, scaling, masks)
            f = 0.5 * f * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (f + 0.044715 * f ** 3)))          # gelu_new
            h = h + self.linear(f, p + "mlp.c_proj", factors, scaling, masks)
        h = F.layer_norm(h, (D,), sd["gpt.ln_f.weight"], sd["gpt.ln_f.bias"], 1e-5)
        enc = F.layer_norm(h, (D,), sd["final_norm.weight"], sd["final_norm.bias"], 1e-5)[:, c.shape[1]:]
        out = {}
        for name, rows, tgt in (("text", enc[:, : tt.shape[1]], tt), ("mel", enc[:, -mt.shape[1]:], mt)):
            logits = rows @ sd[f"{name}_head.weight"].t() + sd[f"{name}_head.bias"]
            nll = F.cross_entropy(logits.reshape(-1, logits.shape[-1]), tgt.reshape(-1), reduction="none").view(B, -1)
            out[f"{name}_nll"], out[f"loss_{name}"] = nll, nll.mean()
        return out


def batch_losses(model, batch, factors=None, scaling=1.0, masks=None):
    """Model.losses of a padded batch (the tuple of its arguments), or of a ragged one -- dict(conds, text_rows, code_rows): every
    utterance alone, as a batch of one, and per head the mean over all utterances' positions."""
    if not isinstance(batch, dict):
        return model.losses(*batch, factors=factors, scaling=scaling, masks=masks)
    conds, parts = batch["conds"].detach().cpu(), []
    for i, (t, c) in enumerate(zip(batch["text_rows"], batch["code_rows"])):
        ci = conds if conds.shape[0] == 1 else conds[i: i + 1]
        parts.append(model.losses(ci, t.reshape(1, -1), torch.tensor([t.numel()]), c.reshape(1, -1), torch.tensor([c.numel() * 1024]),
                                  factors=factors, scaling=scaling, masks=masks))
    out = {}
    for name in ("text", "mel"):
        out[f"{name}_nll"] = [p[f"{name}_nll"][0] for p in parts]
        out[f"loss_{name}"] = torch.cat(out[f"{name}_nll"]).mean()
    return out


def leaves(factors, dtype=torch.float64, requires_grad=True):
    return {k: tuple(t.detach().cpu().to(dtype).clone().requires_grad_(requires_grad) for t in ab) for k, ab in factors.items()}


def loss_and_grads(model, batch, factors, scaling, text_weight, masks=None):
    """(losses, {key: (dA, dB)}) of text_weight loss_text + (1 - text_weight) loss_mel at `factors` (made leaves here)."""
    fl = leaves(factors, model.dtype)
    with torch.enable_grad():                          # (a module imported earlier in the process may have turned grad off)
        o = batch_losses(model, batch, factors=fl, scaling=scaling, masks=masks)
        (text_weight * o["loss_text"] + (1.0 - text_weight) * o["loss_mel"]).backward()
    return o, {k: (a.grad.clone(), b.grad.clone()) for k, (a, b) in fl.items()}


class Trainer:
    """The reference's optimisation loop restated in `dtype`: LoRA+ AdamW (group 0: every A at lr, group 1: every B at lr ratio, both
    decayed, decoupled), clip_grad_norm_ (factor min(1, max_norm / (norm + 1e-6))), the cosine schedule, gradient accumulation."""

    def __init__(self, model, factors, scaling, lr, ratio=2.0, wd=0.01, text_weight=0.1, max_norm=1.0, total_steps=100, warmup_ratio=0.1,
                 beta1=0.9, beta2=0.999, eps=1e-8):
        self.model, self.scaling, self.tw = model, scaling, text_weight
        self.f = leaves(factors, torch.float64 if model is None else model.dtype, requires_grad=False)
        self.m = {k: tuple(torch.zeros_like(t) for t in ab) for k, ab in self.f.items()}
        self.v = {k: tuple(torch.zeros_like(t) for t in ab) for k, ab in self.f.items()}
        self.lr, self.ratio, self.wd, self.max_norm = lr, ratio, wd, max_norm
        self.total, self.warm = total_steps, int(total_steps * warmup_ratio)
        self.b1, self.b2, self.eps, self.t = beta1, beta2, eps, 0

    def step(self, batches):
        batches = batches if isinstance(batches, list) else [batches]
        grads, rep = None, dict(loss_text=0.0, loss_mel=0.0)
        for b in batches:
            o, g = loss_and_grads(self.model, b, self.f, self.scaling, self.tw)
            grads = g if grads is None else {k: (grads[k][0] + g[k][0], grads[k][1] + g[k][1]) for k in g}
            rep["loss_text"] += float(o["loss_text"].detach()) / len(batches)
            rep["loss_mel"] += float(o["loss_mel"].detach()) / len(batches)
        grads = {k: (a / len(batches), b / len(batches)) for k, (a, b) in grads.items()}
        rep.update(self.apply(grads), grads=grads)
        return rep

    def apply(self, grads):
        """Clip, schedule and update from the (averaged) gradients {key: (dA, dB)} -> dict(grad_norm, lr)."""
        norm = math.sqrt(sum(float((t.double() ** 2).sum()) for ab in grads.values() for t in ab))
        clip = 1.0 if self.max_norm is None else min(1.0, self.max_norm / (norm + 1e-6))
        lr = self.lr * cosine_with_warmup(self.t, self.warm, self.total)
        self.t += 1
        bc1, bc2s = 1.0 - self.b1 ** self.t, math.sqrt(1.0 - self.b2 ** self.t)
        for k in self.f:
            for j, group_lr in ((0, lr), (1, lr * self.ratio)):
                p, g = self.f[k][j], grads[k][j] * clip
                p.mul_(1.0 - group_lr * self.wd)
                self.m[k][j].add_((g - self.m[k][j]) * (1.0 - self.b1))
                self.v[k][j].mul_(self.b2).add_(g * g * (1.0 - self.b2))
                p.sub_((group_lr / bc1) * self.m[k][j] / (self.v[k][j].sqrt() / bc2s + self.eps))
        return dict(grad_norm=norm, lr=lr)
