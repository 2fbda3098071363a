#!/usr/bin/env python3
"""Voice fitting measured: ONE optimizer step of FitEngine at the real shape -- 24 layers, D = 1280, 8
utterances of ~500 rows (32 latents, 60 text tokens, ~400 codes; lengths differ by a few rows so that the rectangle has padding), bf16
and fp32, r = 4 and r = 16, synthetic weights -- in ONE process with two arms alternating round by round:
  (fit)    the step as IndexTTS.fit_voice runs it: every block GEMM nat.gemm_conv (split-K slabs summed by itts_rows);
  (linear) the same autograd graph with torch.nn.functional.linear over dense copies in the place of the FROZEN GEMMs (x W and
           dy W^T); the small LoRA products, ittf_lora_wgrad and the optimizer stay.
Each step between two device events, median of 5 after one warm-up round.  The (fit) step is split by device events around every
native call: the frozen GEMMs forward and backward (with their slab sums), the small LoRA products, ittf_lora_wgrad, the optimizer
(ittf_sqnorm, ittf_adamw_step and the pack_weight launches of _refresh); the two heads with their cross-entropy, forward and
backward, are timed on their own over the step's row count; what is left of the step is the torch plumbing (LayerNorm, GELU, the
attention, the residual adds, autograd's own work).  Also reported: the peak bytes a step allocates, and the padding rows computed.
The blocks' causal attention is a category of its own, forward and backward: device events around FitEngine._attention, and for its
backward an event when the gradient of its output arrives and one when the gradient of qkv is complete (tensor hooks: the same for
the torch loop and for the HIP kernels).  --attention torch | hip chooses the arm the step runs (default: torch, the loop);
--attention both alternates the two arms in the place of (fit) / (linear), at r = 4, with two FitEngines over the one GPTEngine, and
reports per arm the step, the attention and the peak bytes beside the analytic difference of the saved tensors (DESIGN.md
section 4.30).
No speed is promised: the output is the record.  Writes profiles/fit_bench.txt.
usage: bench_fit.py [--out FILE] [--layers N] [--attention torch|hip|both]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "index-tts-lora_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import synth  # noqa: E402
import weights  # noqa: E402
from indextts import _native as nat  # noqa: E402
from indextts import _native_fit as nf  # noqa: E402
from indextts.gpt import fit  # noqa: E402
from indextts.gpt.engine import GPTEngine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fit_bench.txt"))
ap.add_argument("--layers", type=int, default=24)
ap.add_argument("--attention", default="torch", choices=("torch", "hip", "both"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_fit.py measures on the GPU: none is visible")
DEV, REPS, WARM = torch.device("cuda:0"), 5, 1
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def med(v):
    return f"{statistics.median(v):8.2f} [{min(v):.2f} .. {max(v):.2f}]"


class Clock:
    """Device events around calls, summed per category after a synchronise."""

    def __init__(self):
        self.pairs, self.on, self.phase = [], False, "fwd"

    def wrap(self, fn, cat):
        def inner(*a, **k):
            if not self.on:
                return fn(*a, **k)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*a, **k)
            e1.record()
            self.pairs.append((cat(self) if callable(cat) else cat, e0, e1))
            return out
        return inner

    def totals(self):
        torch.cuda.synchronize()
        t = {}
        for cat, e0, e1 in self.pairs:
            t[cat] = t.get(cat, 0.0) + e0.elapsed_time(e1)
        self.pairs = []
        return t


clock = Clock()
orig_mm, orig_fwd, orig_bwd = fit._mm, fit._Gemm.forward, fit._Gemm.backward
dense = {}          # data_ptr of a frozen packed weight -> its dense [N, K] copy (F.linear's layout), the (linear) arm's operands
use_linear = False


def mm(T, x, wp, K, N):
    w = dense.get(wp.data_ptr()) if use_linear and min(K, N) > 128 else None      # (the frozen weights only)
    if w is not None:
        return F.linear(x, w).to(torch.float32)
    return orig_mm(T, x, wp, K, N)


def phased(fn, name):
    def inner(*a, **k):
        clock.phase = name
        return fn(*a, **k)
    return inner


fit._mm = clock.wrap(mm, lambda c: "frozen GEMMs " + c.phase if c.big else "LoRA products")
fit._Gemm.forward = staticmethod(phased(orig_fwd, "forward"))
fit._Gemm.backward = staticmethod(phased(orig_bwd, "backward"))
clock.big = True
_mm_timed = fit._mm


def mm_sized(T, x, wp, K, N):
    clock.big = min(K, N) > 128
    return _mm_timed(T, x, wp, K, N)


fit._mm = mm_sized
_gemm_conv = nat.gemm_conv
nat.gemm_conv = clock.wrap(_gemm_conv, lambda c: "LoRA products" if c.in_small else None)
clock.in_small = True          # every nat.gemm_conv that fit.py calls OUTSIDE _mm is a small LoRA product ...
_orig_mm_inner = orig_mm


def orig_mm_quiet(T, x, wp, K, N):        # ... and inside _mm the call is already inside _mm's own pair
    clock.in_small = False
    try:
        return _orig_mm_inner(T, x, wp, K, N)
    finally:
        clock.in_small = True


orig_mm = orig_mm_quiet
nf.lora_wgrad = clock.wrap(nf.lora_wgrad, "ittf_lora_wgrad")
nf.sqnorm = clock.wrap(nf.sqnorm, "optimizer")
nf.adamw_step = clock.wrap(nf.adamw_step, "optimizer")
fit.FitEngine._refresh = clock.wrap(fit.FitEngine._refresh, "optimizer")

_attention = fit.FitEngine._attention


def attention_timed(self, qkv, lens, S, causal, rows):
    if not clock.on:
        return _attention(self, qkv, lens, S, causal, rows)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    ev[0].record()
    out = _attention(self, qkv, lens, S, causal, rows)
    ev[1].record()
    clock.pairs.append(("attention forward", ev[0], ev[1]))
    if out.requires_grad:
        out.register_hook(lambda g: ev[2].record())     # the gradient of the attention's output arrives: its backward starts
        qkv.register_hook(lambda g: ev[3].record())     # the gradient of qkv is complete: it has ended
        clock.pairs.append(("attention backward", ev[2], ev[3]))
    return out


fit.FitEngine._attention = attention_timed
BOTH = args.attention == "both"
ARMS = ("torch", "hip") if BOTH else ("fit", "linear")

say(f"voice fitting: one optimizer step, {args.layers} layers, D = 1280, 8 utterances; ms, median of {REPS} [min .. max]; arms alternating")
sd = dict(weights.gpt_state_dict(args.layers, with_conditioner=False))
sd.update({k: torch.from_numpy(v) for k, v in synth.fill_state_dict({"text_head.weight": (12001, 1280), "text_head.bias": (12001,)},
                                                                     synth.gpt_param).items()})
g = torch.Generator().manual_seed(29)
texts = [torch.randint(2, 12000, (60 - i,), generator=g) for i in range(8)]
codes = [torch.randint(0, 8192, (400 - 3 * i,), generator=g) for i in range(8)]
conds = torch.randn(1, 32, 1280, generator=g).to(DEV) * 0.5
for dtype in (torch.bfloat16, torch.float32):
    eng = GPTEngine(sd, args.layers, 1280, 20, dtype=dtype, device=DEV)
    dense.clear()
    for i, l in enumerate(eng.layers):
        for name, wkey in fit._WKEY.items():
            dense[l[wkey].data_ptr()] = sd[f"gpt.h.{i}.{name}.weight"].to(DEV, dtype).t().contiguous()
    for rank in ((4,) if BOTH else (4, 16)):
        for key in [k for k, v in dense.items() if v is None or getattr(v, "_of_fit", False)]:
            del dense[key]                                 # the transposed copies of the engine before: their addresses are free again
        fes = {a: fit.FitEngine(eng, sd, fit.FitConfig(rank=rank, alpha=2.0 * rank, dropout=0.0, lr=1e-4, attention=a))
               for a in (ARMS if BOTH else (args.attention,))}
        for fe in fes.values():
            for row in fe.targets:
                for tg in row.values():
                    dense[tg.wt.data_ptr()] = dense[tg.w.data_ptr()].t().contiguous()
                    dense[tg.wt.data_ptr()]._of_fit = True
        b = fe.batch(conds, texts, codes)
        real = sum(32 + t.numel() + 2 + c.numel() + 2 for t, c in zip(texts, codes))
        rect = 8 * max(32 + t.numel() + 2 + c.numel() + 2 for t, c in zip(texts, codes))
        times, parts, peak = {a: [] for a in ARMS}, {a: [] for a in ARMS}, {a: 0 for a in ARMS}
        for rnd in range(WARM + REPS):
            for arm in ARMS:
                fe = fes[arm] if BOTH else fes[args.attention]
                use_linear, clock.on = arm == "linear", arm != "linear" and rnd >= WARM
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                rep = fe.step(b)
                e1.record()
                torch.cuda.synchronize()
                if rnd >= WARM:
                    times[arm].append(e0.elapsed_time(e1))
                    if arm != "linear":
                        parts[arm].append(clock.totals())
                        peak[arm] = max(peak[arm], torch.cuda.max_memory_allocated() - base)
        clock.on = False
        # the two heads with their cross-entropy, forward and backward, on their own over the step's head rows
        n_t, n_m = sum(t.numel() + 2 for t in texts), sum(c.numel() + 2 for c in codes)
        heads = []
        for _ in range(WARM + REPS):
            x = torch.randn(n_t + n_m, 1280, device=DEV, requires_grad=True)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            with torch.enable_grad():
                loss = 0
                for name, rows in (("text", x[:n_t]), ("mel", x[n_t:])):
                    W, bias = fe.heads[name]
                    xr = rows if dtype == torch.float32 else rows.to(dtype).to(torch.float32)
                    loss = loss + F.cross_entropy(xr @ W.t() + bias, torch.zeros(rows.shape[0], dtype=torch.long, device=DEV))
                loss.backward()
            e1.record()
            torch.cuda.synchronize()
            heads.append(e0.elapsed_time(e1))
        heads = heads[WARM:]
        name = {torch.bfloat16: "bf16", torch.float32: "fp32"}[dtype]
        say(f"--- {name}, r = {rank}: {real} real rows in a rectangle of {rect} ({rect - real} padding rows computed); "
            f"loss_mel {rep['loss_mel']:.4f}")
        for arm in ARMS:
            if arm == "linear":
                say(f"  step, arm (linear: F.linear frozen)   {med(times['linear'])}")
                continue
            label = f'attention="{arm}"' if BOTH else f'fit, attention="{args.attention}"'
            say(f"  step, arm ({label}){'':<{max(0, 26 - len(label))}}{med(times[arm])}   peak bytes of a step {peak[arm] / 2 ** 20:.0f} MiB")
            tot = statistics.median(times[arm])
            left = tot
            for cat in ("frozen GEMMs forward", "frozen GEMMs backward", "LoRA products", "ittf_lora_wgrad", "optimizer", "attention forward",
                        "attention backward"):
                v = [p.get(cat, 0.0) for p in parts[arm]]
                left -= statistics.median(v)
                say(f"    {cat:<36s}{med(v)}   {100 * statistics.median(v) / tot:5.1f} %")
            left -= statistics.median(heads)
            say(f"    {'heads + cross-entropy (on their own)':<36s}{med(heads)}   {100 * statistics.median(heads) / tot:5.1f} %")
            say(f"    {'plumbing (the rest of the step)':<36s}{left:8.2f}                      {100 * left / tot:5.1f} %")
        if BOTH:
            t, h = times["torch"], times["hip"]
            spread, gain = max(t) - min(t), statistics.median(t) - statistics.median(h)
            lens = [32 + x.numel() + 2 + c.numel() + 2 for x, c in zip(texts, codes)]
            saved = (4 * 20 * sum(n * n for n in lens) - 4 * 20 * rect) * args.layers     # (the hip arm keeps lse, not out)
            say(f"  median(torch) - median(hip) = {gain:.2f} ms against the torch arm's spread (max - min) of {spread:.2f} ms: "
                f"{'faster' if gain > spread else 'NOT faster by the rule'}")
            say(f"  peak bytes torch - hip = {(peak['torch'] - peak['hip']) / 2 ** 20:.0f} MiB; the saved tensors differ by "
                f"4 H sum n^2 L - 4 H M L = {saved / 2 ** 20:.0f} MiB: peak memory is {'lower' if peak['hip'] < peak['torch'] else 'NOT lower'} under hip")
        del fe, fes
    del eng
    torch.cuda.empty_cache()
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
