#!/usr/bin/env python3
"""Likelihood scoring measured: R = 32 x 600 rows, D = 1280, V = 8194, bf16 and fp32, seeded operands, in
ONE process with the arms alternating round by round:
  (a) the materialised form on the device: a GEMM into an [R, V] fp32 buffer (16-bit operands, fp32 output where the framework
      has that GEMM), then log_softmax, gather and a rank count in torch;
  (b) ScoreEngine.score: one ittl_target_logit + one ittl_head_nll (+ its merge launch).
Each arm between two device events, median of 7 after two warm-up rounds; for (b) also every launch between two device events.
Reported: both times, the bytes each arm allocates (peak over the arm), TFLOP/s of the streamed launch, and the number of rows on
which any output differs between the arms beyond the bound of tests/score_refs.py (arm (a) standing where the float64 reference
stands there: its own error is inside the same bound).  No ratio is fixed in advance: the output is the record.
Writes profiles/score.txt.
usage: bench_score.py [--out FILE]"""
import argparse
import os
import statistics
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "index-tts-lora_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch  # noqa: E402

from indextts import _native_score as nl  # noqa: E402
from indextts.gpt.score import ScoreEngine  # noqa: E402

torch.set_grad_enabled(False)
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_score.py measures on the GPU: none is visible")
DEV, REPS, WARM = torch.device("cuda:0"), 7, 2
R, D, V = 32 * 600, 1280, 8194
lines = []
try:                        # a 16-bit GEMM that writes fp32, where the framework has one; else its 16-bit output is widened
    torch.mm(torch.zeros(8, 8, dtype=torch.bfloat16, device=DEV), torch.zeros(8, 8, dtype=torch.bfloat16, device=DEV), out_dtype=torch.float32)
    WIDE_OUT = True
except (TypeError, RuntimeError):
    WIDE_OUT = False


def say(s):
    print(s, flush=True)
    lines.append(s)


def med(v):
    return f"{statistics.median(v):.3f}  [{min(v):.3f} .. {max(v):.3f}]"


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), torch.cuda.max_memory_allocated() - base, out


g = torch.Generator().manual_seed(27)
x = torch.randn(R, D, generator=g).to(DEV)
y = torch.randint(0, V, (R,), generator=g).to(DEV)
sd = {"mel_head.weight": torch.randn(V, D, generator=g) * (4.0 / D ** 0.5), "mel_head.bias": torch.randn(V, generator=g),
      "text_head.weight": torch.zeros(8, D), "text_head.bias": torch.zeros(8)}
say(f"likelihood scoring: R = {R} rows, D = {D}, V = {V}; median of {REPS} [min .. max], ms; arms alternating in one process")
for dtype in (torch.bfloat16, torch.float32):
    se = ScoreEngine(SimpleNamespace(device=DEV, dtype=dtype, weight_dtype=None), sd)
    W, b = se.heads["mel"]
    Wv = W[:, :V].contiguous()

    def arm_a():
        if dtype == torch.float32:
            logits = torch.addmm(b, x, Wv)
        elif WIDE_OUT:
            logits = torch.mm(x.to(dtype), Wv, out_dtype=torch.float32) + b
        else:
            logits = (x.to(dtype) @ Wv).float() + b
        lp = torch.log_softmax(logits, dim=1)
        t = logits.gather(1, y[:, None])
        lpt = lp.gather(1, y[:, None])[:, 0]
        rank = (logits > t).sum(1)
        return dict(nll=-lpt, lse=t[:, 0] - lpt, t=t[:, 0], rank=rank, best=logits.argmax(1))

    def arm_b():
        return se.score(x, y)

    ta, tb, ma, mb = [], [], 0, 0
    for rep in range(WARM + REPS):
        ms_a, mem_a, out_a = timed(arm_a)
        ms_b, mem_b, out_b = timed(arm_b)
        if rep >= WARM:
            ta.append(ms_a), tb.append(ms_b)
            ma, mb = max(ma, mem_a), max(mb, mem_b)
    # the launches of (b), each between two events
    yi = y.to(torch.int32)
    f = torch.empty(3, R, dtype=torch.float32, device=DEV)
    i = torch.empty(2, R, dtype=torch.int32, device=DEV)
    ws = torch.empty(nl.ws_bytes(R, V), dtype=torch.uint8, device=DEV)
    tt, th = [], []
    for rep in range(WARM + REPS):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        e[0].record()
        nl.target_logit(x, W, b, yi, f[0])
        e[1].record()
        nl.head_nll(x, W, b, yi, f[0], f[1], f[2], i[0], i[1], ws=ws)
        e[2].record()
        torch.cuda.synchronize()
        if rep >= WARM:
            tt.append(e[0].elapsed_time(e[1])), th.append(e[1].elapsed_time(e[2]))
    # rows on which the arms differ beyond the test's bound (E as in tests/score_refs.py, from the 16-bit-rounded operands)
    import score_refs as SR  # noqa: E402
    E = torch.cat([(D + 2) * 2.0 ** -24 * (x[r0: r0 + 2400].to(dtype).double().abs() @ Wv.double().abs() + b.double().abs()).max(1).values
                   for r0 in range(0, R, 2400)])
    fb = 2 * E + (V + 2) * 2.0 ** -24 + SR.EPS_FN
    bad = ((out_a["nll"].double() - out_b["nll"].double()).abs() > fb) | ((out_a["lse"].double() - out_b["lse"].double()).abs() > fb)
    drank = (out_a["rank"] - out_b["rank"].long()).abs()
    say(f"{str(dtype)[6:]}:" + ("" if dtype == torch.float32 or WIDE_OUT else "  ((a)'s GEMM rounds its logits to 16 bits: its own error, counted below)"))
    say(f"  (a) GEMM into [R, V] fp32 + log_softmax + gather + rank count   {med(ta)}    peak allocation {ma / 1e6:.1f} MB")
    say(f"  (b) ScoreEngine.score (target logit + streamed head + merge)    {med(tb)}    peak allocation {mb / 1e6:.1f} MB")
    say(f"      ittl_target_logit {med(tt)};  ittl_head_nll {med(th)} = {2.0 * R * D * V / statistics.median(th) / 1e9:.1f} TFLOP/s")
    say(f"  rows with |nll| or |lse| apart beyond the bound: {int(bad.sum())} of {R}; best differs on {int((out_a['best'] != out_b['best'].long()).sum())}; "
        f"|rank difference| max {int(drank.max())}, rows with any {int((drank > 0).sum())}")
    del se, W, Wv
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as fh:
    fh.write("\n".join(lines) + "\n")
