#!/usr/bin/env python3
"""Microseconds per graph-replayed decode token with a per-row LoRA adapter bank, beside the two forms the engine had before
it (BASELINE config 3 shape: 24 layers, bf16, 32 rows, ~72-position prompt, 140 tokens):
  base    no adapter, "fold" form (5 launches per block)
  single  attach_lora with adapters on the two output projections, "launch" form (7 launches per block)
  bank    attach_lora_bank: n = 8 adapters of rank 16 on all four targets, ids spread over the rows ("launch" form + 4 shrinks)
The arms alternate in ONE process on one box, twice (the first round doubles as the spread check); neither `base` nor `single`
runs any code the bank changed.  Appends to $OUT/lora_bank.txt (OUT defaults to out/ under the repository root).
usage: microbench_lora_bank.py [arm ...]      (default: base single bank; `bank` alone under rocprofv3 --kernel-trace --stats
gives the per-kernel time of lora_shrink_kernel)."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "index-tts-lora_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import torch  # noqa: E402

import weights  # noqa: E402
from indextts.gpt.engine import GPTEngine  # noqa: E402

torch.set_grad_enabled(False)
arms = sys.argv[1:] or ["base", "single", "bank"]
L, D, B, P, NEW = 24, 1280, 32, 72, int(os.environ.get("ITTS_TOKENS", "140"))
N_AD, RANK = 8, 16
gsd = weights.gpt_state_dict(L)
eng = GPTEngine(gsd, L, D, 20, dtype=torch.bfloat16, device="cuda")
g = torch.Generator().manual_seed(1)
prefix = torch.randn(B, P, D, generator=g) * 0.1
pad = torch.zeros(B, dtype=torch.int32)
sp = dict(do_sample=True, top_k=30, top_p=0.8, temperature=1.0, repetition_penalty=10.0, seed=7)


def adapters(targets):
    ad = {}
    for i in range(L):
        for name in targets:
            k_in, n_out = gsd[f"gpt.h.{i}.{name}.weight"].shape
            ad[f"gpt.h.{i}.{name}"] = (torch.randn(RANK, k_in, generator=g) * 0.02, torch.randn(n_out, RANK, generator=g) * 0.02)
    return ad


single = adapters(("attn.c_proj", "mlp.c_proj"))
bank = [(adapters(("attn.c_attn", "attn.c_proj", "mlp.c_fc", "mlp.c_proj")), 2.0) for _ in range(N_AD)]
ids = [(b % (N_AD + 1)) - 1 for b in range(B)]          # every voice and the base voice, each shared by 3-4 rows
OUT = os.path.join(ROOT, os.environ.get("OUT", "out"))
os.makedirs(OUT, exist_ok=True)
out = open(os.path.join(OUT, "lora_bank.txt"), "a")
times = {}
for rep in range(2):
    for arm in arms:
        eng.detach_lora_bank()
        eng.detach_lora()
        if arm == "single":
            eng.attach_lora(single, 2.0)
        elif arm == "bank":
            eng.attach_lora_bank(bank)
        elif arm != "base":
            raise SystemExit(f"unknown arm {arm}")

        def run():
            eng.prefill(prefix, pad, NEW + 2, adapter_ids=ids if arm == "bank" else None)
            torch.cuda.synchronize()
            t = time.perf_counter()
            eng.decode(NEW, sp, force_stop=[NEW - 1] * B)
            torch.cuda.synchronize()
            return t
        run()                                                   # warm-up + capture
        t0 = run()
        us = 1e6 * (time.perf_counter() - t0) / NEW
        times.setdefault(arm, []).append(us)
        form = "fold" if eng._fold_now(B) else "launch"
        line = f"{arm:8s} {form:6s} {us:8.1f} us/token  (round {rep})"
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()
if "bank" in times and "single" in times:
    r = min(times["bank"]) / min(times["single"])
    line = f"bank / single = {r:.3f}  (the issue's reporting line: 1.35)"
    print(line, flush=True)
    out.write(line + "\n")
