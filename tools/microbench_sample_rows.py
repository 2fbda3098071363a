#!/usr/bin/env python3
"""Microseconds per graph-replayed decode token with per-row sampling settings beside the scalar form (BASELINE config 3 shape,
as tools/microbench_lora_bank.py sets it up: 24 layers, bf16, 32 rows, ~72-position prompt, 140 tokens):
  scalar   one dict for the batch (itts_sample, sample_kernel<false>: the path the engine had before)
  seeds    32 records with the scalar arm's settings, each with its own seed (itts_sample_rows, sample_kernel<true>): what the
           per-row FORM costs -- the same work per row, the settings fetched from the table
  rows     32 records that differ in every field (greedy rows, top_k 1..1024, top_p, temperature, penalty on / off, own seeds):
           what a MIX of requests costs -- the launch lasts as long as its slowest row, and a top_k = 1024 row sorts and sums
           1024 candidates where top_k = 30 handles about 30
The arms alternate in ONE process, twice (the two rounds show the run-to-run spread).  Appends to $OUT/sample_rows.txt (OUT
defaults to out/ under the repository root).
usage: microbench_sample_rows.py [arm ...]      (one arm alone under rocprofv3 --kernel-trace --stats gives the per-kernel time of
sample_kernel in that form)."""
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
arms = sys.argv[1:] or ["scalar", "seeds", "rows"]
L, D, B, P, NEW = 24, 1280, 32, 72, int(os.environ.get("ITTS_TOKENS", "140"))
eng = GPTEngine(weights.gpt_state_dict(L), L, D, 20, dtype=torch.bfloat16, device="cuda")
g = torch.Generator().manual_seed(1)
prefix = torch.randn(B, P, D, generator=g) * 0.1
pad = torch.zeros(B, dtype=torch.int32)
scalar = dict(do_sample=True, top_k=30, top_p=0.8, temperature=1.0, repetition_penalty=10.0, seed=7)
rows = [dict(do_sample=b % 8 != 0, top_k=(1, 5, 30, 50, 200, 1024)[b % 6], top_p=(0.3, 0.8, 1.0)[b % 3], temperature=0.7 + 0.02 * b,
             repetition_penalty=(10.0, 1.0, 5.0)[b % 3], seed=(1 << 32) + 7 * b, stream=0) for b in range(B)]
seeds = [dict(scalar, seed=(1 << 32) + 7 * b, stream=0) for b in range(B)]
LISTS = {"scalar": scalar, "seeds": seeds, "rows": rows}
OUT = os.path.join(ROOT, os.environ.get("OUT", "out"))
os.makedirs(OUT, exist_ok=True)
out = open(os.path.join(OUT, "sample_rows.txt"), "a")
times = {}
for rep in range(2):
    for arm in arms:
        if arm not in LISTS:
            raise SystemExit(f"unknown arm {arm}")

        def run():
            eng.prefill(prefix, pad, NEW + 2)
            torch.cuda.synchronize()
            t = time.perf_counter()
            eng.decode(NEW, LISTS[arm], force_stop=[NEW - 1] * B)
            torch.cuda.synchronize()
            return t
        run()                                                   # warm-up + capture
        t0 = run()
        us = 1e6 * (time.perf_counter() - t0) / NEW
        times.setdefault(arm, []).append(us)
        line = f"{arm:8s} {us:8.1f} us/token  (round {rep})"
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()
if "scalar" in times and len(times) > 1:
    spread = max(max(v) / min(v) - 1.0 for v in times.values())
    for arm in times:
        if arm != "scalar":
            line = f"{arm} / scalar = {min(times[arm]) / min(times['scalar']):.4f}  (run-to-run spread of an arm: {100 * spread:.2f} %)"
            print(line, flush=True)
            out.write(line + "\n")
