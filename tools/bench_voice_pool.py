#!/usr/bin/env python3
"""The voice pool measured, 24 layers, bf16, rank-4 voices on all four targets (rp = 16):
(a) the time to page ONE voice into a bank slot -- every (layer, target): one strided copy of the B-image, one contiguous copy of
    the A-image -- on the stream, between two events; median (min) of `reps` page-ins, each of a voice that is not resident;
(b) the captured step's time per token for a pool engine with S = 8 slots against attach_lora_bank of 8 voices, alternating in one
    process: 8 rows, greedy, the difference of a 136- and a 40-token decode divided by 96 (prefill and capture cancel);
(c) a 64-utterance queue (texts of U{8..60} tokens, stops after U{30..120} codes, seed 3) through infer_queue with 8 decode slots over
    40 voices with S = 8 against the same queue over 8 voices: loads, evictions, deferrals, tokens/s.
No threshold is set: the output is the record.  profiles/voice_pool.txt is this tool's output.
usage: bench_voice_pool.py [reps] [layers] [--out FILE]"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "index-tts-lora_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import synth  # noqa: E402
import weights  # noqa: E402
from indextts.infer import IndexTTS  # noqa: E402
from refill_voices import make_factors  # noqa: E402

torch.set_grad_enabled(False)
ap = argparse.ArgumentParser()
ap.add_argument("reps", nargs="?", type=int, default=9)
ap.add_argument("layers", nargs="?", type=int, default=24)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voice_pool.txt"))
args = ap.parse_args()
reps, layers = max(9, args.reps), args.layers
if not torch.cuda.is_available():
    sys.exit("bench_voice_pool.py measures on the GPU: none is visible")
S, NV = 8, 40
GEN = dict(do_sample=False, num_beams=1, repetition_penalty=10.0)
cfg = weights.reference_config()
cfg["gpt"]["layers"] = layers
sd = weights.gpt_state_dict(layers)
mk = lambda: IndexTTS.from_weights(cfg, sd, weights.bigvgan_state_dict(), device="cuda:0",   # noqa: E731
                                   precision_config={"gpt": "bf16", "vocoder": "fp16"})
voices = make_factors(sd, (4,) * NV, [1.0 + 0.01 * i for i in range(NV)], layers=layers, seed=3)
pooled, banked = mk(), mk()
pooled.attach_voice_pool(voices, slots=S)
banked.gpt.attach_lora_bank(voices[:S])
cond_mel = torch.from_numpy(synth.uniform("in.cond_mel", (1, 100, 120), -6.0, 2.0)).to("cuda")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


med = lambda v: f"{statistics.median(v):.3f} (min {min(v):.3f})"   # noqa: E731
eng = pooled.gpt.engine
say(f"voice pool: {layers} layers, bf16, {NV} voices of rank 4 (rp = 16) on four targets, S = {S} slots; "
    f"{eng.bank.pool.nbytes_per_voice() / 1e6:.1f} MB per voice")

# ---- (a) one page-in
eng._slots(list(range(S)), None)
torch.cuda.synchronize()
ms = []
for i in range(reps + 2):
    v = S + i % (NV - S)                         # never resident: 8 slots, 32 other voices in turn
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    loads = eng.bank.res.acquire([v])
    assert len(loads) == 1
    e0.record()
    eng._page_in(loads)
    e1.record()
    torch.cuda.synchronize()
    ms.append(e0.elapsed_time(e1))
say(f"(a) page-in of one voice ({layers * 4 * 2} copies): {med(ms[2:])} ms on the stream, {reps} page-ins")

# ---- (b) the captured step, pool against bank
rng = np.random.default_rng(11)
rows = torch.from_numpy(rng.integers(2, 12000, size=(8, 40))).to(torch.int32).to("cuda")


def decode_ms(tts, ids, T):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tts.gpt.inference_speech(cond_mel, rows, max_generate_length=T, force_stop=[T - 1] * 8, adapter_ids=ids, **GEN)
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


per = {"pool": [], "bank": []}
for i in range(reps + 2):
    for name, tts, ids in (("pool", pooled, list(range(20, 28))), ("bank", banked, list(range(8)))):
        short, long_ = decode_ms(tts, ids, 40), decode_ms(tts, ids, 136)
        if i >= 2:
            per[name].append(1e3 * (long_ - short) / 96)
say(f"(b) captured step, 8 rows, us per token: pool S = 8 {med(per['pool'])}, attach_lora_bank of 8 {med(per['bank'])} "
    f"(alternating, {reps} pairs; same launches, same arguments: the bank signature is {eng.bank.sig[:2]} in both)")

# ---- (c) a queue over 40 voices against the same queue over 8
rng = np.random.default_rng(3)
texts = [torch.from_numpy(rng.integers(2, 12000, size=int(n))).to(torch.int32) for n in rng.integers(8, 61, size=64)]
stops = [int(v) for v in rng.integers(30, 121, size=64)]
many, few = [int(v) for v in rng.integers(0, NV, size=64)], [int(v) for v in rng.integers(0, S, size=64)]


def queue(ids):
    pooled.detach_voice_pool()
    pooled.attach_voice_pool(voices, slots=S)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    _, codes = pooled.infer_queue(cond_mel, texts, slots=8, max_mel_tokens=160, force_stop=stops, return_codes=True, adapter_ids=ids, **GEN)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    return sum(int(c.numel()) for c in codes) / dt, pooled.gpt.engine.pool_stats()


for name, ids in (("warm-up", few), ("8 voices", few), ("40 voices", many), ("8 voices", few), ("40 voices", many)):
    tps, st = queue(ids)
    if name != "warm-up":
        say(f"(c) 64 utterances, 8 decode slots, S = {S}, {name}: {tps:.0f} tokens/s (GPT + latent + vocoder), {st}")
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
