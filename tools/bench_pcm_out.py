#!/usr/bin/env python3
"""The PCM output back-end measured: 32 utterances of 6 s (fp32 at 24 kHz on the device, Gaussian at
amplitude 8000) -> 8 kHz mu-law and -> 48 kHz pcm16 in host memory.
Timed region: a host clock from the waveforms on the device to the encoded bytes in host memory, synchronised; median of 9 after
two warm-up rounds; the arms alternate inside one process.
  (a) today's route: device -> host of the fp32 samples, feature_extractors.resample and a numpy encode on the host
  (b) the same torch ops on the device tensors (resample, clamp, truncate, compand with torch ops), then device -> host
  (c) PcmOutEngine.encode: one itto_pcm_out launch for the 32 rows, then device -> host of the encoded samples
Beside them: the kernel alone between two device events behind a queued spin kernel (bench_prompt_frontend.py's method), the
bytes each arm moves off the device, and the cost one stream boundary adds -- PcmOutEngine.push_many over 8 rows of 32 tokens
(8192 samples) each, host clock, synchronised, the state carried from boundary to boundary.
No ratio is fixed in advance: the output is the record.  Writes profiles/pcm_out.txt.
usage: bench_pcm_out.py [--out FILE]"""
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

import pcm_out_refs as R  # noqa: E402
from indextts import _native_out as nato  # noqa: E402
from indextts.utils.feature_extractors import resample  # noqa: E402
from indextts.utils.pcm_out import OutputFormat, PcmOutEngine  # noqa: E402

torch.set_grad_enabled(False)
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pcm_out.txt"))
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("bench_pcm_out.py measures on the GPU: none is visible")
DEV, REPS, WARM, SPIN_CYCLES = torch.device("cuda:0"), 9, 2, 2_000_000
ROWS, SECONDS = 32, 6
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


gen = torch.Generator().manual_seed(23)
waves = [(torch.randn(SECONDS * 24000, generator=gen) * 8000.0).to(DEV) for _ in range(ROWS)]
engine = PcmOutEngine(DEV)
MU_ENDS = torch.tensor(R.MU_ENDS, device=DEV)


def mulaw_torch(s):
    mag = s.abs().clamp(max=R.MU_CLIP) + R.MU_BIAS
    seg = torch.bucketize(mag, MU_ENDS)
    code = torch.where(s < 0, 0x80, 0) | (seg << 4) | ((mag >> (seg + 3)) & 0xF)
    return (~code & 0xFF).to(torch.uint8)


def arm_host(fmt):
    out, moved = [], 0
    for w in waves:
        h = w.cpu()
        moved += h.numel() * 4
        v = resample(h[None], 24000, fmt.sample_rate)[0].numpy()
        p = R.pcm16_of(v)
        out.append(R.mulaw_encode(p) if fmt.encoding == "mulaw" else p)
    return out, moved


def arm_device(fmt):
    out, moved = [], 0
    for w in waves:
        p = resample(w[None], 24000, fmt.sample_rate)[0].clamp(-32767.0, 32767.0).to(torch.int32)
        h = (mulaw_torch(p) if fmt.encoding == "mulaw" else p.to(torch.int16)).cpu()
        moved += h.numel() * h.element_size()
        out.append(h.numpy())
    return out, moved


def arm_hip(fmt):
    out = [o.cpu() for o in engine.encode(waves, fmt)]
    return [o.numpy() for o in out], sum(o.numel() * o.element_size() for o in out)


def timed(fn, fmt):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn(fmt)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


say(f"timing  ({ROWS} rows of {SECONDS} s; host clock, fp32 on the device -> encoded bytes in host memory, synchronised; ms, median of 9 [min .. max])")
for fmt in (OutputFormat(8000, "mulaw"), OutputFormat(48000, "pcm16")):
    arms = [("(a) device -> host, torch resample + numpy encode on the host", arm_host), ("(b) the torch ops on the device, then device -> host", arm_device),
            ("(c) HIP engine, then device -> host", arm_hip)]
    times, outs = {n: [] for n, _ in arms}, {}
    for rep in range(WARM + REPS):
        for n, fn in arms:                       # alternating: every arm once per round
            ms, out = timed(fn, fmt)
            outs[n] = out
            if rep >= WARM:
                times[n].append(ms)
    say(f"  {fmt.sample_rate} Hz {fmt.encoding}:")
    med = {}
    for n, _ in arms:
        t = times[n]
        med[n] = statistics.median(t)
        say(f"    {n}: {med[n]:.3f}  [{min(t):.3f} .. {max(t):.3f}]   {outs[n][1]} bytes off the device")
    c = arms[2][0]
    say(f"    (c) against (a): {med[arms[0][0]] / med[c]:.2f} x; against (b): {med[arms[1][0]] / med[c]:.2f} x")
    for n, _ in arms[:2]:
        diff = sum(int((a != b).sum()) for a, b in zip(outs[n][0], outs[c][0]))
        say(f"    samples of {n[:3]} that differ from (c): {diff} of {sum(a.size for a in outs[c][0])} (conv1d sums in another order)")

say("kernel alone  (the launch between two device events behind a queued spin kernel, no graph; us, median of 9 [min .. max])")
real = nato.pcm_out
for fmt in (OutputFormat(8000, "mulaw"), OutputFormat(48000, "pcm16")):
    spans, per = [], []

    def wrapped(*a):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(SPIN_CYCLES)       # keeps the stream busy while the host enqueues what follows
        e0.record()
        r = real(*a)
        e1.record()
        spans.append((e0, e1))
        return r

    nato.pcm_out = wrapped
    try:
        for rep in range(WARM + REPS):
            spans.clear()
            engine.encode(waves, fmt)
            torch.cuda.synchronize()
            if rep >= WARM:
                per.append(sum(a.elapsed_time(b) for a, b in spans) * 1e3)
    finally:
        nato.pcm_out = real
    n_in = ROWS * SECONDS * 24000
    say(f"  {fmt.sample_rate} Hz {fmt.encoding}: {statistics.median(per):.1f}  [{min(per):.1f} .. {max(per):.1f}]   ({n_in} samples in)")

say("one stream boundary  (push_many over 8 rows of 8192 new samples each, state carried; host clock, synchronised; us, median of 9 [min .. max])")
for fmt in (OutputFormat(8000, "mulaw"), OutputFormat(48000, "pcm16")):
    streams, per = [engine.stream(fmt) for _ in range(8)], []
    for rep in range(WARM + REPS):
        items = [(s, waves[i][rep * 8192:(rep + 1) * 8192], False) for i, s in enumerate(streams)]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        engine.push_many(items)
        torch.cuda.synchronize()
        if rep >= WARM:
            per.append((time.perf_counter() - t0) * 1e6)
    say(f"  {fmt.sample_rate} Hz {fmt.encoding}: {statistics.median(per):.1f}  [{min(per):.1f} .. {max(per):.1f}]")

os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
